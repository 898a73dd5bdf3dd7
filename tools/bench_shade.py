"""Time of the colour camera on the experiment's scene (floor, wall, the unit ball at (0, 5, 0)): 64 views at
640 x 480, the ball moved a little from view to view, three ways in the same run:
  depth            render_depth alone (dss_depth_render);
  colour           render_color with one light and shadows off (dss_depth_render + dss_shade_render);
  colour, shadows  render_color with one light and shadows on.
The same again with the ball as a 128^3 grid sampled from the same sphere's distance (scale 1.5; the block minima are computed
before the timed calls).  Wall clock around each call with a device synchronisation, 2 warm-up and 7 timed calls each: median
(min, max) for the 64 views, launches, the launchers' host reads and render_color's concatenation included.  One chunk holds all
64 views (max_bytes is raised to fit them).  Writes profiles/shade_bench.json.

    python tools/bench_shade.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsdfsim_amd import depth_camera, experiments as X  # noqa: E402
from diffsdfsim_amd import world_abi as abi  # noqa: E402
from diffsdfsim_amd.grids import GridTable  # noqa: E402

dev = torch.device("cuda:0")
N, SCALE, NVIEW = 128, 1.5, 64


def timeit(f, reps=7, warm=2):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
pose = t([[[1.0, 0, 0, 0, 0.0, -0.5, 0.0], [1.0, 0, 0, 0, 5.0, 5.0, 0.0], [1.0, 0, 0, 0, 0.0, 5.0, 0.0]]]).repeat(NVIEW, 1, 1)
pose[:, 2, 5] = torch.linspace(5.0, 1.0, NVIEW, dtype=torch.float64, device=dev)      # the ball comes down to the floor
prm_a = t([[[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], [1.0, 0.0, 0.0, 0.0]]]).repeat(NVIEW, 1, 1)
prm_g = t([[[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], [0.0, 0.0, 0.0, SCALE]]]).repeat(NVIEW, 1, 1)
kind_a = t([[abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_SPHERE]], torch.int32).repeat(NVIEW, 1)
kind_g = t([[abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_GRID]], torch.int32).repeat(NVIEW, 1)
lin = torch.linspace(-1.0, 1.0, N, dtype=torch.float64, device=dev)
gx, gy, gz = torch.meshgrid(lin, lin, lin, indexing="ij")
table = GridTable([torch.sqrt(gx * gx + gy * gy + gz * gz) - 1.0 / SCALE], dev)
table.block_min()
gid = [[-1, -1, 0]] * NVIEW
cam = X.camera_pose()
K = {k: X.CAMERA[k] for k in ("fx", "fy", "cx", "cy")}
colors, lights = [[0.8, 0.8, 0.8], [0.9, 0.6, 0.3], [0.2, 0.3, 0.9]], [([-1.0, 2.0, 1.5], 0.8)]
big = dict(size=X.CAMERA["size"], max_bytes=1 << 32)

row = dict(device=torch.cuda.get_device_name(0), size=list(X.CAMERA["size"]), views=NVIEW, grid=[N, N, N], lights=1)
for name, kind, prm, g in (("analytic", kind_a, prm_a, {}), ("grid", kind_g, prm_g, dict(grids=table, grid_id=gid))):
    depth = lambda: depth_camera.render_depth(pose, kind, prm, cam, size=X.CAMERA["size"], **K, **g)
    plain = lambda: depth_camera.render_color(pose, kind, prm, cam, *K.values(), colors, lights, shadows=False, **big, **g)
    shadow = lambda: depth_camera.render_color(pose, kind, prm, cam, *K.values(), colors, lights, shadows=True, **big, **g)
    (r0, d0, s0), (r1, _, _) = plain(), shadow()
    res = dict(depth_ms=timeit(depth), color_ms=timeit(plain), color_shadows_ms=timeit(shadow), pixels_hit=int((s0 >= 0).sum()),
               pixels_darker_with_shadows=int((r1.to(torch.int32).sum(-1) < r0.to(torch.int32).sum(-1)).sum()))
    res["shade_over_depth"] = (res["color_ms"]["median"] - res["depth_ms"]["median"]) / res["depth_ms"]["median"]
    res["shadow_share_of_frame"] = (res["color_shadows_ms"]["median"] - res["color_ms"]["median"]) / res["color_shadows_ms"]["median"]
    row[name] = res
    print("%s, %d views of 640 x 480: depth %.3f ms (%.3f .. %.3f), colour %.3f ms (%.3f .. %.3f), colour with shadows %.3f ms (%.3f .. %.3f); "
          "%d pixels hit, %d darker with shadows" % (name, NVIEW, *res["depth_ms"].values(), *res["color_ms"].values(),
                                                    *res["color_shadows_ms"].values(), res["pixels_hit"], res["pixels_darker_with_shadows"]))
out = os.path.join(ROOT, "profiles", "shade_bench.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
