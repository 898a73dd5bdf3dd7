"""Time of the depth camera on the experiment's scene at 640 x 480 (floor, wall, the unit ball at (0, 5, 0)),
two ways in the same run:
  analytic   render_depth with the ball as an analytic sphere (dss_depth_render);
  grid       the same scene with the ball replaced by a 128^3 grid sampled from the same sphere's distance (scale 1.5, as the
             sphere's own query cube), render_depth(..., grids=) (dss_depth_render_grids; the block minima are computed before
             the timed calls, once per table, and timed on their own).
Wall clock around each call with a device synchronisation, 2 warm-up and 7 timed calls each: median (min, max).  The two images
are compared first: same segment outside the silhouette's rim, depth of the ball to the grid's interpolation error.
Writes profiles/depth_grid_bench.json.

    python tools/bench_depth_grid.py
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
N, SCALE = 128, 1.5


def timeit(f, reps=7, warm=2):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
pose = t([[[1.0, 0, 0, 0, 0.0, -0.5, 0.0], [1.0, 0, 0, 0, 5.0, 5.0, 0.0], [1.0, 0, 0, 0, 0.0, 5.0, 0.0]]])
prm_a = t([[[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], [1.0, 0.0, 0.0, 0.0]]])
prm_g = t([[[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], [0.0, 0.0, 0.0, SCALE]]])
kind_a = t([[abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_SPHERE]], torch.int32)
kind_g = t([[abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_GRID]], torch.int32)
lin = torch.linspace(-1.0, 1.0, N, dtype=torch.float64, device=dev)
gx, gy, gz = torch.meshgrid(lin, lin, lin, indexing="ij")
grid = torch.sqrt(gx * gx + gy * gy + gz * gz) - 1.0 / SCALE
cam = X.camera_pose()
gid = [[-1, -1, 0]]

table = GridTable([grid], dev)
t_min = timeit(lambda: setattr(table, "_blk_min", None) or table.block_min())
analytic = lambda: depth_camera.render_depth(pose, kind_a, prm_a, cam, **X.CAMERA)
through_grid = lambda: depth_camera.render_depth(pose, kind_g, prm_g, cam, grids=table, grid_id=gid, **X.CAMERA)
(da, sa), (dg, sg) = analytic(), through_grid()
same = sa == sg
ball = same & (sa == 2)
row = dict(device=torch.cuda.get_device_name(0), size=list(X.CAMERA["size"]), grid=[N, N, N], block=4,
           pixels_of_the_ball=[int((sa == 2).sum()), int((sg == 2).sum())], pixels_with_another_segment=int((~same).sum()),
           max_depth_difference_on_the_ball=float((da - dg)[ball].abs().max()))
ta, tg = timeit(analytic), timeit(through_grid)
row.update(analytic_ms=dict(median=ta[0], min=ta[1], max=ta[2]), grid_ms=dict(median=tg[0], min=tg[1], max=tg[2]),
           block_min_ms=dict(median=t_min[0], min=t_min[1], max=t_min[2]), grid_over_analytic=tg[0] / ta[0])
print("640 x 480, ball as a sphere %.3f ms (%.3f .. %.3f), as a %d^3 grid %.3f ms (%.3f .. %.3f), x%.2f; block minima %.3f ms (%.3f .. %.3f); "
      "ball pixels %s, other segment at %d pixels, depth difference on the ball <= %.2e"
      % (*ta, N, *tg, row["grid_over_analytic"], *t_min, row["pixels_of_the_ball"], row["pixels_with_another_segment"],
         row["max_depth_difference_on_the_ball"]))
out = os.path.join(ROOT, "profiles", "depth_grid_bench.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
