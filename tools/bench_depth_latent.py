"""Time of the last link of the depth camera's gradient to a neural body's latent code, g_latent = sum_i g_grid[i] d f(x_i; z) / d z,
two ways in the same run, on the g_grid that one 640 x 480 view of a 128^3 neural body leaves (floor, wall and the body; the
adjoint of sum w depth with random w, by dss_depth_adjoint):
  compact  igr.igr_grid_adjoint (dss_igr_grid_adjoint: a count over the dense g_grid, scan, compaction of the chunks that carry weight, the
           network over the compacted list, reduction; two host reads), what the backward of igr.igr_lattice_values calls;
  dense    igr.igr_query_list(MODE_LATENT) on all 128^3 nodes and a torch contraction of the same g_grid with the tangents, what
           a user could do before.
Both network shapes (8 x 128 with a latent code of 2 numbers, 8 x 256 with 4; scenes.geometric_init_weights).  The two results are
compared first.  Wall clock around each call with a device synchronisation, 10 warm-up and 100 timed calls, the two ways
alternating: median (min, max).  The whole backward of the view (dss_depth_adjoint, then the compact call, through autograd) is
timed beside it.  Writes profiles/depth_latent_bench.json (--out: elsewhere).

    python tools/bench_depth_latent.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsdfsim_amd import depth_camera, experiments, igr, meshsdf, scenes  # noqa: E402
from diffsdfsim_amd import world_abi as abi  # noqa: E402

W_, H_ = 640, 480
INTR = (515.0, 515.0, 319.5, 239.5)
RES, SCALE = 128, 3.0


def view(dev):
    pose = np.array([[[1.0, 0, 0, 0, 0.0, -0.5, 0.0], [1.0, 0, 0, 0, 5.0, 5.0, 0.0], [0.9, 0.2, -0.3, 0.1, 0.0, 2.0, 3.0]]])
    pose[0, 2, :4] /= np.linalg.norm(pose[0, 2, :4])
    prm = np.array([[[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], [0.0, 0.0, 0.0, SCALE]]])
    T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt)
    g = torch.Generator(device="cpu").manual_seed(0)
    return dict(pose=T(pose), prm=T(prm), types=T([[abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_IGR]], torch.int32), cam=experiments.camera_pose(),
                gid=torch.tensor([[-1, -1, 0]], dtype=torch.int32), w=(torch.rand(1, H_, W_, dtype=torch.float64, generator=g) * 2.0 - 1.0).to(dev))


def render(V, grid):
    return depth_camera.render_depth_diff(V["pose"], V["types"], V["prm"], V["cam"], *INTR, size=(W_, H_), grids=[grid], grid_id=V["gid"])


def timeit(fs, reps=100, warm=10):
    for _ in range(warm):
        for f in fs: f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for k, f in enumerate(fs):
            t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts[k].append(1e3 * (time.perf_counter() - t0))
    return [dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_latent_bench.json"))
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    V, rows = view(dev), []
    pts = meshsdf._grid_cached(RES, dev)
    for name, (width, nlat) in zip(("bob_spot", "shapenet"), igr.SHAPES):
        P = igr.pack_weights(*scenes.geometric_init_weights(0, 0.5, width, nlat), device=dev)
        z = torch.tensor(np.random.default_rng(1).normal(0, 0.1, nlat), dtype=torch.float64, device=dev)
        leaf = igr.igr_lattice_values(z, P, RES).requires_grad_()
        depth, seg = render(V, leaf)
        (depth * V["w"]).sum().backward()
        g_grid = leaf.grad.contiguous()
        hits = int((seg == 2).sum())
        dims = [[RES] * 3]

        def compact():
            return igr.igr_grid_adjoint(g_grid, dims, [0], z[None], P)[0]

        def dense():
            J = igr.igr_query_list(pts, z, P, igr.MODE_LATENT)[1][:, :nlat]
            return g_grid.reshape(-1) @ J

        def whole_backward():
            zz = z.clone().requires_grad_()
            d, _s = render(V, igr.igr_lattice_values(zz, P, RES))
            (d * V["w"]).sum().backward()
            return zz.grad

        c, nodes = igr.igr_grid_adjoint(g_grid, dims, [0], z[None], P, return_nodes=True)
        d = dense()
        diff = float((c[0] - d).abs().max() / d.abs().max())
        tc, td = timeit([compact, dense], a.reps)
        tw, = timeit([whole_backward], max(a.reps // 5, 1), 3)
        row = dict(network=name, width=width, latent=nlat, size=[W_, H_], grid=[RES] * 3, hit_pixels=hits, nonzero_nodes=nodes, nodes=RES ** 3,
                   g_grid_bytes_read_by_count=8 * RES ** 3, max_difference_over_largest_entry=diff, compact_ms=tc, dense_ms=td,
                   dense_over_compact=td["median"] / tc["median"], forward_and_backward_of_the_view_ms=tw, timed_calls=a.reps)
        print("%-9s %d hit pixels, %d of %d nodes   compact %.3f ms (%.3f .. %.3f)  dense %.3f ms (%.3f .. %.3f)  x%.2f   grid + render + "
              "backward %.3f ms   results differ by %.1e" % (name, hits, nodes, RES ** 3, tc["median"], tc["min"], tc["max"], td["median"], td["min"],
                                                             td["max"], row["dense_over_compact"], tw["median"], diff))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
