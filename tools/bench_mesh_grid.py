"""Time of the mesh voxeliser (mesh_grid.mesh_grid_sdf, csrc/mesh_grid.hip) against a float64 torch restatement on the same
device and the same inputs, alternating, one workload after the other:
  grids of 32^3, 64^3 and 128^3 samples (scale 1) x octaspheres of radius 0.6 with 2 048 (k = 4) and 32 768 (k = 6) faces.
  kernel   one dss_mesh_grid_sdf call on device tensors (check=False), with the read-back of its status word;
  torch    the restatement of tests/mesh_grid_ref.py in torch ops: plane foot or the least of three segment distances, the
           solid-angle atan2, [samples, faces] blocks of at most 2^26 elements so it fits memory, the faces in chunks.
Wall clock around each call with a device synchronisation: 3 warm-up and 20 timed calls, median (min, max).  A side whose
first call takes more than 2 s is given that one warm-up and 3 timed calls instead, more than 20 s that one and 1 timed call, so
that the whole run stays within minutes; the row says how many it had.  The two first results are compared (max |difference| /
scale, signs).
pairs/s is set against the fp64 vector peak of the MI355X, 78.6 TFLOP/s = 39.3e12 fp64 VALU lane-operations/s (a fused
multiply-add counted once), through the kernel's fp64 operations per sample-face pair (OPS_PER_PAIR: counted in the regular
path of the compiled inner loop).  Writes profiles/mesh_grid_bench.json.

    python tools/bench_mesh_grid.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_grid_ref as ref  # noqa: E402
from diffsdfsim_amd import mesh_grid  # noqa: E402

dev = torch.device("cuda:0")
PEAK_OPS = 39.3e12      # fp64 VALU lane-operations per second
OPS_PER_PAIR = 235      # fp64 operations per pair in the kernel's regular path
BLOCK = 1 << 26


def dot(a, b):
    return (a * b).sum(-1)


def segment(p, a, b):
    e = b - a
    t = (dot(p - a, e) / dot(e, e)).clamp(0.0, 1.0)
    return (p - a - t[..., None] * e).norm(dim=-1)


def torch_grid(verts, faces, res, scale):
    ax = scale * (-1.0 + 2.0 * torch.arange(res, dtype=torch.float64, device=dev) / (res - 1))
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), 3).reshape(-1, 3)
    out = torch.empty(pts.shape[0], dtype=torch.float64, device=dev)
    fc = max(1, min(faces.shape[0], BLOCK // min(pts.shape[0], 1 << 21)))
    rows = max(1, BLOCK // fc)
    for lo in range(0, pts.shape[0], rows):
        p = pts[lo:lo + rows, None, :]
        best = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=dev)
        ang = torch.zeros(p.shape[0], dtype=torch.float64, device=dev)
        for f0 in range(0, faces.shape[0], fc):
            f = faces[f0:f0 + fc]
            a, b, c = verts[f[:, 0]][None], verts[f[:, 1]][None], verts[f[:, 2]][None]
            n = torch.cross(b - a, c - a, dim=-1)
            nn = dot(n, n)
            h = dot(p - a, n) / nn
            foot = p - h[..., None] * n
            inside = (dot(torch.cross((b - a).expand_as(foot), foot - a, dim=-1), n) >= 0) & \
                     (dot(torch.cross((c - b).expand_as(foot), foot - b, dim=-1), n) >= 0) & \
                     (dot(torch.cross((a - c).expand_as(foot), foot - c, dim=-1), n) >= 0)
            edges = torch.minimum(torch.minimum(segment(p, a, b), segment(p, b, c)), segment(p, c, a))
            d = torch.where(inside, dot(p - a, n).abs() / nn.sqrt(), edges)
            best = torch.minimum(best, d.min(1).values)
            A, B, C = a - p, b - p, c - p
            la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
            num = dot(A, torch.cross(B, C, dim=-1))
            den = la * lb * lc + dot(A, B) * lc + dot(B, C) * la + dot(C, A) * lb
            ang = ang + torch.atan2(num, den).sum(1)
        w = ang / (2.0 * np.pi)
        out[lo:lo + rows] = torch.where(w > 0.5, -best, best) / scale
    return out.reshape(res, res, res)


def timeit(f):
    """-> (the first call's result, the times)"""
    t0 = time.perf_counter(); res = f(); torch.cuda.synchronize(); first = time.perf_counter() - t0
    warm, reps = (1, 1) if first > 20.0 else ((1, 3) if first > 2.0 else (3, 20))
    for _ in range(warm - 1): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    return res, dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), warm_up=warm, timed=reps)


rows = []
for k in (4, 6):
    v, f = ref.octasphere(k)
    vd, fd = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    for res in (32, 64, 128):
        kernel = lambda: mesh_grid.mesh_grid_sdf([vd], [fd], (res, res, res), 1.0, check=False)[0]
        restated = lambda: torch_grid(vd, fd, res, 1.0)
        (a, tk), (b, tt) = timeit(kernel), timeit(restated)
        diff, signs = float((a - b).abs().max()), int(((a < 0) != (b < 0)).sum())
        pairs = res ** 3 * len(f)
        rate = pairs / (1e-3 * tk["median"])
        rows.append(dict(grid=res, faces=len(f), pairs=pairs, workgroups=-(-res ** 3 // 256), max_abs_difference=diff, sign_differences=signs,
                         kernel_ms=tk, torch_ms=tt, speedup=tt["median"] / tk["median"], kernel_wins=bool(tk["median"] < tt["median"]),
                         pairs_per_s=rate, fraction_of_fp64_vector_peak=rate * OPS_PER_PAIR / PEAK_OPS))
        print("%3d^3 x %5d faces  kernel %10.3f ms (%.3f .. %.3f, %d calls)  torch %10.3f ms (%.3f .. %.3f, %d calls)  x%.1f  %.3g pairs/s = %.2f "
              "of the fp64 vector peak  |diff| %.1e, %d signs" % (res, len(f), tk["median"], tk["min"], tk["max"], tk["timed"], tt["median"], tt["min"],
                                                                 tt["max"], tt["timed"], rows[-1]["speedup"], rate, rows[-1]["fraction_of_fp64_vector_peak"], diff, signs),
              flush=True)
out = os.path.join(ROOT, "profiles", "mesh_grid_bench.json")
with open(out, "w") as fh:
    json.dump(dict(device=torch.cuda.get_device_name(0), tile=mesh_grid.TILE, fp64_ops_per_pair=OPS_PER_PAIR, peak_fp64_valu_ops_per_s=PEAK_OPS,
                   neural_marching_cubes_mesh="not measured: no 128^3 neural value grid was at hand", rows=rows), fh, indent=1)
print("wrote", out)
