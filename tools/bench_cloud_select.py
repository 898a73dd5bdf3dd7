"""Time of the front of the recorded point-cloud fit on one recording of T = 90 frames of 640 x 480: recorded.select_points
(count kernel, the scan in torch with its one read-back, emit kernel) and recorded._stats (both kernels, allocation of out
and workspace), and of the torch formulation of the same work on the same device and inputs: `pcs[t][segs[t] == 4]` per frame
and mean / min / max of each frame's points, as optim_pointcloud_real.py:326-331 and :499 write it.  HIP events around each
call, 3 warm-up and 20 timed calls each, median (min, max); the two are checked against each other first.  A tenth of the
pixels carry the label (a ball seen from near by), 0.1 % of those have a NaN coordinate.  DESIGN.md section 4.

    python tools/bench_cloud_select.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsdfsim_amd import recorded  # noqa: E402

dev = torch.device("cuda:0")
T, H, W = 90, 480, 640
gen = torch.Generator(device=dev); gen.manual_seed(0)
pcs = torch.rand(T, H, W, 3, dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
segs = torch.where(((yy - 240) ** 2 + (xx - 320) ** 2 < 99 ** 2)[None].expand(T, -1, -1), 4, 1).to(torch.int32).contiguous()
bad = (torch.rand(T, H, W, device=dev, generator=gen) < 1e-3) & (segs == 4)
pcs[..., 1] = torch.where(bad, torch.full_like(pcs[..., 1], float("nan")), pcs[..., 1])


def kernels_select():
    return recorded.select_points(pcs, segs)


def torch_select():
    keep = (segs == 4) & torch.isfinite(pcs).all(dim=3)
    return [pcs[t][keep[t]] for t in range(T)]


pts, off = kernels_select()


def kernels_stats():
    return recorded._stats(pts, off)


frames = torch_select()


def torch_stats():
    return torch.stack([torch.cat([p.mean(dim=0), p.min(dim=0)[0], p.max(dim=0)[0]]) for p in frames])


def timeit(f, reps=20, warm=3):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


o, ref = kernels_stats(), torch_stats()
print("agreement: points equal %s, offsets equal %s, mean %.2e, min / max equal %s" % (
    torch.equal(pts, torch.cat(frames)), list(off[1:]) == list(np.cumsum([len(p) for p in frames])),
    float((o[:, 1:4] / o[:, :1] - ref[:, :3]).abs().max()), torch.equal(o[:, 4:], ref[:, 3:])))
print("%d frames of %d x %d, %d points selected" % (T, W, H, len(pts)))
print("select, kernels (count + scan + emit): median %.3f ms (min %.3f max %.3f)" % timeit(kernels_select))
print("select, torch boolean indexing       : median %.3f ms (min %.3f max %.3f)" % timeit(torch_select))
print("stats, kernels                       : median %.3f ms (min %.3f max %.3f)" % timeit(kernels_stats))
print("stats, torch per-frame mean/min/max  : median %.3f ms (min %.3f max %.3f)" % timeit(torch_stats))
