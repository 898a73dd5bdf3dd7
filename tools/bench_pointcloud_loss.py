"""Time of one dss_pointcloud_loss call (diffsdfsim_amd.pointcloud._launch: allocation of out and workspace, the launcher's
read-back of shape_type with its stream synchronisation, both kernels) on 64 segments x 20 000 points of rounded boxes, and
of a float64 torch restatement of the same loss with its autograd backward on the same device and inputs.  HIP events,
5 warm-up and 30 timed calls each, median (min, max); the two are checked against each other first.  DESIGN.md section 5.

    python tools/bench_pointcloud_loss.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsdfsim_amd import pointcloud  # noqa: E402

dev = torch.device("cuda:0")
r = np.random.default_rng(0)
nseg, n = 64, 20000
q = r.standard_normal((nseg, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
pose = torch.tensor(np.concatenate([q, r.uniform(-1, 1, (nseg, 3))], 1), device=dev)
prm = torch.tensor(np.concatenate([r.uniform(0.8, 1.4, (nseg, 3)), np.full((nseg, 1), 0.2)], 1), device=dev)
types = torch.full((nseg,), 3, dtype=torch.int32, device=dev)
pts = torch.tensor(r.uniform(-1.0, 1.0, (nseg * n, 3)), device=dev) + pose[:, 4:].repeat_interleave(n, 0)
off = torch.arange(nseg + 1, dtype=torch.int32, device=dev) * n
def kernel():
    return pointcloud._launch(pts, off, n, pose, types, prm)
def quat_R(q):
    r_, i, j, k = q.unbind(1); ts = 2.0 / (q * q).sum(1)
    return torch.stack([1 - ts * (j * j + k * k), ts * (i * j - k * r_), ts * (i * k + j * r_), ts * (i * j + k * r_), 1 - ts * (i * i + k * k),
                        ts * (j * k - i * r_), ts * (i * k - j * r_), ts * (j * k + i * r_), 1 - ts * (i * i + j * j)], 1).reshape(-1, 3, 3)
def torch_ref():
    po, pr = pose.clone().requires_grad_(), prm[:, :3].clone().requires_grad_()
    R = quat_R(po[:, :4])
    d = pts.reshape(nseg, n, 3) - po[:, None, 4:]
    p = torch.einsum("sji,snj->sni", R, d)
    scale = pr.max(1).values * 0.75
    mask = (p.abs() <= scale[:, None, None]).all(2)
    u = p / scale[:, None, None]
    hd = (pr - 0.4) / scale[:, None] / 2
    qq = u.abs() - hd[:, None]
    sdf = (qq.clamp(min=0).norm(dim=2) + qq.max(2).values.clamp(max=0) - 0.2 / scale[:, None]) * scale[:, None]
    loss = (torch.where(mask, sdf, torch.zeros_like(sdf)) ** 2).sum(1)
    g = torch.autograd.grad(loss.sum(), [po, pr])
    return loss, mask.sum(1), g
def timeit(f, reps=30, warm=5):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))
o = kernel(); l, c, g = torch_ref()
print("agreement: loss %.2e count %s gpose %.2e gprm %.2e" % (float((o[:, 0] - l).abs().max() / l.abs().max()), bool((o[:, 1] == c).all()),
      float((o[:, 2:9] - g[0]).abs().max() / g[0].abs().max()), float((o[:, 9:12] - g[1]).abs().max() / g[1].abs().max())))
print("dss_pointcloud_loss 64 x 20000: median %.3f ms (min %.3f max %.3f)" % timeit(kernel))
print("torch restatement fwd+bwd     : median %.3f ms (min %.3f max %.3f)" % timeit(torch_ref))
