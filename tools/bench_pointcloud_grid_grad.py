"""Time of the point-cloud loss of voxel-grid segments with its gradient w.r.t. the samples, forward + backward, two ways in the
same run:
  kernel   match_pointcloud on a table whose grids require grad, then backward (dss_pointcloud_loss_grids for the value and the pose
           Jacobian, dss_pointcloud_loss_grids_adjoint for the samples; the zeroing of g_data is inside the timed call);
  torch    the same value and the same sample gradient restated in float64 torch on the device: the 8 corner indices and weights
           per point gathered, the gradient scattered with index_add_ (no pose Jacobian: it does less).
Workloads: 64 segments x 4096 points on 8 grids of 32^3 and of 128^3 (8 scenes seen 8 times); one 640 x 480 segment on a 128^3
grid; the same segment on an 8^3 grid, where 307 200 points add into 512 samples.  The points lie near a unit sphere in a
query cube of half side 1.5, those of the image in scan-line order, so that neighbouring lanes share cells.
Wall clock around each call with a device synchronisation, 10 warm-up and 200 timed calls, the two ways alternating: median (min,
max).  The kernel's figure is that of the whole path a fitting loop runs per iteration: a new GridTable (host work and small
copies), two launches and a host read of the shape types in the forward, the zeroing of g_data and the adjoint.  The adjoint call
alone (dss_pointcloud_loss_grids_adjoint on a table made beforehand: its host read and its one kernel) is timed beside it, 200
calls back to back between two synchronisations, time per call.  The two gradients are compared first.
Writes profiles/pointcloud_grid_grad_bench.json (--out: elsewhere).

    python tools/bench_pointcloud_grid_grad.py
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
from diffsdfsim_amd import pointcloud  # noqa: E402
from diffsdfsim_amd import world_abi as abi  # noqa: E402
from diffsdfsim_amd.grids import GridTable  # noqa: E402

SCALE = 1.5


def workload(nseg, npts, res, ngrid, image, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if image:      # a 640 x 480 patch of the sphere in scan-line order
        a, b = torch.meshgrid(torch.linspace(-1.0, 1.0, 480, dtype=torch.float64), torch.linspace(-1.3, 1.3, 640, dtype=torch.float64), indexing="ij")
        d = torch.stack([torch.cos(a) * torch.sin(b), torch.sin(a), torch.cos(a) * torch.cos(b)], 2).reshape(1, -1, 3)
    else:
        d = torch.randn(nseg, npts, 3, dtype=torch.float64, generator=g)
        d = d / d.norm(dim=2, keepdim=True)
    d = d * (1.0 + 0.02 * torch.randn(d.shape[:2], dtype=torch.float64, generator=g))[..., None]
    q = torch.randn(nseg, 4, dtype=torch.float64, generator=g)
    pose = torch.cat([q / q.norm(dim=1, keepdim=True), torch.randn(nseg, 3, dtype=torch.float64, generator=g)], 1)
    r, i, j, k = pose[:, 0], pose[:, 1], pose[:, 2], pose[:, 3]
    R = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r), 2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r),
                     2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], 1).reshape(nseg, 3, 3)
    pts = (d @ R.transpose(1, 2) + pose[:, None, 4:]).reshape(-1, 3)
    lin = torch.linspace(-1.0, 1.0, res, dtype=torch.float64)
    ball = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), 3).norm(dim=3) - 1.2 / SCALE      # a start grid off the target
    prm = torch.zeros(nseg, 4, dtype=torch.float64)
    prm[:, 3] = SCALE
    n = pts.shape[0] // nseg
    return dict(pts=pts.to(dev), off=np.arange(nseg + 1) * n, pose=pose.to(dev), types=torch.full((nseg,), abi.SHAPE_GRID, dtype=torch.int32),
                prm=prm.to(dev), gid=torch.arange(nseg, dtype=torch.int32) % ngrid, grids=[ball.clone().to(dev).requires_grad_() for _ in range(ngrid)],
                seg=torch.arange(nseg).repeat_interleave(n).to(dev), w=torch.linspace(0.5, 1.5, nseg, dtype=torch.float64).to(dev))


def by_kernel(W):
    for g in W["grids"]:
        g.grad = None
    loss, _ = pointcloud.match_pointcloud(W["pts"], W["off"], W["pose"], W["types"], W["prm"], grids=GridTable(W["grids"], W["pts"].device), grid_id=W["gid"])
    (loss * W["w"]).sum().backward()
    return loss.detach(), torch.cat([g.grad.reshape(-1) for g in W["grids"]])


def by_torch(W):
    table = GridTable([g.detach() for g in W["grids"]], W["pts"].device)
    seg, data = W["seg"], table.data
    q, pos = W["pose"][seg, :4], W["pose"][seg, 4:]
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ts = 2.0 / (q * q).sum(1)
    d = W["pts"] - pos
    p = torch.stack([(1 - ts * (j * j + k * k)) * d[:, 0] + ts * (i * j + k * r) * d[:, 1] + ts * (i * k - j * r) * d[:, 2],
                     ts * (i * j - k * r) * d[:, 0] + (1 - ts * (i * i + k * k)) * d[:, 1] + ts * (j * k + i * r) * d[:, 2],
                     ts * (i * k + j * r) * d[:, 0] + ts * (j * k - i * r) * d[:, 1] + (1 - ts * (i * i + j * j)) * d[:, 2]], 1)
    scale = W["prm"][seg, 3]
    inside = (p.abs() <= scale[:, None]).all(1)
    gid = W["gid"].to(seg.device).long()[seg]
    n = table.dims.long()[gid]
    ind = (p / scale[:, None] + 1.0) * 0.5 * (n - 1)
    c0 = torch.minimum(torch.clamp(torch.floor(ind), min=0.0), (n - 2).to(ind.dtype))
    f, c0 = ind - c0, c0.long()
    base = table.off.long()[gid]
    corners, phi = [], torch.zeros_like(scale)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wt = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                idx = base + ((c0[:, 0] + dx) * n[:, 1] + c0[:, 1] + dy) * n[:, 2] + c0[:, 2] + dz
                corners.append((idx, wt))
                phi = phi + wt * data[idx]
    phi = torch.where(inside, phi * scale, torch.zeros_like(phi))
    loss = torch.zeros(W["pose"].shape[0], dtype=torch.float64, device=seg.device).index_add_(0, seg, phi * phi)
    k = 2.0 * W["w"][seg] * phi * scale
    grad = torch.zeros_like(data)
    for idx, wt in corners:
        grad.index_add_(0, idx, k * wt)
    return loss, grad


def timeit(fs, reps=200, warm=10):
    for _ in range(warm):
        for f in fs: f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for k, f in enumerate(fs):
            t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts[k].append(1e3 * (time.perf_counter() - t0))
    return [dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for t in ts]


def adjoint_alone(W, reps=200, warm=10):
    """ms per call of the adjoint entry point on a table made once (g_data zeroed inside, as the backward pass does)."""
    dev = W["pts"].device
    table = GridTable([g.detach() for g in W["grids"]], dev)
    off, gid, types = torch.as_tensor(W["off"]).to(dev, torch.int32), W["gid"].to(dev), W["types"].to(dev)
    max_len = int(np.diff(W["off"]).max())
    f = lambda: pointcloud._launch_grids_adjoint(W["pts"], off, max_len, W["pose"], types, W["prm"], table.ngrid, table.off, table.dims, table.data, gid, W["w"])
    for _ in range(warm): f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud_grid_grad_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, nseg, npts, res, ngrid, image in (("64 x 4096 on 8 grids of 32^3", 64, 4096, 32, 8, False), ("64 x 4096 on 8 grids of 128^3", 64, 4096, 128, 8, False),
                                                 ("640 x 480 on 128^3", 1, 640 * 480, 128, 1, True), ("640 x 480 on 8^3 (contended)", 1, 640 * 480, 8, 1, True)):
        W = workload(nseg, npts, res, ngrid, image, dev)
        (lk, gk), (lt, gt) = by_kernel(W), by_torch(W)
        top = float(gt.abs().max())
        row = dict(workload=name, segments=nseg, points=int(W["pts"].shape[0]), grid=[res] * 3, grids=ngrid, samples_reached=int((gk != 0).sum()),
                   max_gradient_difference_over_largest_entry=float((gk - gt).abs().max()) / top,
                   max_loss_difference_relative=float(((lk - lt).abs() / lt.abs().clamp_min(1e-300)).max()))
        tk, tt = timeit([lambda: by_kernel(W), lambda: by_torch(W)])
        row.update(kernel_ms=tk, torch_ms=tt, torch_over_kernel=tt["median"] / tk["median"], adjoint_call_alone_ms=adjoint_alone(W), timed_calls=200)
        print("%-32s kernel %.3f ms (%.3f .. %.3f)  torch %.3f ms (%.3f .. %.3f)  x%.2f   adjoint call alone %.3f ms   gradients differ by %.1e of the largest entry"
              % (name, tk["median"], tk["min"], tk["max"], tt["median"], tt["min"], tt["max"], row["torch_over_kernel"], row["adjoint_call_alone_ms"],
                 row["max_gradient_difference_over_largest_entry"]))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
