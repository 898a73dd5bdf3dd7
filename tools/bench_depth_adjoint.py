"""Time of the differentiable depth camera, render + adjoint, two ways in the same run:
  kernel   depth_camera.render_depth_diff and the backward of sum w depth (dss_depth_render[_grids], then dss_depth_adjoint with its
           host read of the shape types, the zeroing of its outputs and, for a grid, of g_grid; a new GridTable per call as a
           fitting loop makes one);
  torch    the same render (render_depth: torch has no ray caster) and the adjoint restated in float64 torch on the device: per
           body the hit points o + t d_w of its pixels, phi at R(q)^T (x - pos) as torch ops (box, sphere, the trilinear value of a
           grid by gathers), one autograd pass for n_w . d_w = grad_x phi . d_w, the implicit formula k = -w / (n_w . d_w) with
           the cosine rule, and a second autograd pass of sum k phi to the poses, parameters and samples.  A pixel's view row of pose
           and prm is taken by a one-hot product, so that its backward is a product as well: indexing (a sort of 300 000 duplicates)
           and index_select (as many atomic adds into one row) took 200 and 590 ms per call here.  The samples are gathered by
           index_select.
Workloads: 1 and 16 views of 640 x 480 from the experiment's camera of floor, wall and a sphere (the views differ in the sphere's
place), and the same with the sphere as a voxel body of 128^3 samples.  The gradients of the two ways are compared first.
Wall clock around each call with a device synchronisation, 10 warm-up and 100 timed calls, the two ways alternating: median (min,
max).  The adjoint call alone (dss_depth_adjoint on buffers made beforehand, outputs zeroed inside) is timed beside it, 100 calls
back to back between two synchronisations, time per call; so is the render alone.
Writes profiles/depth_adjoint_bench.json (--out: elsewhere).

    python tools/bench_depth_adjoint.py
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
from diffsdfsim_amd import _lib, depth_camera, experiments  # noqa: E402
from diffsdfsim_amd import world_abi as abi  # noqa: E402
from diffsdfsim_amd.grids import GridTable  # noqa: E402

W_, H_ = 640, 480
INTR = (515.0, 515.0, 319.5, 239.5)
SCALE, MIN_COS = 1.5, 1e-3


def workload(nview, grid, dev, seed=0):
    r = np.random.default_rng(seed)
    obj = np.tile([0.9, 0.2, -0.3, 0.1, 0.0, 2.0, 3.0], (nview, 1))
    obj[:, :4] /= np.linalg.norm(obj[0, :4])
    obj[:, 4:] += 0.2 * r.standard_normal((nview, 3))
    pose = np.stack([np.tile([1.0, 0, 0, 0, 0.0, -0.5, 0.0], (nview, 1)), np.tile([1.0, 0, 0, 0, 5.0, 5.0, 0.0], (nview, 1)), obj], 1)
    body = [0.0, 0.0, 0.0, SCALE] if grid else [1.0, 0.0, 0.0, 0.0]
    prm = np.tile([[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0], body], (nview, 1, 1))
    types = np.tile([abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_GRID if grid else abi.SHAPE_SPHERE], (nview, 1))
    lin = torch.linspace(-1.0, 1.0, 128, dtype=torch.float64)
    ball = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), 3).norm(dim=3) - 1.0 / SCALE
    T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return dict(pose=T(pose), prm=T(prm), types=T(types, torch.int32), kinds=types[0].tolist(), cam=experiments.camera_pose(),
                grids=[ball.to(dev)] if grid else None, gid=torch.tensor([[-1, -1, 0]] * nview, dtype=torch.int32) if grid else None,
                w=(torch.rand(nview, H_, W_, dtype=torch.float64, generator=g) * 2.0 - 1.0).to(dev))


def by_kernel(Wl):
    pose, prm = Wl["pose"].clone().requires_grad_(), Wl["prm"].clone().requires_grad_()
    gs = None if Wl["grids"] is None else [g.clone().requires_grad_() for g in Wl["grids"]]
    depth, seg = depth_camera.render_depth_diff(pose, Wl["types"], prm, Wl["cam"], *INTR, size=(W_, H_),
                                                grids=None if gs is None else GridTable(gs, pose.device), grid_id=Wl["gid"], min_cos=MIN_COS)
    (depth * Wl["w"]).sum().backward()
    return pose.grad, prm.grad[..., :3], None if gs is None else gs[0].grad


def _rot(q):
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2.0 / (q * q).sum(1)
    return torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r), s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                        s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], 1).reshape(-1, 3, 3)


def _phi(kind, p, prm, grid):
    if kind == abi.SHAPE_SPHERE:
        return p.norm(dim=1) - prm[:, 0]
    if kind == abi.SHAPE_BOX:
        q = p.abs() - prm[:, :3] / 2
        return q.clamp_min(0.0).norm(dim=1) + q.max(dim=1).values.clamp_max(0.0)
    n = grid.shape[0]
    ind = (p / SCALE + 1.0) * 0.5 * (n - 1)
    c = torch.clamp(torch.floor(ind.detach()), 0, n - 2)
    f, c = ind - c, c.long()
    flat, out = grid.reshape(-1), 0.0
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wt = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out = out + wt * flat.index_select(0, ((c[:, 0] + dx) * n + c[:, 1] + dy) * n + c[:, 2] + dz)
    return out * SCALE


def by_torch(Wl):
    dev = Wl["pose"].device
    pose, prm = Wl["pose"].clone().requires_grad_(), Wl["prm"].clone().requires_grad_()
    grid = None if Wl["grids"] is None else Wl["grids"][0].clone().requires_grad_()
    with torch.no_grad():
        depth, seg = depth_camera.render_depth(pose, Wl["types"], prm, Wl["cam"], *INTR, size=(W_, H_), grids=Wl["grids"], grid_id=Wl["gid"])
        cam = torch.as_tensor(Wl["cam"], dtype=torch.float64, device=dev)
        col, row = torch.meshgrid(torch.arange(W_, device=dev, dtype=torch.float64), torch.arange(H_, device=dev, dtype=torch.float64), indexing="xy")
        nx, ny = (col + 0.5 - INTR[2]) / INTR[0], (row + 0.5 - INTR[3]) / INTR[1]
        dw = torch.stack([nx, -ny, -torch.ones_like(nx)], 2) @ cam[:3, :3].T
        L = torch.sqrt(nx * nx + ny * ny + 1.0)
    total = 0.0
    for b, kind in enumerate(Wl["kinds"]):
        v, r, c = torch.nonzero(seg == b, as_tuple=True)
        if v.numel() == 0:
            continue
        d = dw[r, c]
        x = (cam[:3, 3] + depth[v, r, c][:, None] * d).requires_grad_()
        oh = torch.nn.functional.one_hot(v, pose.shape[0]).to(torch.float64)      # (the view's row by a product: its backward is a product too)
        ps, pr = oh @ pose[:, b], oh @ prm[:, b]
        R = _rot(ps[:, :4])
        p = torch.einsum("nji,nj->ni", R, x - ps[:, 4:])
        phi = _phi(kind, p, pr, grid)
        gx, = torch.autograd.grad(phi.sum(), x, retain_graph=True)
        nd = (gx * d).sum(1)
        cos = nd.abs() / (gx.norm(dim=1) * L[r, c])
        keep = (p.detach().abs() <= (SCALE if kind == abi.SHAPE_GRID else 1e30)).all(1) & (cos >= MIN_COS) & (nd != 0)
        k = torch.where(keep, -Wl["w"][v, r, c] / nd, torch.zeros_like(nd)).detach()
        total = total + (k * phi).sum()
    total.backward()
    return pose.grad, prm.grad[..., :3], None if grid is None else grid.grad


def timeit(fs, reps=100, warm=10):
    for _ in range(warm):
        for f in fs: f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for k, f in enumerate(fs):
            t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts[k].append(1e3 * (time.perf_counter() - t0))
    return [dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for t in ts]


def back_to_back(f, reps=100, warm=10):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def calls_alone(Wl):
    """ms per call of the render and of dss_depth_adjoint on buffers made once (the outputs zeroed inside, as the backward does)."""
    dev = Wl["pose"].device
    nview = Wl["pose"].shape[0]
    table = None if Wl["grids"] is None else GridTable(Wl["grids"], dev)
    render = lambda: depth_camera.render_depth(Wl["pose"], Wl["types"], Wl["prm"], Wl["cam"], *INTR, size=(W_, H_), grids=table, grid_id=Wl["gid"])
    depth, seg = render()
    cam = depth_camera._camera(Wl["cam"], dev)
    L = _lib.lib()
    nbytes = L.dss_depth_adjoint_workspace_bytes(nview, 3, W_, H_)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    ids = None if table is None else table.ids(Wl["gid"], (nview, 3), dev)
    gargs = (None, 0, None, None, None) if table is None else (_lib.ptr(ids), table.ngrid, _lib.ptr(table.off), _lib.ptr(table.dims), _lib.ptr(table.data))

    def adjoint():
        gp, gq = torch.zeros(nview, 3, 7, dtype=torch.float64, device=dev), torch.zeros(nview, 3, 3, dtype=torch.float64, device=dev)
        dr = torch.zeros(nview, 3, dtype=torch.int32, device=dev)
        gg = None if table is None else torch.zeros_like(table.data)
        _lib.check(L.dss_depth_adjoint(nview, 3, _lib.ptr(Wl["pose"]), _lib.ptr(Wl["types"]), _lib.ptr(Wl["prm"]), _lib.ptr(cam), *INTR, W_, H_,
                                       _lib.ptr(depth), _lib.ptr(seg), _lib.ptr(Wl["w"]), MIN_COS, *gargs, _lib.ptr(gp), _lib.ptr(gq),
                                       None if gg is None else _lib.ptr(gg), _lib.ptr(dr), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev)), "dss_depth_adjoint")
    return back_to_back(render), back_to_back(adjoint), [int((seg == b).sum()) for b in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_adjoint_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, nview, grid in (("1 view, sphere", 1, False), ("16 views, sphere", 16, False), ("1 view, 128^3 grid", 1, True), ("16 views, 128^3 grid", 16, True)):
        Wl = workload(nview, grid, dev)
        gk, gt = by_kernel(Wl), by_torch(Wl)
        diff = [float((x - y).abs().max() / y.abs().max().clamp_min(1e-300)) for x, y in zip(gk, gt) if x is not None]
        tk, tt = timeit([lambda: by_kernel(Wl), lambda: by_torch(Wl)])
        render_ms, adjoint_ms, hits = calls_alone(Wl)
        row = dict(workload=name, views=nview, size=[W_, H_], grid=[128] * 3 if grid else None, hits_per_body=hits,
                   max_gradient_difference_over_largest_entry=dict(zip(("pose", "prm", "grid"), diff)), kernel_ms=tk, torch_ms=tt,
                   torch_over_kernel=tt["median"] / tk["median"], render_call_alone_ms=render_ms, adjoint_call_alone_ms=adjoint_ms, timed_calls=100)
        print("%-22s kernel %.3f ms (%.3f .. %.3f)  torch %.3f ms (%.3f .. %.3f)  x%.2f   render alone %.3f ms, adjoint alone %.3f ms   gradients differ by %s"
              % (name, tk["median"], tk["min"], tk["max"], tt["median"], tt["min"], tt["max"], row["torch_over_kernel"], render_ms, adjoint_ms,
                 ", ".join("%.1e" % d for d in diff)))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
