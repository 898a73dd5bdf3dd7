"""GPU: the depth camera's gradient to a neural body's latent code -- dss_igr_grid_adjoint (csrc/igr_grid_adjoint.hip) on the
device, igr.igr_lattice_values, depth_camera.body_grid(diff=True), experiments.fit_depth("igr") and its command line.

  * the device kernel against the long-double restatement of tests/test_emu_igr_grid_adjoint.py part 1 (tests/implicit_net.py at the
    lattice nodes, contracted with g_grid in long double), on a 13^3 and a 17^3 grid with both networks and the same bound:
    1e-11 sum |g_i| + n eps sum |g_i d f / d z_l|; two runs bit-equal.  256 nodes carry weight (among them the samples on both
    sides of the chunk boundary and the grid's last), the density of what a depth image leaves; the restatement runs once per case.
  * the dense end: every node of 130 grids of 13^3 in one call (full ballots, more than 256 entries per chunk, 260 chunks for the
    scan's carry, two interleaved latent rows, the second call after a capacity that was too small), same restatement and bound.
  * igr_lattice_values: the forward bits are body_grid's; latent.grad of a random linear functional is the raw call's output, for
    one code and for a batch.
  * end to end: one 40 x 30 view of the floor and a neural body at res = 17; z.grad of (w * depth).sum() through
    render_depth_diff(grids=[igr_lattice_values(z)]) against the raw call applied to the g_grid the same render yields for a leaf
    grid, to 1e-12 sum |contributions| (the bound of tests/test_emu_depth_adjoint.py part 2: g_grid comes from fp64 atomics, so the two
    agree to rounding, not in their bits); seg and the depth bits are render_depth's.
  * fit_depth("igr"): 2 scenes, 40 x 30, res = 17, 10 iterations: every scene's data loss ends below its start.
  * `depth --shape igr --net bob_spot --iters 2` exits 0 as a fresh child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_camera_ref as ref
import igr_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTOL, EPS = 1e-11, np.finfo(np.float64).eps
NETS = {"bob_spot": (128, 2, 3), "shapenet": (256, 4, 5)}      # width, latent size, seed
IGR = 6                                                        # DSS_SHAPE_IGR
CAM = dict(fx=515.0 / 16, fy=515.0 / 16, cx=19.5, cy=14.5, size=(40, 30))      # the experiment's 640 x 480 at 1/16 size
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


@functools.lru_cache(None)
def network(name):
    from diffsdfsim_amd import igr, scenes
    width, latent, seed = NETS[name]
    Ws, bs = scenes.geometric_init_weights(seed, 0.5, width, latent)
    return Ws, bs, igr.pack_weights(Ws, bs, DEV)


@functools.lru_cache(None)
def case(name, res):
    """256 weighted nodes of a res^3 grid, the code, and the long-double restatement with its bound (computed once)."""
    Ws, bs, _P = network(name)
    latent = NETS[name][1]
    r = np.random.default_rng(41 + res)
    size = res ** 3
    idx = np.unique(np.concatenate([[0, 2047, 2048, size - 1], r.choice(size, 252, replace=False)]))
    g = np.zeros(size); g[idx] = r.normal(0, 1.0, len(idx))
    z = r.normal(0, 0.1, latent)
    ijk = np.unravel_index(idx, (res, res, res))
    pts = np.stack([np.longdouble(-1) + np.longdouble(2) * i.astype(np.longdouble) / np.longdouble(res - 1) for i in ijk], 1)
    J = H.reference(Ws, bs, pts, z[None], dtype=np.longdouble)[1]
    w = g[idx].astype(np.longdouble)[:, None]
    want = (w * J).sum(0)
    bound = GTOL * np.abs(g).sum() + len(idx) * EPS * np.abs(w * J).sum(0).astype(np.float64)
    return g, z, want, bound


@pytest.mark.parametrize("res", [13, 17])
@pytest.mark.parametrize("name", list(NETS))
def test_device_kernel_matches_the_long_double_restatement(name, res):
    from diffsdfsim_amd import igr
    g, z, want, bound = case(name, res)
    P = network(name)[2]
    out, n = igr.igr_grid_adjoint(dev(g), [[res] * 3], [0], dev(z[None]), P, return_nodes=True)
    again = igr.igr_grid_adjoint(dev(g), [[res] * 3], [0], dev(z[None]), P, cap=n)      # (the capacity at the need)
    got = out[0].cpu().numpy()
    err = np.abs(got - want).astype(np.float64)
    print("%s %d^3: %d nodes, measured / bound %s" % (name, res, n, err / bound))
    assert n == int(np.count_nonzero(g)) and torch.equal(out, again)
    assert np.all(err <= bound) and np.abs(got).min() > 1e-6


NDENSE = 130      # grids of 13^3 = 2197 samples, two chunks each: 260 chunks, more than one tile of the scan's 256


@functools.lru_cache(None)
def dense_case(name):
    """Every node of NDENSE 13^3 grids carries weight; the grids name rows 0 and 1 of a table whose two codes are equal, so one
    long-double Jacobian of the 2197 lattice points serves all of them.  -> g [NDENSE,2197], rows, z, want [2,L], bound [2,L]."""
    Ws, bs, _P = network(name)
    latent, res = NETS[name][1], 13
    r = np.random.default_rng(77)
    g = r.normal(0, 1.0, (NDENSE, res ** 3))
    rows = (r.random(NDENSE) < 0.4).astype(np.int64)
    rows[:2] = (0, 1)
    z = r.normal(0, 0.1, latent)
    ijk = np.unravel_index(np.arange(res ** 3), (res, res, res))
    pts = np.stack([np.longdouble(-1) + np.longdouble(2) * i.astype(np.longdouble) / np.longdouble(res - 1) for i in ijk], 1)
    J = H.reference(Ws, bs, pts, z[None], dtype=np.longdouble)[1]
    want, bound = np.zeros((2, latent), np.longdouble), np.zeros((2, latent))
    for k in (0, 1):
        w = g[rows == k].astype(np.longdouble)[:, :, None]
        want[k] = (w * J[None]).sum((0, 1))
        bound[k] = GTOL * np.abs(g[rows == k]).sum() + w.shape[0] * res ** 3 * EPS * np.abs(w * J[None]).sum((0, 1)).astype(np.float64)
    return g, rows, z, want, bound


@pytest.mark.parametrize("name", list(NETS))
def test_every_node_of_many_grids_matches_the_long_double_restatement(name):
    """The dense end of the seams: full ballots in every iteration of a chunk (the emit kernel's carry), more than 256 entries per
    chunk (the later trips of the reduce kernel's strided loop), 260 chunks (the scan's carry over tiles) and two latent rows that
    interleave in grid order; same restatement and bound as above, two runs bit-equal."""
    from diffsdfsim_amd import igr
    g, rows, z, want, bound = dense_case(name)
    P = network(name)[2]
    args = (dev(g), [[13] * 3] * NDENSE, rows, dev(np.stack([z, z])), P)
    out, n = igr.igr_grid_adjoint(*args, return_nodes=True)      # (the default capacity is too small: the call is made twice)
    again = igr.igr_grid_adjoint(*args, cap=n)
    err = np.abs(out.cpu().numpy() - want).astype(np.float64)
    print("%s: %d nodes of %d grids, measured / bound\n%s" % (name, n, NDENSE, err / bound))
    assert n == NDENSE * 2197 and torch.equal(out, again)
    assert np.all(err <= bound) and float(out.abs().min()) > 1e-6


@pytest.mark.parametrize("name", list(NETS))
def test_lattice_values_forward_bits_and_backward(name):
    from diffsdfsim_amd import depth_camera, igr
    from diffsdfsim_amd.physics3d import SDF3D
    Ws, bs, P = network(name)
    latent, res = NETS[name][1], 13
    r = np.random.default_rng(7)
    lat = torch.tensor(r.normal(0, 0.1, latent), dtype=torch.float64, requires_grad=True)      # (on the host, as the drivers keep it)
    body = SDF3D([0, 0, 0], 1.0, igr.decode_igr(igr.IgrNet(Ws, bs, device=DEV)), [lat], res=res)
    plain, scale = depth_camera.body_grid(body)
    diff, scale_d = depth_camera.body_grid(body, diff=True)
    assert not plain.requires_grad and diff.requires_grad and scale == scale_d == 1.0 and torch.equal(plain, diff.detach())
    w = dev(r.normal(0, 1.0, (res, res, res)) * (r.random((res, res, res)) < 0.1))      # a sparse random linear functional
    (g,) = torch.autograd.grad((w * diff).sum(), lat)
    raw = igr.igr_grid_adjoint(w, [[res] * 3], [0], lat.detach().to(DEV)[None], P)
    assert g.device == lat.device and torch.equal(g, raw[0].cpu()) and float(g.abs().min()) > 1e-6
    # a batch: [B,L] -> [B,res,res,res], one backward call for all grids; each grid's bits are the single form's
    lats = dev(r.normal(0, 0.1, (3, latent))).requires_grad_()
    vals = igr.igr_lattice_values(lats, P, res)
    assert tuple(vals.shape) == (3, res, res, res) and torch.equal(vals[1].detach(), igr.igr_lattice_values(lats[1].detach(), P, res))
    wb = torch.stack([w, 0 * w, w.flip(0)])
    (gb,) = torch.autograd.grad((wb * vals).sum(), lats)
    rawb = igr.igr_grid_adjoint(wb, [[res] * 3] * 3, [0, 1, 2], lats.detach(), P)
    assert torch.equal(gb, rawb) and torch.all(gb[1] == 0.0) and float(gb[[0, 2]].abs().min()) > 1e-6


def test_end_to_end_depth_gradient_reaches_the_latent_code():
    from diffsdfsim_amd import depth_camera, igr
    Ws, bs, P = network("bob_spot")
    res, scale = 17, 3.0      # (seen larger: the unit body covers few pixels at 40 x 30)
    r = np.random.default_rng(9)
    pose = dev(np.array([ref.FLOOR[0], [1.0, 0, 0, 0, 1.0, 3.0, 5.0]])[None])
    kind = np.array([[ref.BOX, IGR]], np.int32)
    prm = dev(np.array([ref.FLOOR[2], [0.0, 0.0, 0.0, scale]])[None])
    cam, ids = ref.experiment_camera(), [[-1, 0]]
    w = dev(r.normal(0, 1.0, (1, 30, 40)))
    z = dev(r.normal(0, 0.1, 2)).requires_grad_()
    depth, seg = depth_camera.render_depth_diff(pose, kind, prm, cam, grids=[igr.igr_lattice_values(z, P, res)], grid_id=ids, **CAM)
    (w * depth).sum().backward()
    # the same render with the value grid as a leaf: its g_grid, carried on by the raw call
    leaf = igr.igr_lattice_values(z.detach(), P, res).requires_grad_()
    depth_l, seg_l = depth_camera.render_depth_diff(pose, kind, prm, cam, grids=[leaf], grid_id=ids, **CAM)
    (w * depth_l).sum().backward()
    want = igr.igr_grid_adjoint(leaf.grad, [[res] * 3], [0], z.detach()[None], P)[0]
    plain_d, plain_s = depth_camera.render_depth(pose, kind, prm, cam, grids=[leaf.detach()], grid_id=ids, **CAM)
    assert torch.equal(depth.detach(), plain_d) and torch.equal(seg, plain_s) and torch.equal(depth_l.detach(), plain_d)
    npix, nodes = int((seg == 1).sum()), int((leaf.grad != 0).sum())
    J = igr.igr_query_list(_lattice(res), z.detach(), P, igr.MODE_LATENT)[1][:, :2]
    bound = 1e-12 * (leaf.grad.reshape(-1, 1) * J).abs().sum(0)
    err = (z.grad - want).abs()
    print("%d pixels of the neural body, %d weighted nodes; z.grad %s, |diff| %s, bound %s" % (npix, nodes, z.grad.tolist(), err.tolist(), bound.tolist()))
    assert npix > 5 and nodes > 8 and float(z.grad.abs().min()) > 1e-6
    assert bool(torch.all(err <= bound))


def _lattice(res):
    from diffsdfsim_amd import meshsdf
    return meshsdf._grid_cached(res, torch.device(DEV))


def test_fit_depth_fits_the_latent_code():
    from diffsdfsim_amd import experiments as X
    P = network("bob_spot")[2]
    r = np.random.default_rng(3)
    target, start = 0.1 * r.standard_normal((2, 2)), 0.1 * r.standard_normal((2, 2))
    out = X.fit_depth("igr", size=(40, 30), res=17, max_iter=10, target_latents=target, start_latents=start, packed=P)
    print("data loss %s -> %s; |latent - target| %s -> %s" % (out["loss_start"], out["loss_final"], np.abs(start - target).max(1),
                                                              np.abs(out["latent"] - target).max(1)))
    assert out["latent"].shape == (2, 2) and len(out["history"]) == 11
    assert np.all(out["loss_final"] < out["loss_start"])


def test_command_line_depth_igr():
    cmd = [sys.executable, "-m", "diffsdfsim_amd.experiments", "depth", "--shape", "igr", "--net", "bob_spot", "--iters", "2", "--scenes", "2",
           "--res", "17"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "depth igr scene 1: loss" in p.stdout and "mean |latent - target|" in p.stdout
