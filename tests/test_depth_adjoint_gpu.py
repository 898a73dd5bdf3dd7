"""GPU: the depth camera's adjoint (csrc/depth_adjoint.hip) through depth_camera.render_depth_diff and experiments.fit_depth.

Bounds are those of tests/test_emu_depth_adjoint.py, whose text derives them: every output within 1e-12 x the sum of its absolute
summands of the restatement tests/depth_adjoint_ref.py at the device's own depth / seg; the masked central difference of the
device's renderer (kept: same seg at theta and theta +- h, cosine >= 0.2, at least 80 % of the body's pixels) within
sum |w| (DC_TAU / (0.2 h) + 1e3 h^2) at h = 1e-4 for analytic bodies and sum |w| (2e-13 / h + 1e3 h^2) at h = 1e-6 for the grid.
torch.autograd.gradcheck is not used: it knows nothing of the kept mask.

fit_depth (2 scenes, 30 Adam iterations, 80 x 60, three cameras): the loss and the radius error end below their start values;
for shape="grid" at 17^3 the loss does.  Measured on the MI355X: see DESIGN.md section 7."""
import numpy as np
import pytest
import torch

import depth_adjoint_ref as A
import depth_camera_ref as ref

pytestmark = pytest.mark.gpu
DC_TAU = 1e-10


def _dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt)


def run(pose, kind, prm, grids, gid, cam, I, w, min_cos=1e-3, want=("pose", "prm", "grid")):
    """render_depth_diff and the backward of sum w depth -> dict(depth, seg, g_pose, g_prm, g_grids, dropped) as numpy."""
    from diffsdfsim_amd import depth_camera
    from diffsdfsim_amd.grids import GridTable
    p, q = _dev(pose).requires_grad_("pose" in want), _dev(prm).requires_grad_("prm" in want)
    gs = [_dev(g).requires_grad_("grid" in want) for g in grids]
    depth, seg, dropped = depth_camera.render_depth_diff(p, _dev(kind, torch.int32), q, cam, I["fx"], I["fy"], I["cx"], I["cy"], (I["W"], I["H"]),
                                                         grids=GridTable(gs, "cuda"), grid_id=gid, min_cos=min_cos, return_dropped=True)
    (depth * _dev(w)).sum().backward()
    return dict(depth=depth.detach().cpu().numpy(), seg=seg.cpu().numpy(), g_pose=None if p.grad is None else p.grad.cpu().numpy(),
                g_prm=None if q.grad is None else q.grad.cpu().numpy(), g_grids=[None if g.grad is None else g.grad.cpu().numpy() for g in gs],
                dropped=dropped.cpu().numpy())


def render(pose, kind, prm, grids, gid, cam, I):
    from diffsdfsim_amd import depth_camera
    d, s = depth_camera.render_depth(_dev(pose), _dev(kind, torch.int32), _dev(prm), cam, I["fx"], I["fy"], I["cx"], I["cy"], (I["W"], I["H"]),
                                     grids=[_dev(g) for g in grids], grid_id=gid)
    return d.cpu().numpy(), s.cpu().numpy()


def compare(got, want, name):
    worst = 0.0
    pairs = [(got["g_pose"], want["g_pose"], want["mag_pose"]), (got["g_prm"][..., :3], want["g_prm"], want["mag_prm"])]
    pairs += [(a, b, m) for a, b, m in zip(got["g_grids"], want["g_grids"], want["mag_grids"])]
    for a, b, mag in pairs:
        err, bound = np.abs(a - b), 1e-12 * mag
        if (mag > 0).any():
            worst = max(worst, float((err[mag > 0] / bound[mag > 0]).max()))
        assert np.all(err <= bound), (name, float(err.max()))
        assert np.all(a[mag == 0] == 0.0), name
    assert np.all(got["g_prm"][..., 3] == 0.0)      # the corner radius / a grid's scale is a constant
    assert np.array_equal(got["dropped"], want["dropped"]), (name, got["dropped"], want["dropped"])
    return worst


@pytest.fixture(scope="module")
def scene():
    pose, kind, prm, grids, gid = A.seam_scene(3, 8)
    cam, I = ref.experiment_camera(), A.intrinsics(80, 60)
    w = np.random.default_rng(4).uniform(-1, 1, (3, 60, 80))
    return pose, kind, prm, grids, gid, cam, I, w, run(pose, kind, prm, grids, gid, cam, I, w)


@pytest.mark.parametrize("min_cos", [1e-3, 0.99])
def test_kernel_matches_the_restatement(scene, min_cos):
    pose, kind, prm, grids, gid, cam, I, w, got = scene
    if min_cos != 1e-3:
        got = run(pose, kind, prm, grids, gid, cam, I, w, min_cos)
    want = A.adjoint(pose, kind, prm, cam, depth=got["depth"], seg=got["seg"], g_depth=w, min_cos=min_cos, grids=grids, grid_id=gid, **I)
    assert all((got["seg"] == b).sum() > 20 for b in range(7)) and not (got["seg"] == 7).any() and (got["seg"][1] < 0).all()
    worst = compare(got, want, "min_cos %g" % min_cos)
    print("min_cos %g: hits per body %s, dropped %s, worst error / (1e-12 x abs-sum) %.4f" %
          (min_cos, [int((got["seg"] == b).sum()) for b in range(8)], got["dropped"].sum(0).tolist(), worst))
    assert np.all(got["g_pose"][1] == 0.0) and np.all(got["g_pose"][:, 7] == 0.0)      # a view of nothing, a body no pixel shows


def test_two_runs_agree_bit_for_bit_except_the_samples(scene):
    pose, kind, prm, grids, gid, cam, I, w, a = scene
    b = run(pose, kind, prm, grids, gid, cam, I, w)
    assert np.array_equal(a["g_pose"], b["g_pose"]) and np.array_equal(a["g_prm"], b["g_prm"]) and np.array_equal(a["dropped"], b["dropped"])
    mag = A.adjoint(pose, kind, prm, cam, depth=a["depth"], seg=a["seg"], g_depth=w, grids=grids, grid_id=gid, **I)["mag_grids"][0]
    assert np.all(np.abs(a["g_grids"][0] - b["g_grids"][0]) <= 1e-12 * mag) and (mag > 0).sum() > 8


def test_forward_bits_and_which_inputs_get_a_gradient(scene):
    pose, kind, prm, grids, gid, cam, I, w, got = scene
    d, s = render(pose, kind, prm, grids, gid, cam, I)
    assert np.array_equal(d, got["depth"]) and np.array_equal(s, got["seg"])
    assert got["g_pose"].shape == (3, 8, 7) and got["g_prm"].shape == (3, 8, 4) and got["g_grids"][0].shape == (9, 9, 9)
    assert np.abs(got["g_pose"]).max() > 0 and np.abs(got["g_prm"]).max() > 0 and np.abs(got["g_grids"][0]).max() > 0
    only = run(pose, kind, prm, grids, gid, cam, I, w, want=("pose",))
    assert only["g_prm"] is None and only["g_grids"][0] is None and np.array_equal(only["g_pose"], got["g_pose"])
    only = run(pose, kind, prm, grids, gid, cam, I, w, want=("grid",))
    assert only["g_pose"] is None and only["g_prm"] is None and only["g_grids"][0] is not None


@pytest.mark.parametrize("name", ["sphere", "rounded", "disc"])
def test_masked_central_differences_of_the_renderer(name):
    pose, kind, prm, grids, gid = A.fd_view(name)
    cam, I = A.camera(8.0), (A.intrinsics(80, 60) if name == "disc" else A.intrinsics(40, 30))
    is_grid = name == "disc"
    h = 1e-6 if is_grid else 1e-4
    per_weight = (2e-13 if is_grid else DC_TAU / 0.2) / h + 1e3 * h * h
    depth, seg = render(pose, kind, prm, grids, gid, cam, I)
    w = np.random.default_rng(2).uniform(-1, 1, depth.shape)
    r0 = A.adjoint(pose, kind, prm, cam, depth=depth, seg=seg, g_depth=w, grids=grids, grid_id=gid, **I)
    body = seg[0] == 1
    comps = [("pose", c) for c in range(7)] + [("prm", c) for c in range(A.LIVE_PRM[name])]
    if is_grid:
        order = np.argsort(-r0["mag_grids"][0].reshape(-1))
        comps += [("sample", int(order[0])), ("sample", int(order[7]))]
    worst = 0.0
    for what, c in comps:
        def at(s):
            ps, pr, gr = pose.copy(), prm.copy(), [g.copy() for g in grids]
            if what == "pose": ps[0, 1, c] += s
            elif what == "prm": pr[0, 1, c] += s
            else: gr[0].reshape(-1)[c] += s
            return render(ps, kind, pr, gr, gid, cam, I)
        (dp, sp), (dm, sm) = at(h), at(-h)
        kept = body & (sp[0] == 1) & (sm[0] == 1) & (r0["cos"][0] >= 0.2)
        assert kept.sum() >= 0.8 * body.sum(), (name, what, c, kept.sum(), body.sum())
        gd = np.where(kept, w[0], 0.0)[None]
        got = run(pose, kind, prm, grids, gid, cam, I, gd)
        mine = got["g_pose"][0, 1, c] if what == "pose" else (got["g_prm"][0, 1, c] if what == "prm" else got["g_grids"][0].reshape(-1)[c])
        want = (gd[0] * (dp[0] - dm[0])).sum() / (2 * h)
        bound = np.abs(gd).sum() * per_weight
        worst = max(worst, abs(mine - want) / bound)
        assert abs(mine - want) <= bound, (name, what, c, mine, want, bound)
    print("%s: %d pixels, worst error / bound %.3f over %d components" % (name, body.sum(), worst, len(comps)))


def test_fit_depth_sphere_lowers_loss_and_radius_error():
    from diffsdfsim_amd import experiments
    tgt, st = np.array([0.8, 1.0]), np.array([1.1, 0.75])
    r = experiments.fit_depth("sphere", tgt, st, max_iter=30, optimizer="Adam", size=(80, 60))
    print("fit_depth sphere: loss %s -> %s, |rad - rad*| %s -> %s, chamfer %s -> %s" %
          (r["loss_start"], r["loss_final"], np.abs(st - tgt), np.abs(r["rad"] - tgt), r["chamfer_start"], r["chamfer_final"]))
    assert np.all(r["loss_final"] < r["loss_start"]) and np.all(np.abs(r["rad"] - tgt) < np.abs(st - tgt))


def test_fit_depth_grid_lowers_the_loss():
    from diffsdfsim_amd import experiments
    tgt, st = np.array([0.8, 1.0]), np.array([1.1, 0.75])
    r = experiments.fit_depth("grid", tgt, st, res=17, max_iter=30, optimizer="Adam", size=(80, 60))
    print("fit_depth grid 17^3: loss %s -> %s, chamfer %s -> %s" % (r["loss_start"], r["loss_final"], r["chamfer_start"], r["chamfer_final"]))
    assert np.all(r["loss_final"] < r["loss_start"]) and r["sdf"].shape == (2, 17, 17, 17)
