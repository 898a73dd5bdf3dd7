"""GPU: the Python layer over dss_pointcloud_loss_igr -- pointcloud.match_pointcloud with neural segments, SDF3D.pointcloud_loss,
the neural estimate of the experiment losses and fit_pointcloud_latent.  The kernel itself is pinned by
tests/test_pointcloud_loss_igr_gpu.py; here the routing is: analytic and grid rows are the bits of the calls without neural
segments, neural rows the bits of the direct entry point, backward is g . Jacobian."""
import os

import numpy as np
import pytest
import torch

import igr_helpers as H
import pointcloud_igr_cases as C

pytestmark = pytest.mark.gpu
GRID_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pointcloud_loss_grid.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def packed():
    from diffsdfsim_amd import igr
    return {k: igr.pack_weights(*C.weights(k), device=DEV) for k in (0, 1)}


@pytest.fixture(scope="module")
def mixed(packed):
    """Box, grid and rounded-box segments of the grid golden interleaved with three neural segments of network 0."""
    from diffsdfsim_amd.engine import TorchBackend
    from diffsdfsim_amd.grids import GridTable
    gg, gn = dict(np.load(GRID_GOLDEN)), C.golden()
    names = [str(n) for n in gg["names"]]
    other = [names.index(n) for n in ("box", "torus_257", "rounded")]
    neural = C.named(0, ["mixed_257", "pair_a", "pair_b"])
    order = [("n", neural[0]), ("o", other[0]), ("o", other[1]), ("n", neural[1]), ("n", neural[2]), ("o", other[2])]
    pts, off, pose, types, prm, gid, lid = [], [0], [], [], [], [], []
    for kind, s in order:
        g = gn if kind == "n" else gg
        x = g["pts"][g["seg_off"][s]:g["seg_off"][s + 1]]
        pts.append(x); off.append(off[-1] + len(x)); pose.append(g["pose"][s])
        types.append(6 if kind == "n" else int(gg["shape_type"][s]))
        prm.append([0, 0, 0, gn["scale"][s]] if kind == "n" else gg["prm"][s])
        gid.append(-1 if kind == "n" else int(gg["grid_id"][s]))
        lid.append(int(gn["lat_row"][s]) if kind == "n" else -1)
    t = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    is_n = np.array([k == "n" for k, _ in order])
    back = TorchBackend(DEV)
    direct = C.launch(back, H.packed_on(back, *C.weights(0)), 0, neural)      # [3][13], the bare entry point
    return dict(pts=t(np.concatenate(pts)), off=np.array(off), pose=t(pose), types=np.array(types, np.int32), prm=t(prm), gid=np.array(gid),
                lid=np.array(lid), is_n=is_n, table=GridTable([gg["grid_0"], gg["grid_1"]], torch.device(DEV)), latent=t(gn["latents_0"]),
                direct=torch.tensor(direct, device=DEV))


def _subset(m, keep):
    rows = np.concatenate([np.arange(m["off"][i], m["off"][i + 1]) for i in np.nonzero(keep)[0]])
    lens = np.diff(m["off"])[keep]
    return m["pts"][torch.as_tensor(rows, device=DEV)], np.concatenate([[0], np.cumsum(lens)])


def test_mixed_segments_rows_and_backward(mixed, packed):
    from diffsdfsim_amd import pointcloud
    m = mixed
    o = ~m["is_n"]
    po, oo = _subset(m, o)
    today = pointcloud._launch(po.contiguous(), torch.as_tensor(oo, dtype=torch.int32, device=DEV), int(np.diff(oo).max()), m["pose"][o].contiguous(),
                               torch.as_tensor(m["types"][o], device=DEV), m["prm"][o].contiguous(), m["table"],
                               m["table"].ids(m["gid"][o], (int(o.sum()),), torch.device(DEV)))
    pose, prm, lat = m["pose"].clone().requires_grad_(), m["prm"].clone().requires_grad_(), m["latent"].clone().requires_grad_()
    loss, count = pointcloud.match_pointcloud(m["pts"], m["off"], pose, m["types"], prm, grids=m["table"], grid_id=m["gid"], igr=packed[0],
                                              latent=lat, latent_id=m["lid"])
    n = torch.as_tensor(m["is_n"], device=DEV)
    assert torch.equal(loss[~n], today[:, 0]) and torch.equal(count[~n], today[:, 1])
    assert torch.equal(loss[n], m["direct"][:, 0]) and torch.equal(count[n], m["direct"][:, 1]) and not count.requires_grad
    w = torch.linspace(0.5, 2.0, loss.numel(), dtype=torch.float64, device=DEV)
    (loss * w).sum().backward()
    assert torch.equal(pose.grad[~n], w[~n][:, None] * today[:, 2:9]) and torch.equal(pose.grad[n], w[n][:, None] * m["direct"][:, 2:9])
    assert torch.equal(prm.grad[~n][:, :3], w[~n][:, None] * today[:, 9:12]) and bool((prm.grad[n] == 0).all()) and bool((prm.grad[:, 3] == 0).all())
    want = torch.zeros_like(lat).index_add_(0, torch.as_tensor(m["lid"][m["is_n"]], device=DEV), w[n][:, None] * m["direct"][:, 9:11])
    assert torch.equal(lat.grad, want) and bool((lat.grad[1:] != 0).all())


def test_only_neural_segments_and_the_value_error_paths(mixed, packed):
    from diffsdfsim_amd import pointcloud
    m = mixed
    pn, on = _subset(m, m["is_n"])
    n = torch.as_tensor(m["is_n"], device=DEV)
    args = (pn, on, m["pose"][n], m["types"][m["is_n"]], m["prm"][n])
    loss, count = pointcloud.match_pointcloud(*args, igr=packed[0], latent=m["latent"], latent_id=m["lid"][m["is_n"]])
    assert torch.equal(loss, m["direct"][:, 0]) and torch.equal(count, m["direct"][:, 1])
    kw = dict(igr=packed[0], latent=m["latent"], latent_id=m["lid"][m["is_n"]])
    for missing in kw:
        with pytest.raises(ValueError, match=missing + "="):
            pointcloud.match_pointcloud(*args, **{k: v for k, v in kw.items() if k != missing})
    with pytest.raises(ValueError, match="latent_id"):
        pointcloud.match_pointcloud(*args, **dict(kw, latent_id=[0, -1, 1]))
    with pytest.raises(ValueError, match="latent"):
        pointcloud.match_pointcloud(*args, **dict(kw, latent=m["latent"][:, :1].contiguous()))


@pytest.mark.parametrize("k", [0, 1])
def test_sdf3d_pointcloud_loss_is_the_goldens_first_segment(k):
    from diffsdfsim_amd import igr
    from diffsdfsim_amd.physics3d import SDF3D
    g = C.golden()
    s = C.segments_of(k)[0]
    assert g["names"][s] == "mixed_257"
    L = C.latent_size(k)
    pose = torch.tensor(g["pose"][s], dtype=torch.float64, requires_grad=True)
    lat = torch.tensor(g["latents_%d" % k][g["lat_row"][s]], dtype=torch.float64, requires_grad=True)
    body = SDF3D(pose, float(g["scale"][s]), igr.decode_igr(igr.IgrNet(*C.weights(k), device=DEV)), [lat], res=16)
    loss, count = body.pointcloud_loss(g["pts"][g["seg_off"][s]:g["seg_off"][s + 1]])
    loss.backward()
    got = np.concatenate([[float(loss.detach()), float(count)], pose.grad.numpy(), lat.grad.numpy(), np.zeros(4 - L)])
    assert got[1] == g["out"][s, 1] and np.all(np.abs(got - g["out"][s]) <= C.bound(s)), (got, g["out"][s])


@pytest.fixture(scope="module")
def fit_setup(packed):
    r = np.random.default_rng(3)
    return 0.1 * r.standard_normal((2, 2)), 0.1 * r.standard_normal((2, 2))


def test_fit_pointcloud_latent_first_frame_stage(packed, fit_setup):
    from diffsdfsim_amd import experiments
    tgt, st = fit_setup
    res = experiments.fit_pointcloud_latent(tgt, st, packed[0], run_time=0.1, max_iter=10, fit_trajectory=False, res=32)
    h = res["history"]["frame"]
    assert len(h) == 10
    print("first-frame loss per scene: %s -> %s" % (h[0]["loss"], h[-1]["loss"]))
    assert np.all(h[-1]["loss"] < h[0]["loss"])
    for e in h:
        assert np.all(np.isfinite(e["grad"])) and np.all(np.abs(e["grad"]).max(axis=1) > 0)


def test_fit_pointcloud_latent_trajectory_stage_one_iteration(packed, fit_setup):
    """bounce_world_latent + run_world_fixed_dt + pointcloud_trajectory_loss compose with the latent attached to the world and to
    the loss, and the latent's gradient is finite and non-zero.  The loss's own path is taken alone too (world built from the
    detached code).  In 0.1 s the thrown body touches nothing, so the stepper's path carries an exact zero here and the two agree;
    a run long enough to reach the wall is an experiment, not a test of seconds."""
    from diffsdfsim_amd import experiments as E
    tgt, st = fit_setup
    res = E.fit_pointcloud_latent(tgt, st, packed[0], run_time=0.1, max_iter=1, fit_first_frame=False, res=32)
    g_all = res["history"]["trajectory"][0]["grad"]
    assert np.all(np.isfinite(g_all)) and np.all(np.abs(g_all).max(axis=1) > 0)
    obs = res["observations"]
    lat = torch.tensor(st, dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        world = E.bounce_world_latent(lat.detach(), packed[0], run_time=0.1, res=32)
        traj = E.run_world_fixed_dt(world, 0.1)
    loss = E.pointcloud_trajectory_loss(traj, obs, None, "igr", packed=packed[0], latent=lat) + 1e-4 * (lat.to(DEV) ** 2).sum(dim=1)
    loss.sum().backward()
    g_loss = lat.grad.numpy()
    assert np.all(np.isfinite(g_loss)) and np.all(np.abs(g_loss).max(axis=1) > 0)
    print("latent gradient: through the loss alone %s, whole composition %s" % (g_loss, g_all))
    assert np.allclose(loss.detach().cpu().numpy(), res["history"]["trajectory"][0]["loss"], rtol=1e-9)      # the same forward value
