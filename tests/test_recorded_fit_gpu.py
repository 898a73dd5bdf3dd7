"""GPU: the recorded-sequence fit (diffsdfsim_amd/experiments.py: plane_pose, plane_world, run_world_frames,
recorded_trajectory_loss, fit_recorded, synthesize_recording; diffsdfsim_amd/recorded.py) against
tests/golden/recorded_fit.npz, what the reference's optim_pointcloud_real.py computes (tools/gen_recorded_golden.py).

Tolerances: plane poses 1e-12 (a dozen double operations on numbers of order one; acos at 1 - 5e-7 turns 1e-16 into 1e-13);
match_pointcloud's count exact and its loss 1e-5 relative, as test_points_of_the_reference_golden_and_its_loss holds its
golden; the rollout as the project holds rollout_igr_push (tests/test_igr_stepper_gpu.py): trajectory 1e-6,
loss 1e-7, and per leaf max |got - want| < 1e-5 max |want|.

First-frame stage on a synthetic recording: the camera stops at phi <= 1e-10, so every selected point lies within 1e-10 of
the true sphere; with both poses at the truth the loss is dr^2 (to 2 dr 1e-10) and gradient descent with lr 0.1 contracts dr by
1 - 2 * 0.1 per step: dr_k = dr_0 0.8^k, held to 1e-7 for 10 steps (the argument of tests/test_depth_camera_gpu.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "recorded_fit.npz")
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G))


def test_plane_poses_of_the_reference(g):
    from diffsdfsim_amd import experiments as X
    got = X.plane_pose(g["plane_sets"]).numpy()
    err = np.abs(got - g["plane_poses"]).max()
    print("plane poses: max |difference| %.2e" % err)
    assert got.shape == g["plane_poses"].shape and err < 1e-12


def test_normal_parallel_to_up_gives_identity_or_half_turn():
    from diffsdfsim_amd import experiments as X
    got = X.plane_pose(np.array([[0.0, 2.0, 0.0, 0.3], [0.0, -1.0, 0.0, -0.4], [0.0, 1.0, 0.0, 0.0]])).numpy()
    assert np.array_equal(got, [[1, 0, 0, 0, 0, -1.6, 0], [0, 1, 0, 0, 0, -0.9, 0], [1, 0, 0, 0, 0, 0, 0]])


def test_selected_points_and_loss_of_the_reference(g):
    from diffsdfsim_amd import pointcloud, recorded
    pts, off = recorded.select_points(dev(g["cloud_pcs"]), dev(g["cloud_segs"], torch.int32))
    keep = (g["cloud_segs"] == 4) & np.isfinite(g["cloud_pcs"]).all(-1)
    assert list(np.diff(off)) == [int(k.sum()) for k in keep] and np.array_equal(pts.cpu().numpy(), g["cloud_pcs"][keep])
    loss, count = pointcloud.match_pointcloud(pts, off, dev(g["cloud_pose"]), g["cloud_kind"], dev(g["cloud_prm"]))
    print("loss", loss.tolist(), "reference", g["cloud_loss"].tolist())
    assert np.array_equal(count.cpu().numpy(), g["cloud_count"])
    assert (np.abs(loss.cpu().numpy() - g["cloud_loss"]) <= 1e-5 * g["cloud_loss"]).all()
    assert int((g["cloud_segs"][2] == 4).sum()) - int(count[2]) == 3, "the three non-finite points of the last cloud are the ones dropped"


def test_load_recording_reads_the_pickle_layout_and_an_npz(g, tmp_path):
    import pickle
    from diffsdfsim_amd import recorded
    T = len(g["roll_pcs"])
    r = np.random.default_rng(5)
    planes = g["roll_planes"][None] + 1e-3 * r.standard_normal((T, 2, 4))
    grav = np.array([0.0, -9.81, 0.0]) + 1e-2 * r.standard_normal((T, 3))
    raw = dict(pcs=list(g["roll_pcs"]), segs=list(g["roll_segs"].astype(np.int64)), planes=list(planes), grav_dirs=list(grav),
               rgbs=[np.zeros((12, 16, 3), np.uint8)] * T, depths=[])
    with open(tmp_path / "rec.pkl", "wb") as f:
        pickle.dump(raw, f)
    np.savez(tmp_path / "rec.npz", pcs=g["roll_pcs"], segs=g["roll_segs"], planes=planes, grav_dirs=grav)
    for name in ("rec.pkl", "rec.npz"):
        rec = recorded.load_recording(str(tmp_path / name), device=DEV)
        assert rec["pcs"].is_cuda and rec["pcs"].dtype == torch.float64 and rec["segs"].dtype == torch.int32
        assert np.array_equal(rec["pcs"].cpu().numpy(), g["roll_pcs"], equal_nan=True) and np.array_equal(rec["segs"].cpu().numpy(), g["roll_segs"])
        assert np.abs(rec["planes"].cpu().numpy() - planes.mean(0)).max() < 1e-15 and abs(rec["g"] - np.linalg.norm(grav.mean(0))) < 1e-14
        assert (rec["rgbs"] is None) == (name == "rec.npz")
    with pytest.raises(ValueError):
        np.savez(tmp_path / "bad.npz", pcs=g["roll_pcs"], segs=g["roll_segs"])
        recorded.load_recording(str(tmp_path / "bad.npz"), device=DEV)


def _leaves(g):
    leaf = lambda v: torch.tensor(np.asarray(v, np.float64).reshape(1, -1), requires_grad=True)
    return dict(rad=torch.tensor([float(g["roll_rad"])], dtype=torch.float64, requires_grad=True), rot=leaf(g["roll_pose"][:4]), pos=leaf(g["roll_pose"][4:]),
                vel=leaf(g["roll_vel"]), fric=torch.tensor([float(g["roll_fric"])], dtype=torch.float64, requires_grad=True),
                restitution=torch.tensor([float(g["roll_restitution"])], dtype=torch.float64, requires_grad=True))


def _world(g, v, restitution=None):
    from diffsdfsim_amd import experiments as X
    return X.plane_world(v["rad"], g["roll_planes"][None], v["fric"], v["restitution"] if restitution is None else restitution,
                         torch.cat([v["rot"], v["pos"]], 1), v["vel"], float(g["roll_g"]), "sphere", device=DEV)


def test_rollout_loss_and_gradients_of_the_reference(g):
    from diffsdfsim_amd import experiments as X
    v = _leaves(g)
    T = len(g["roll_pcs"])
    traj = X.run_world_frames(_world(g, v), T)
    assert tuple(traj["pose"].shape) == (T - 1, 1, 7) and bool(traj["valid"].all()) and traj["repeated"] == [[]]
    terr = np.abs(traj["pose"][:, 0].detach().cpu().numpy() - g["roll_traj"]).max()
    obs = X.recorded_observations([dict(pcs=dev(g["roll_pcs"]), segs=dev(g["roll_segs"], torch.int32))])
    loss = X.recorded_trajectory_loss(traj, obs, v["rad"], "sphere")
    loss.sum().backward()
    lerr = abs(float(loss[0]) - float(g["roll_loss"]))
    print("trajectory: max |difference| %.2e; loss %.10e vs %.10e (%.2e)" % (terr, float(loss[0]), float(g["roll_loss"]), lerr))
    rows = []
    for k in ("rad", "pos", "rot", "vel", "fric", "restitution"):
        want, got = np.asarray(g["roll_g_" + k], np.float64).reshape(-1), v[k].grad.numpy().reshape(-1)
        rows.append((k, np.abs(got - want).max() / np.abs(want).max(), np.abs(want).max()))
        print("d loss / d %-12s reference max %.3e   max |difference| / that %.2e" % (rows[-1][0], rows[-1][2], rows[-1][1]))
    assert terr < 1e-6
    assert lerr < 1e-7
    assert all(r[1] < 1e-5 for r in rows), rows


def test_detach_2nd_bounce_repeats_the_frames_the_reference_repeats(g):
    from diffsdfsim_amd import experiments as X
    v = _leaves(g)
    T = len(g["roll_pcs"])
    rest = torch.tensor([float(g["roll_detach_restitution"])], dtype=torch.float64)
    traj = X.run_world_frames(_world(g, v, rest), T, detach_2nd_bounce=True)
    assert tuple(traj["pose"].shape) == (T - 1, 1, 7)
    assert len(g["roll_repeated"]) > 0 and traj["repeated"] == [list(g["roll_repeated"])]
    assert np.abs(traj["pose"][:, 0].detach().cpu().numpy() - g["roll_traj_detach"]).max() < 1e-6
    # two recordings of different lengths: the shorter one's entries end with its frames
    v2 = {k: torch.cat([x.detach(), x.detach()]) for k, x in v.items()}
    both = X.plane_world(v2["rad"], g["roll_planes"][None], v2["fric"], torch.cat([rest, rest]), torch.cat([v2["rot"], v2["pos"]], 1), v2["vel"],
                         float(g["roll_g"]), "sphere", device=DEV)
    t2 = X.run_world_frames(both, np.array([T, 7]), detach_2nd_bounce=True)
    assert tuple(t2["pose"].shape) == (T - 1, 2, 7) and t2["valid"].sum(0).tolist() == [T - 1, 6]
    assert float((t2["pose"][:, 0] - traj["pose"][:, 0].detach()).abs().max()) < 1e-12 and float((t2["pose"][:6, 1] - t2["pose"][:6, 0]).abs().max()) < 1e-12
    assert t2["repeated"] == [list(g["roll_repeated"]), [f for f in g["roll_repeated"] if f < 6]]


@pytest.fixture(scope="module")
def synthetic():
    from diffsdfsim_amd import experiments as X
    return X.synthesize_recording(rad=[0.1, 0.08], nframes=4, size=(80, 60), noise=0.0, device=DEV)


def test_synthetic_recording_and_its_statistics(synthetic):
    from diffsdfsim_amd import recorded
    for rec in synthetic:
        assert tuple(rec["pcs"].shape) == (4, 60, 80, 3) and rec["segs"].dtype == torch.int32
        labels = set(torch.unique(rec["segs"]).tolist())
        assert 4 in labels and labels <= {0, 1, 2, 4}
        pts, off = recorded.select_points(rec["pcs"], rec["segs"])
        st = recorded.segment_stats(pts, off)
        c, r = rec["truth"]["pose"][:, 4:], rec["truth"]["rad"]
        x = pts.cpu().numpy()
        for t in range(4):
            on = np.abs(np.linalg.norm(x[off[t]:off[t + 1]] - c[t], axis=1) - r)
            assert off[t + 1] - off[t] > 50 and on.max() < 1e-9, (t, on.max())
        diam = float((st["max"][0] - st["min"][0]).max())
        assert 1.5 * r < diam <= 2 * r + 1e-9


def test_first_frame_stage_contracts_the_radius_error(synthetic):
    from diffsdfsim_amd import experiments as X
    r = np.array([rec["truth"]["rad"] for rec in synthetic])
    p0 = np.array([rec["truth"]["pose"][0] for rec in synthetic]); p1 = np.array([rec["truth"]["pose"][1] for rec in synthetic])
    first, traj = X.fit_recorded(synthetic, "sphere", lr=0.1, max_iter=11, optimize_init_pose=False, fit_trajectory=False,
                                 start_rad=1.3 * r, start_pose0=p0, start_pose1=p1, conv_thresh=0.0, device=DEV)
    assert traj is None and len(first["rad_hist"]) == 11
    for k, rk in enumerate(first["rad_hist"]):
        assert np.abs((rk - r) - 0.3 * r * 0.8 ** k).max() < 1e-7, (k, rk)
    assert np.abs(first["loss_hist"][0] - (0.3 * r) ** 2).max() < 1e-8


def test_fit_recorded_runs_both_stages(synthetic):
    from diffsdfsim_amd import experiments as X
    first, traj = X.fit_recorded(synthetic, "sphere", max_iter=2, device=DEV)
    assert len(first["loss_hist"]) == 2 and len(traj["loss_hist"]) == 2
    assert np.isfinite(first["loss_hist"] + traj["loss_hist"]).all() and (first["loss_hist"][1] < first["loss_hist"][0]).all()
    assert traj["init_vel"].shape == (2, 6) and traj["friction"].shape == (2,) and traj["final_pose"].shape == (2, 7)
    assert np.abs(first["start_rad"] - [0.1, 0.08]).max() < 0.02      # half the bounding box of what the camera sees of the ball
