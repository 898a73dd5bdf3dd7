"""GPU: the depth camera (diffsdfsim_amd/depth_camera.py over csrc/depth_camera.hip) against the float64 oracle of
tests/depth_camera_ref.py, the reference's own selection (tests/golden/depth_camera_points.npz), and through the experiment
layer.  Scenes, checks and tolerances are those of tests/test_emu_depth_camera.py (derived there); in addition one 640 x 480
view of the experiment's scene at t = 0.  On that view the eroded segment has lost the sphere's rim pixel, so every point left
was hit at cosine >= 0.27 and lies within tau / 0.27 = 4e-10 of the sphere: | |x - c| - r | < 1e-8; an estimate of radius
r + 0.3 at the true pose then has loss 0.3^2 = 0.09 (to 2 * 0.3 * 4e-10 < 1e-8), and gradient descent with lr = 0.1 on
loss = dr^2 contracts dr by 1 - 2 * 0.1 per step: dr_k = 0.3 * 0.8^k (to 1e-7)."""
import os

import numpy as np
import pytest
import torch

import depth_camera_ref as ref

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "depth_camera_points.npz")
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def render(pose, kind, prm, cam, fx, fy, cx, cy, W, H):
    from diffsdfsim_amd import depth_camera
    depth, seg = depth_camera.render_depth(dev(pose), dev(kind, torch.int32), dev(prm), cam, fx, fy, cx, cy, size=(W, H))
    return depth, seg


@pytest.fixture(scope="module")
def views():
    pose, kind, prm = ref.bounce_views()
    cam = ref.experiment_camera()
    depth, seg = render(pose, kind, prm, cam, **ref.SMALL)
    return pose, kind, prm, cam, depth, seg


@pytest.fixture(scope="module")
def full_view():
    """The experiment's scene at t = 0 (floor, wall, the unit sphere at (0, 5, 0)) at 640 x 480, and the oracle's images."""
    pose = np.array([ref.FLOOR[0], ref.WALL[0], [1.0, 0, 0, 0, 0.0, 5.0, 0.0]])
    kind = np.array([ref.BOX, ref.BOX, ref.SPHERE], np.int32)
    prm = np.array([ref.FLOOR[2], ref.WALL[2], [1.0, 0, 0, 0]])
    cam = ref.experiment_camera()
    depth, seg = render(pose[None], kind[None], prm[None], cam, **ref.FULL)
    return pose, kind, prm, cam, depth, seg, ref.render(pose, kind, prm, cam, **ref.FULL)


@pytest.mark.parametrize("v", range(4))
def test_rendered_view_matches_the_oracle(views, v):
    pose, kind, prm, cam, depth, seg = views
    want = ref.render(pose[v], kind[v], prm[v], cam, **ref.SMALL)
    ref.check_view(depth[v].cpu().numpy(), seg[v].cpu().numpy(), want, pose[v], kind[v], prm[v], cam, name="view %d" % v, **ref.SMALL)


def test_object_behind_the_wall_is_not_seen_and_calls_repeat(views):
    pose, kind, prm, cam, depth, seg = views
    assert not bool((seg[4] == 2).any()) and bool((seg[4] == 1).any()) and bool((seg != -2).all())
    d2, s2 = render(pose, kind, prm, cam, **ref.SMALL)
    assert torch.equal(d2, depth) and torch.equal(s2, seg)


@pytest.mark.parametrize("kind", [4, 5, 6, 7])
def test_unsupported_types_raise_and_leave_the_outputs_alone(kind):
    from diffsdfsim_amd import _lib, depth_camera
    pose, types, prm = ref.bounce_views()
    types = types[:2].copy(); types[1, 2] = kind
    with pytest.raises(_lib.HipLibraryError, match="boxes, spheres, cylinders and rounded boxes"):
        render(pose[:2], types, prm[:2], ref.experiment_camera(), **ref.SMALL)
    depth = torch.full((2, 60, 80), -7.0, dtype=torch.float64, device=DEV)
    seg = torch.full((2, 60, 80), -7, dtype=torch.int32, device=DEV)
    p, t, q, c = dev(pose[:2]), dev(types, torch.int32), dev(prm[:2]), dev(ref.experiment_camera())
    rc = _lib.lib().dss_depth_render(2, 3, _lib.ptr(p), _lib.ptr(t), _lib.ptr(q), _lib.ptr(c), 64.375, 64.375, 39.5, 29.5, 80, 60, 0.1, 100.0,
                                     _lib.ptr(depth), _lib.ptr(seg), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc != 0 and bool((depth == -7.0).all()) and bool((seg == -7).all())
    with pytest.raises(_lib.HipLibraryError):
        depth_camera.render_depth(torch.zeros(1, 3, 7, dtype=torch.float64), types[:1], torch.zeros(1, 3, 4, dtype=torch.float64) + 1,
                                  ref.experiment_camera(), 1.0, 1.0, 0.0, 0.0)      # host tensors


def test_points_of_the_reference_golden_and_its_loss():
    from diffsdfsim_amd import depth_camera, pointcloud
    g = np.load(G)
    fx, fy, cx, cy = g["intrinsics"]
    for k in range(3):
        pts, off = depth_camera.observed_points(dev(g["depth"][k:k + 1]), dev(g["seg"][k:k + 1], torch.int32), int(g["body"]), g["cam"][k],
                                                fx, fy, cx, cy)
        want = g["pts"][g["seg_off"][k]:g["seg_off"][k + 1]]
        assert len(pts) == len(want) and list(off) == [0, len(want)]
        assert len(want) == 0 or np.abs(pts.cpu().numpy() - want).max() < 5e-6
        loss, count = pointcloud.match_pointcloud(pts, off, dev(g["pose"][k:k + 1]), g["shape_type"][k:k + 1], dev(g["prm"][k:k + 1]))
        assert int(count[0]) == int(g["count"][k]) and abs(float(loss[0]) - g["loss"][k]) <= 1e-5 * g["loss"][k]


@pytest.mark.parametrize("W,H,kind", [(67, 5, "border"), (80, 5, "border"), (67, 5, "full"), (80, 60, "full"), (67, 5, "empty"),
                                      (130, 7, "border"), (3, 3, "full"), (2, 9, "full")])
def test_points_of_synthetic_masks(W, H, kind):
    from diffsdfsim_amd import depth_camera
    from test_emu_depth_camera import _synthetic
    r = np.random.default_rng(W * 100 + H)
    depth, seg = _synthetic(r, 3, H, W, kind)
    seg[1] = 0      # an empty view in the middle
    cam = ref.experiment_camera()
    args = (2, cam, 64.375, 64.375, (W - 1) / 2, (H - 1) / 2)
    pts, off = depth_camera.observed_points(dev(depth), dev(seg, torch.int32), *args)
    want, woff = ref.observed_points(depth, seg, *args)
    assert np.array_equal(off, woff) and off[1] == off[2]
    assert len(pts) == len(want) and (len(want) == 0 or np.abs(pts.cpu().numpy() - want).max() < 1e-12)
    again, _ = depth_camera.observed_points(dev(depth), dev(seg, torch.int32), *args)
    assert torch.equal(pts, again)


def test_full_size_view_of_the_experiment_scene(full_view):
    pose, kind, prm, cam, depth, seg, want = full_view
    assert (want["seg"] == 2).sum() > 200      # (the wall hides most of the sphere even at t = 0)
    ref.check_view(depth[0].cpu().numpy(), seg[0].cpu().numpy(), want, pose, kind, prm, cam, name="640 x 480", **ref.FULL)


def test_eroded_sphere_points_lie_on_the_sphere_and_fit_its_radius(full_view):
    from diffsdfsim_amd import depth_camera, experiments
    pose, kind, prm, cam, depth, seg, want = full_view
    f = ref.FULL
    pts, off = depth_camera.observed_points(depth, seg, 2, cam, f["fx"], f["fy"], f["cx"], f["cy"])
    mine, _ = ref.observed_points(want["depth"][None], want["seg"][None], 2, cam, f["fx"], f["fy"], f["cx"], f["cy"])
    assert len(pts) > 100 and abs(len(pts) - len(mine)) <= int(want["delicate"].sum()) * 5
    x = pts.cpu().numpy()
    err = np.abs(np.linalg.norm(x - pose[2, 4:], axis=1) - 1.0).max()
    print("%d points, | |x - c| - r | <= %.2e" % (len(x), err))
    assert err < 1e-8
    obs = dict(pts=pts, seg_off=off, time=np.array([-1.0]), scene=np.array([0]))
    true_pose = dev(pose[2:3])
    rad = torch.tensor([1.3], dtype=torch.float64, requires_grad=True)
    for k in range(6):
        loss = experiments.pointcloud_frame_loss(obs, np.array([0]), true_pose, rad, "sphere")
        if k == 0:
            assert abs(float(loss.detach()[0]) - 0.09) < 1e-8, float(loss.detach()[0])
        assert abs(float(rad.detach()[0]) - 1.0 - 0.3 * 0.8 ** k) < 1e-7, (k, float(rad.detach()[0]))
        g, = torch.autograd.grad(loss.sum(), rad)
        rad = (rad - 0.1 * g).detach().requires_grad_()


def test_observations_through_the_depth_camera_see_the_wall_occlude():
    from diffsdfsim_amd import experiments as X
    cam = X.camera_pose()
    assert np.array_equal(cam, ref.experiment_camera())
    world = lambda: X.bounce_world(np.array([1.0]), run_time=0.8, device=DEV)
    kw = dict(every=4, run_time=0.8)
    a = X.pointcloud_observations(world(), cam, observe="depth", **kw)
    v = X.pointcloud_observations(world(), cam, **kw)
    assert np.array_equal(a["time"], v["time"]) and np.array_equal(a["scene"], v["scene"]) and len(a["seg_off"]) == len(v["seg_off"])
    n = np.diff(a["seg_off"])
    print("points per frame:", n)
    assert n[0] > 0 and np.all(n[-2:] < n[0]), "the wall should hide more of the body as it flies towards it"
    b = X.pointcloud_observations(world(), cam, observe="depth", **kw)
    assert torch.equal(a["pts"], b["pts"]) and np.array_equal(a["seg_off"], b["seg_off"])
    with pytest.raises(ValueError):
        X.pointcloud_observations(world(), cam, observe="mesh", **kw)


def test_fit_pointcloud_from_depth_observations():
    from diffsdfsim_amd import experiments as X
    # (every frame: the wall hides the sphere from t = 0.1 on, and only frames with points give the trajectory stage a loss)
    res = X.fit_pointcloud("sphere", [1.0], [1.3], run_time=0.2, max_iter=3, observe="depth", device=DEV)
    frame = [float(h["loss"][0]) for h in res["history"]["frame"]]
    traj = [float(h["loss"][0]) for h in res["history"]["trajectory"]]
    print("first-frame loss", frame, "trajectory loss", traj)
    assert len(frame) == 3 and len(traj) >= 1 and np.all(np.isfinite(frame + traj))
    assert frame[0] > frame[1] > frame[2] > 0 and traj[0] > 0
