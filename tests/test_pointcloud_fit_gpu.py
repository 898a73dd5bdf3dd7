"""GPU: the point-cloud fitting driver (diffsdfsim_amd.experiments.fit_pointcloud and its parts) on quantities that can be derived.

(a) first-frame fit of a sphere with the pose at truth and the icosphere's vertices times r* as the points: every point has
    sdf = r* - rad, so the loss is exactly dr^2 and gradient descent with lr = 0.1 gives dr_k = 0.3 * 0.8^k.
(b) trajectory stage without contact (run_time 0.1, gravity on, start pose at truth): estimate and target fall alike, so
    d loss / d rad = 2 dr; d loss / d start position against central differences of the driver's own loss (h = 1e-5, tolerance
    1e-6 max(1, |g|), the finite-difference tolerance of tests/test_emu_sdf_mesh.py).
(c) through a bounce (B = 2, run_time 0.8): the gradients of the driver's loss w.r.t. rad and the start pose against the same
    loss assembled from the torch restatement (tests/pointcloud_ref.py) on the same trajectory tensors -- both go back through
    the same stepper, which isolates the kernel inside the composite; relative 1e-9 of the largest component.
(d), (e) the rounded cube's world and fit_pointcloud(shape='cube'): see the two tests' own texts."""
import numpy as np
import pytest
import torch

import pointcloud_ref as ref

pytestmark = pytest.mark.gpu
TRUTH = [1.0, 0.0, 0.0, 0.0, 0.0, 5.0, 0.0]


def test_first_frame_fit_of_a_sphere_contracts_by_the_derived_factor():
    from diffsdfsim_amd import experiments as X, meshes
    r_true, dev = 0.8, torch.device("cuda:0")
    uv, _ = meshes.icosphere(4)
    pts = torch.tensor(uv * r_true + np.array(TRUTH[4:]), device=dev)
    obs = dict(pts=pts, seg_off=np.array([0, len(uv)]), time=np.array([-1.0]), scene=np.array([0]))
    pose = torch.tensor([TRUTH], dtype=torch.float64)
    rad = torch.tensor([r_true + 0.3], dtype=torch.float64, requires_grad=True)
    for k in range(1, 6):
        rad.grad = None
        loss = X.pointcloud_frame_loss(obs, np.array([0]), pose, rad, "sphere")
        loss.sum().backward()
        with torch.no_grad():
            rad -= 0.1 * rad.grad
        print("k", k, "dr", float(rad) - r_true, "want", 0.3 * 0.8 ** k)
        assert abs((float(rad) - r_true) - 0.3 * 0.8 ** k) < 1e-9


def _free_fall_loss(obs, rad, pos, run_time=0.1):
    from diffsdfsim_amd import experiments as X
    pose0 = torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64), pos], 1)
    world = X.bounce_world(rad, run_time=run_time, init_pose=pose0)
    traj = X.run_world_fixed_dt(world, run_time, detach_2nd_bounce=True)
    return X.pointcloud_trajectory_loss(traj, obs, rad, "sphere")


def test_trajectory_stage_without_contact_has_the_derived_gradients():
    from diffsdfsim_amd import experiments as X
    r_true, dr = 0.8, 0.25
    truth = torch.tensor([TRUTH], dtype=torch.float64)
    with torch.no_grad():
        obs = X.pointcloud_observations(X.bounce_world(torch.tensor([r_true], dtype=torch.float64), run_time=0.1, init_pose=truth),
                                        X.camera_pose(), run_time=0.1)
    assert len(obs["time"]) > 3 and obs["seg_off"][-1] > 1000
    rad = torch.tensor([r_true + dr], dtype=torch.float64, requires_grad=True)
    pos = truth[:, 4:].clone().requires_grad_()
    loss = _free_fall_loss(obs, rad, pos)
    loss.sum().backward()
    print("loss", float(loss), "want", dr * dr, "d/drad", float(rad.grad), "want", 2 * dr, "d/dpos", pos.grad)
    assert abs(float(loss) - dr * dr) < 1e-9 and abs(float(rad.grad) - 2 * dr) < 1e-9
    h = 1e-5
    for i in range(3):
        with torch.no_grad():
            e = torch.zeros(1, 3, dtype=torch.float64); e[0, i] = h
            fd = (float(_free_fall_loss(obs, rad.detach(), pos.detach() + e)) - float(_free_fall_loss(obs, rad.detach(), pos.detach() - e))) / (2 * h)
        g = float(pos.grad[0, i])
        print("axis", i, "autograd", g, "central difference", fd)
        assert abs(g - fd) < 1e-6 * max(1.0, abs(g))


def _cube_free_fall_loss(obs, rad, pos, run_time=0.1):
    from diffsdfsim_amd import experiments as X
    pose0 = torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64), pos], 1)
    world = X.bounce_world(rad, run_time=run_time, init_pose=pose0, shape="cube")
    traj = X.run_world_fixed_dt(world, run_time, detach_2nd_bounce=True)
    return X.pointcloud_trajectory_loss(traj, obs, rad, "cube")


def test_cube_trajectory_stage_without_contact_against_central_differences():
    """(d) the rounded cube's world (level-set mesh, mesh inertia, differentiable start pose) through the same contact-free
    stage as (b): d loss / d rad and d loss / d start position against central differences of the driver's own loss, h = 1e-5,
    tolerance 1e-6 max(1, |g|).  The observed points are the target's mesh vertices, which lie on the level set only to the
    mesher's accuracy, so no closed form is asserted for the value."""
    from diffsdfsim_amd import experiments as X
    truth = torch.tensor([TRUTH], dtype=torch.float64)
    with torch.no_grad():
        tw = X.bounce_world(torch.tensor([0.7], dtype=torch.float64), run_time=0.1, init_pose=truth, shape="cube")
        assert int(tw.engine.get("shape_type")[0, -1]) == 3 and abs(float(tw.engine.get("shape_prm")[0, -1, 0]) - 1.4) < 1e-15
        obs = X.pointcloud_observations(tw, X.camera_pose(), run_time=0.1)
    assert len(obs["time"]) > 3 and obs["seg_off"][-1] > 1000
    rad = torch.tensor([0.85], dtype=torch.float64, requires_grad=True)
    pos = (truth[:, 4:] + torch.tensor([[0.03, -0.02, 0.04]], dtype=torch.float64)).requires_grad_()
    loss = _cube_free_fall_loss(obs, rad, pos)
    loss.sum().backward()
    assert float(loss) > 1e-3
    h = 1e-5
    with torch.no_grad():
        e = torch.tensor([h], dtype=torch.float64)
        fd = (float(_cube_free_fall_loss(obs, rad.detach() + e, pos.detach())) - float(_cube_free_fall_loss(obs, rad.detach() - e, pos.detach()))) / (2 * h)
    print("cube d/drad autograd", float(rad.grad), "central difference", fd)
    assert abs(float(rad.grad) - fd) < 1e-6 * max(1.0, abs(fd))
    with torch.no_grad():
        e = torch.zeros(1, 3, dtype=torch.float64); e[0, 1] = h
        fd = (float(_cube_free_fall_loss(obs, rad.detach(), pos.detach() + e)) - float(_cube_free_fall_loss(obs, rad.detach(), pos.detach() - e))) / (2 * h)
    print("cube d/dpos_y autograd", float(pos.grad[0, 1]), "central difference", fd)
    assert abs(float(pos.grad[0, 1]) - fd) < 1e-6 * max(1.0, abs(fd))


def test_fit_pointcloud_cube_runs_both_stages_and_moves_towards_the_target():
    """(e) fit_pointcloud(shape='cube') end to end on one scene without contact: both stages run, the first-frame loss falls from
    one iteration to the next, and the half size moves from its start towards the target."""
    from diffsdfsim_amd import experiments as X
    res = X.fit_pointcloud("cube", target_rad=[0.7], start_rad=[0.9], run_time=0.1, max_iter=3, optimize_pose=False)
    f, t = res["history"]["frame"], res["history"]["trajectory"]
    print("frame", [float(h["loss"][0]) for h in f], "trajectory", [float(h["loss"][0]) for h in t], "rad", res["rad"])
    assert len(f) == 3 and len(t) == 3
    assert f[1]["loss"][0] < f[0]["loss"][0] and f[2]["loss"][0] < f[1]["loss"][0]
    assert 0.7 < res["rad"][0] < 0.9 and all(np.isfinite(h["loss"]).all() and np.isfinite(h["grad_rad"]).all() for h in f + t)


def _restated_match(kind_name):
    def match(pts, seg_off, pose, shape_type, prm):
        s, n = [], []
        for i in range(pose.shape[0]):
            kind = int(shape_type[i])
            l, c = ref.segment_loss(kind, prm[i, :3], prm[i, 3], pose[i], pts[int(seg_off[i]):int(seg_off[i + 1])])
            s.append(l); n.append(c)
        return torch.stack(s), torch.stack(n).to(torch.float64)
    return match


def test_gradients_through_a_bounce_equal_the_restated_loss_on_the_same_trajectory(shape="sphere"):
    from diffsdfsim_amd import experiments as X
    run_time = 0.8
    tgt = torch.tensor([0.9, 0.7], dtype=torch.float64)
    tp = torch.tensor([TRUTH, TRUTH], dtype=torch.float64)
    with torch.no_grad():
        obs = X.pointcloud_observations(X.bounce_world(tgt, run_time=run_time, init_pose=tp, shape=shape), X.camera_pose(), run_time=run_time, every=4)
    rad = torch.tensor([1.0, 0.85], dtype=torch.float64, requires_grad=True)
    q = torch.tensor([[0.99, 0.05, -0.08, 0.03], [0.98, -0.1, 0.02, 0.06]], dtype=torch.float64)
    rot = (q / q.norm(dim=1, keepdim=True)).requires_grad_()
    pos = (tp[:, 4:] + torch.tensor([[0.05, -0.04, 0.03], [-0.02, 0.06, 0.04]], dtype=torch.float64)).requires_grad_()
    world = X.bounce_world(rad, run_time=run_time, init_pose=torch.cat([rot, pos], 1), shape=shape)
    traj = X.run_world_fixed_dt(world, run_time, detach_2nd_bounce=True)
    # the wall's face is at x = 4.5: the sphere's centre gets as far as 4.5 - rad and comes back
    x = traj["pose"][:, :, -1, 4].detach().cpu()
    assert bool((x.max(0).values > 4.5 - rad.detach() - 0.01).all()) and bool((x[-1] < x.max(0).values - 0.05).all()), "no bounce off the wall"
    l_k = X.pointcloud_trajectory_loss(traj, obs, rad, shape)
    g_k = torch.autograd.grad(l_k.sum(), [rad, rot, pos], retain_graph=True)
    l_r = X.pointcloud_trajectory_loss(traj, obs, rad, shape, match=_restated_match(shape))
    g_r = torch.autograd.grad(l_r.sum(), [rad, rot, pos])
    print("loss", l_k.tolist(), l_r.tolist())
    assert torch.allclose(l_k.cpu(), l_r.cpu(), rtol=1e-12, atol=0)
    for name, a, b in zip(("rad", "rot", "pos"), g_k, g_r):
        print(name, a.tolist(), "deviation %.2e of the largest component" % float((a - b).abs().max() / b.abs().max()))
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()), name
