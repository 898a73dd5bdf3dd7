"""GPU: the stepper and its reverse sweep in scenes whose equality rows are NOT "six identity rows on body 0" (the floor under
TotalConstraint3D of every other golden), against the reference's own stepping and torch.autograd
(tests/golden/rollout_general_*.npz with a stored joint Jacobian `Je`, oracle/gen/gen_general_golden.py):

    rotlocked_box   pinned floor + a tilted box under RotConstraint3D (neq = 9), dropped sliding, a time-of-contact event
    planar_sphere   pinned floor + a spinning sphere under ZConstraint (neq = 7)
    two_pinned      pinned floor and pinned wall (neq = 12, n = 30), a sphere thrown into the corner hits both
    three_free      sphere, box, sphere meeting in free space: no floor, no joint, no gravity (neq = 0, n = 18: the register
                    factorisation of csrc/lcp_contact.hip without equality rows, inside dss_step_attempt and the reverse sweep)

The loss, the leaves and the bounds are those of test_step_general_grad_gpu.py: sub-step counts exact, final pose and velocity
1e-8, every compared leaf 1e-5 relative against the reference run whose normal choices the build reproduced, replicated scenes
bit-identical.  Dead leaves are listed by name in the goldens (`dead_leaves`: the mass of every pinned body) and were held
below 1e-12 of the scene's largest leaf when the goldens were made; a rotation-locked body's leaves stay alive as a whole (its
shape and mass act through the contact geometry and the linear rows; only their inertia-coupled parts vanish).
Measured on the MI355X: DESIGN.md section 2."""
import numpy as np
import pytest

import rollout_helpers as R
from test_step_general_grad_gpu import check_forward, check_replicas, run

pytestmark = pytest.mark.gpu

SCENES = [("rollout_general_rotlocked_box", 12, 9), ("rollout_general_planar_sphere", 16, 7), ("rollout_general_two_pinned", 16, 12),
          ("rollout_general_three_free", 14, 0)]


@pytest.mark.parametrize("name,nsteps,neq", SCENES)
def test_every_leaf_matches_reference_autograd(name, nsteps, neq):
    g, E = run(name, nsteps)
    assert E.neq == neq and E.nb == len(g["mass"])
    check_forward(E, g)
    if name == "rollout_general_rotlocked_box":
        assert (E.get("tp_flags") & 1).any(), "the scene was meant to go through a time-of-contact event"
    for s in (0, 1):
        R.check_general(E, g, s)
    check_replicas(E)


def test_rotation_locked_box_through_the_world3d_surface():
    """`rollout_general_rotlocked_box` through the public classes: the equality rows are built by physics3d/world.py from
    TotalConstraint3D(floor) and RotConstraint3D(box), every leaf is a torch tensor, `loss.backward()`.  Trajectory 1e-7 (the
    package's own meshes are 1 ulp from the reference's, as in test_step_general_grad_gpu.py), gradients 1e-5."""
    import torch
    from diffsdfsim_amd.physics3d import ExternalForce3D, Gravity3D, RotConstraint3D, SDFBox, TotalConstraint3D, World3D
    g = R.load_rollout("rollout_general_rotlocked_box")
    L = {str(k): torch.tensor(g["leaf_" + str(k)], dtype=torch.float64, requires_grad=True) for k in g["leaves"]}
    kw = lambda b: dict(mass=L["mass_%d" % b], fric_coeff=L["fric_%d" % b], restitution=L["rest_%d" % b], custom_mesh=True, custom_inertia=True)
    floor = SDFBox([0, -0.5, 0], [4.0, 1.0, 4.0], **kw(0))
    box = SDFBox(g["pose0"][1, 4:].tolist(), L["shape_0"], vel=L["vel_1"], **kw(1))
    box.set_p(L["pose_1"])
    box.add_force(Gravity3D(float(g["gravity"])))
    box.add_force(ExternalForce3D(lambda t: L["wrench_1"], multiplier=1.0))
    w = World3D([floor, box], [TotalConstraint3D(floor), RotConstraint3D(box)], time_of_contact_diff=True)
    assert np.array_equal(w.engine.get("Je")[0], g["Je"])
    for _ in range(12):
        w.step(fixed_dt=True)
    assert len(w.trajectory) == len(g["traj_t"])
    k = len(g["traj_t"]) - 1
    assert np.abs(box.p.detach().cpu().numpy() - g["traj_p"][k][1]).max() < 1e-7
    assert np.abs(box.v.detach().cpu().numpy() - g["traj_v"][k][1]).max() < 1e-7
    cp, cv = (torch.as_tensor(g[n][1], device=box.p.device) for n in ("loss_cp", "loss_cv"))
    loss = (cp * box.p).sum() + (cv * box.v).sum() + 0.5 * (box.p ** 2).sum()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    loss.backward()
    assert R.check_branches_and_pick_reference(w.engine, g, 0) == "A"      # (corner contacts only: no flat-on-flat coin flip)
    got = {n: (t.grad.cpu().numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for n, t in L.items()}
    errs = R.leaf_errors(got, g, "A")
    print("World3D leaf errors: " + ", ".join("%s %.1e" % kv for kv in sorted(errs.items())))
    assert max(errs.values()) < 1e-5, errs
