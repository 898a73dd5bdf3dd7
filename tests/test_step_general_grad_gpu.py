"""GPU: EVERY output of the reverse sweep (csrc/step_bwd.hip: g_mass, g_inertia, g_fric, g_rest, g_fext, g_prm and the
adjoint of the start state a_pose / a_vel) against the reference's torch.autograd, for a terminal loss that seeds every row
of the incoming adjoint (tests/golden/rollout_general_*.npz, oracle/gen/gen_general_golden.py):

    loss = sum_b  cp_b . p_T,b + cv_b . v_T,b + 0.5 |p_T,b|^2        (moving bodies; p the 7-number pose)

The scenes give every body its own mass, friction coefficient and restitution (the pinned floor too) and a constant wrench
next to gravity, so that the per-body split of the combined coefficients, the f/m terms of a time-of-contact event and the
quaternion / velocity rows of the seed all have a reference value of their own.

north_star tolerance: gradients 1e-5 relative (measured on the largest component of each leaf; components whose reference
magnitude is below 1e-9 are not compared -- no leaf drops out whole: the generator refuses a scene in which a compared leaf
carries less than 1e-3 of the scene's largest leaf gradient).  Sub-step counts exact, final poses / velocities 1e-8.
Measured on the MI355X: worst leaf 1.4e-7."""
import numpy as np
import pytest

import rollout_helpers as R

pytestmark = pytest.mark.gpu

SCENES = [("rollout_general_boxdrop", 12), ("rollout_general_sphere_on_box", 12), ("rollout_general_cylinder", 10),
          ("rollout_general_sphere_notoc", 24)]
SWEEP_OUTPUTS = ("a_pose", "a_vel", "g_mass", "g_inertia", "g_fric", "g_rest", "g_fext", "g_prm")


def run(name, nsteps, part=""):
    from diffsdfsim_amd.engine import BatchEngine
    g = R.load_rollout(name)
    E = BatchEngine(R.spec_from_golden(g, 2), **R.engine_kwargs(g, max_sub=96))
    R.rollout_and_sweep(E, nsteps, R.general_seed(g, part))
    return g, E


def check_forward(E, g):
    assert int(E.get("overflow").max()) == 0
    assert (E.get("nsub") == len(g["traj_t"])).all(), (E.get("nsub"), len(g["traj_t"]))
    k = len(g["traj_t"]) - 1
    perr, verr = np.abs(E.get("pose")[0] - g["traj_p"][k]).max(), np.abs(E.get("vel")[0] - g["traj_v"][k]).max()
    print("final pose error %.1e, final velocity error %.1e" % (perr, verr))
    assert perr < 1e-8 and verr < 1e-8, (perr, verr)


def check_replicas(E):
    for k in SWEEP_OUTPUTS:
        a = E.be.to_numpy(E.adj[k])
        assert np.array_equal(a[0], a[1]), "replicated scenes must give identical " + k


@pytest.mark.parametrize("name,nsteps", SCENES)
def test_every_leaf_matches_reference_autograd(name, nsteps):
    g, E = run(name, nsteps)
    check_forward(E, g)
    if name != "rollout_general_sphere_notoc":
        assert (E.get("tp_flags") & 1).any(), "the scene was meant to go through a time-of-contact event"
    for s in (0, 1):
        R.check_general(E, g, s)
    check_replicas(E)


@pytest.mark.parametrize("part", ["quatonly_", "velonly_"])
def test_quaternion_and_velocity_rows_of_the_seed_alone(part):
    """The tilted box drop with only the quaternion rows of the seed, then only its velocity rows (the rest zero), against the
    reference's gradient of that piece of the loss alone: an error in what the sweep does with an incoming quaternion adjoint
    that cancels against one on the velocity path -- or hides behind the much larger position term -- shows here."""
    g, E = run("rollout_general_boxdrop", 12, part)
    check_forward(E, g)
    R.check_general(E, g, 0, part)
    check_replicas(E)


def test_every_leaf_through_the_world3d_surface():
    """`rollout_general_boxdrop` through the public classes: every leaf a torch tensor, `loss.backward()`, the same golden
    numbers -- every slot `_StepFn.backward` returns (pose, vel, mass, inertia, restitution, fric, fext, shape_prm) is chained
    onto a leaf by torch here, one autograd node per outer step.  The box's and floor's meshes are the package's own (1 ulp
    from the reference's torch.linspace, test_world3d_gpu.py), so the trajectory is held to 1e-7 like the other tests of this
    surface; the gradients to the same 1e-5."""
    import torch
    from diffsdfsim_amd.physics3d import ExternalForce3D, Gravity3D, SDFBox, TotalConstraint3D, World3D
    g = R.load_rollout("rollout_general_boxdrop")
    L = {str(k): torch.tensor(g["leaf_" + str(k)], dtype=torch.float64, requires_grad=True) for k in g["leaves"]}
    kw = lambda b: dict(mass=L["mass_%d" % b], fric_coeff=L["fric_%d" % b], restitution=L["rest_%d" % b], custom_mesh=True, custom_inertia=True)
    floor = SDFBox([0, -0.5, 0], [4.0, 1.0, 4.0], **kw(0))
    box = SDFBox(g["pose0"][1, 4:].tolist(), L["shape_0"], vel=L["vel_1"], **kw(1))
    box.set_p(L["pose_1"])
    box.add_force(Gravity3D(float(g["gravity"])))
    box.add_force(ExternalForce3D(lambda t: L["wrench_1"], multiplier=1.0))
    w = World3D([floor, box], [TotalConstraint3D(floor)], time_of_contact_diff=True)
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
    assert R.check_branches_and_pick_reference(w.engine, g, 0) == "A"      # (no flat-on-flat contact in this scene)
    got = {n: (t.grad.cpu().numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for n, t in L.items()}
    errs = R.leaf_errors(got, g, "A")
    print("World3D leaf errors: " + ", ".join("%s %.1e" % kv for kv in sorted(errs.items())))
    assert max(errs.values()) < 1e-5, errs
