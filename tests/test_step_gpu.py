"""GPU: the batched stepper (csrc/step.hip, narrowphase.hip, lcp_contact.hip) through the C ABI against
rollouts recorded from the reference's CPU path (tests/golden/rollout_*.npz).

north_star tolerance: contact-pair indices exact, positions/velocities 1e-5 relative.  Held to 1e-8 here.
Each golden scene is replicated along the batch axis; replicas must agree bit for bit (no cross-scene
coupling, deterministic reductions)."""
import numpy as np
import pytest

import rollout_helpers as R

pytestmark = pytest.mark.gpu


def make(name, copies, **kw):
    from diffsdfsim_amd.engine import BatchEngine
    g = R.load_rollout(name)
    return g, BatchEngine(R.spec_from_golden(g, copies), **R.engine_kwargs(g, **kw))


@pytest.mark.parametrize("name", ["rollout_sphere", "rollout_stack1", "rollout_stack2"])
def test_initial_contacts_match_reference(name):
    g, E = make(name, 3)
    for s in range(3):
        R.check_contacts(E, s, g["init_body"], g["init_geom"], len(g["init_body"]))


@pytest.mark.parametrize("name,nsteps,copies", [("rollout_sphere", 24, 5), ("rollout_stack1", 4, 4), ("rollout_stack2", 3, 130), ("rollout_boxdrop", 12, 3), ("rollout_cylinder", 10, 3), ("rollout_sphere_long", 100, 2)])
def test_rollout_matches_reference(name, nsteps, copies):
    g, E = make(name, copies, max_sub=320)
    for _ in range(nsteps):
        E.step()
    nsub = E.get("nsub")
    assert (nsub == len(g["traj_t"])).all(), nsub
    k = len(g["traj_t"]) - 1
    pose, vel = E.get("pose"), E.get("vel")
    assert np.abs(pose[0] - g["traj_p"][k]).max() < 1e-8
    assert np.abs(vel[0] - g["traj_v"][k]).max() < 1e-8
    assert (pose == pose[:1]).all() and (vel == vel[:1]).all(), "replicated scenes diverged"
    assert int(E.get("overflow").max()) == 0
    for s in (0, copies - 1):
        R.check_contacts(E, s, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]))
    # the tape holds every accepted sub-step: start poses equal the reference's previous end poses
    tp = E.get("tp_pose")
    for j in range(1, k + 1):
        assert np.abs(tp[j, 0] - g["traj_p"][j - 1]).max() < 1e-8


@pytest.mark.parametrize("name,nsteps,copies", [("rollout_sphere_notoc", 24, 3), ("rollout_sphere", 24, 3), ("rollout_stack1", 4, 2), ("rollout_stack2", 3, 65), ("rollout_boxdrop", 12, 2), ("rollout_cylinder", 10, 2), ("rollout_sphere_long", 100, 2)])
def test_gradients_match_reference_autograd(name, nsteps, copies):
    """Reverse sweep (csrc/step_bwd.hip) vs torch.autograd of the reference: d sum|pos_T|^2 / d(dims | radius).
    Flat-on-flat contacts make the reference gradient bimodal (both branches are in the golden)."""
    g, E = make(name, copies, max_sub=320)
    R.rollout_and_sweep(E, nsteps)
    picked = []
    for s in (0, copies - 1):
        picked.append(R.check_gradients(E, g, tol=1e-3 if name == "rollout_stack2" else 1e-4, s=s)[0])
    print(name, "branch run matched:", picked)
    gp = E.be.to_numpy(E.adj["g_prm"])
    assert (gp == gp[:1]).all(), "replicated scenes must give identical gradients"


@pytest.mark.parametrize("name,nsteps", [("rollout_sphere", 24), ("rollout_boxdrop", 12)])
def test_full_kernel_variants_agree_with_the_lean_ones(name, nsteps):
    """The device twin of tests/test_emu_step.py's test of the same name: the same goldens through the full variants of the
    narrow phase and the contact adjoint (selected with spec['full_kernels'], reached through launch_bwd_pre_all):
    bit-identical state, gradients equal to rounding."""
    from diffsdfsim_amd.engine import BatchEngine
    g = R.load_rollout(name)
    out = []
    for full in (False, True):
        spec = R.spec_from_golden(g)
        spec["full_kernels"] = full
        E = BatchEngine(spec, max_sub=64, **R.engine_kwargs(g))
        assert int(E.W.shape_rare) == int(full)
        R.rollout_and_sweep(E, nsteps)
        out.append((E.get("pose").copy(), E.get("vel").copy(), E.get("nsub").copy(), E.be.to_numpy(E.adj["g_prm"]).copy()))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)
    # the lean reverse sweep differentiates the contact geometry in reverse mode, the full one in forward mode: the same
    # derivative to rounding
    ga, gb = out[0][3], out[1][3]
    assert np.abs(gb).max() > 0.0
    assert np.abs(ga - gb).max() < 3e-8 * np.abs(gb).max()      # (rounding differences of 1e-16 grow through 57 sub-steps)


def test_pair_that_outgrows_the_wavefront_scratch_matches_reference():
    """A wide flat box on the floor has ~800 contacts before thinning: the wavefront that starts the pair hands it
    to the deferred list, a whole workgroup redoes it.  Same contacts, same trajectory as the reference."""
    # (400 replicas: with fewer work items than the grid has workgroups such an item is given a whole workgroup from the start)
    g, E = make("rollout_bigbox", 400, max_sub=16, max_cand=2048, maxc=64)
    for _ in range(3):
        E.step()
    assert int(E.get("n_pairs")[4]) >= 1, "the pair was expected to be deferred"
    assert int(E.get("overflow").max()) == 0
    k = len(g["traj_t"]) - 1
    assert (E.get("nsub") == len(g["traj_t"])).all()
    assert np.abs(E.get("pose")[0] - g["traj_p"][k]).max() < 1e-8 and np.abs(E.get("vel")[0] - g["traj_v"][k]).max() < 1e-8
    for s in (0, 399):
        R.check_contacts(E, s, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]))
    # ... and the same pair started on a workgroup (a batch of two)
    g2, E2 = make("rollout_bigbox", 2, max_sub=16, max_cand=2048, maxc=64)
    for _ in range(3):
        E2.step()
    assert int(E2.get("n_pairs")[4]) == 0 and np.array_equal(E2.get("pose")[0], E.get("pose")[0])


def test_config3_scene_seven_box_stack_matches_reference():
    """BASELINE configs[2] itself at batch 1 (floor + 7 stacked boxes, 123-128 contacts, shoved so that friction
    saturates), three steps: trajectory, contact sets and the tape against the reference; replicas bit-identical.
    With 125 contacts on seven stacked flat faces the interior point method stops at its iteration limit (max_iter = 10,
    engines.py:25) short of full convergence, and the order of the contacts inside a pair differs from Qhull's, so the
    last digits of the velocities depend on the path: held to 1e-6 here (north star: 1e-5), poses to 1e-7."""
    g, E = make("rollout_stack7", 3, max_sub=16, maxc=128)
    for _ in range(3):
        E.step()
    assert int(E.get("overflow").max()) == 0 and (E.get("nsub") == len(g["traj_t"])).all()
    k = len(g["traj_t"]) - 1
    pose, vel = E.get("pose"), E.get("vel")
    assert np.abs(pose[0] - g["traj_p"][k]).max() < 1e-7 and np.abs(vel[0] - g["traj_v"][k]).max() < 1e-6
    assert (pose == pose[:1]).all() and (vel == vel[:1]).all()
    for s in (0, 2):
        # (one pair may hold one contact more or less than the reference's: the corner tie, rollout_helpers.check_contacts)
        assert R.check_contacts(E, s, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]), tol=1e-5, corner_ties=True) <= 1
    tp, tnc = E.get("tp_pose"), E.get("tp_nc")
    for j in range(1, k + 1):
        assert np.abs(tp[j, 0] - g["traj_p"][j - 1]).max() < 1e-7
        assert int(tnc[j, 0]) == int(g["traj_nc"][j - 1])


def test_config3_scene_gradients_against_reference_autograd():
    """d sum|pos_T|^2 / d dims of the seven boxes.  Every flat-on-flat contact of the stack takes its normal from one
    body or the other by comparing two rounding-noise Laplacians (contacts.py:198), in the reference as here, so the
    reference's own two recorded evaluations differ from each other; the kernel's gradient must be as close to them as
    they are to each other."""
    g, E = make("rollout_stack7", 2, max_sub=16, maxc=128)
    R.rollout_and_sweep(E, 3)
    got = R.param_grads(E, g, 0)
    a = np.concatenate([g["grad_%d" % i] for i in range(7)]); b = np.concatenate([g["gradB_%d" % i] for i in range(7)])
    mine = np.concatenate(got)
    spread = np.abs(a - b).max()
    err = min(np.abs(mine - a).max(), np.abs(mine - b).max())
    assert np.isfinite(mine).all() and err < max(3.0 * spread, 1e-4 * np.abs(a).max()), (err, spread)
    gp = E.be.to_numpy(E.adj["g_prm"])
    assert (gp == gp[:1]).all()
    # the normal choice of every contact against the reference's recorded one: required to agree wherever the two Laplacians
    # differ by more than noise; if the build's choices coincide with one recorded run at every contact, 1e-5 against it
    which = R.check_branches_and_pick_reference(E, g, 0)
    if which is not None:
        ref = a if which == "A" else b
        assert np.abs(mine - ref).max() < 1e-5 * np.abs(ref).max(), (which, np.abs(mine - ref).max())


@pytest.mark.parametrize("name,nsteps", [("rollout_two_spheres", 12), ("rollout_sphere_on_box", 12), ("rollout_floor_last", 20),
                                         ("rollout_no_contact", 6), ("rollout_sphere_roll", 40), ("rollout_boxdrop_fd4", 12)])
def test_cases_found_by_random_comparison(name, nsteps):
    """Scenes kept from random comparisons against the reference (tools/dbg_fuzz.py): sphere against sphere, three
    bodies, a pinned body that is not body 0, a no_contact pair, a rolling sphere with coincident contact points, four friction directions.  Held:
    the number of sub-steps, the contact COUNT of every sub-step (the thinning stage must pick Qhull's vertices), poses
    to 1e-9 and d sum|pos_T|^2 / d parameters to 1e-5 (gradients below 1e-9 in magnitude are not compared)."""
    g, E = make(name, 2, max_sub=96)
    R.rollout_and_sweep(E, nsteps)
    assert int(E.get("overflow").max()) == 0 and (E.get("nsub") == len(g["traj_t"])).all()
    k = len(g["traj_t"]) - 1
    assert np.abs(E.get("pose")[0] - g["traj_p"][k]).max() < 1e-9 and np.abs(E.get("vel")[0] - g["traj_v"][k]).max() < 1e-8
    tp, tnc = E.get("tp_pose"), E.get("tp_nc")
    for j in range(1, k + 1):
        assert np.abs(tp[j, 0] - g["traj_p"][j - 1]).max() < 1e-9
        assert int(tnc[j, 0]) == int(g["traj_nc"][j - 1]), (j, int(tnc[j, 0]), int(g["traj_nc"][j - 1]))
    R.check_contacts(E, 1, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]))
    got = R.param_grads(E, g, 0)
    for i, gi in enumerate(got):
        want = g["grad_%d" % i]
        if np.abs(want).max() > 1e-9:
            assert np.abs(gi - want).max() < 1e-5 * np.abs(want).max(), (i, gi, want)


def test_scenes_of_a_batch_do_not_influence_each_other():
    """64 different sphere drops (different radii, heights, speeds: impacts, dt halving and time-of-contact events
    fall in different attempts) stepped as one batch and one by one: poses, velocities, sub-step counts and gradients must
    be bit-identical -- the lock-step retry loop, the work lists of the persistent narrow phase and the per-scene scratch
    of the reverse sweep (DssAdjoint.cscr: rows of a scene must not reach into its neighbours') couple nothing."""
    from diffsdfsim_amd import scenes
    from diffsdfsim_amd.engine import BatchEngine
    nS = 64
    spec = scenes.sphere_drop(nS, seed=5, floor_dims=(4.0, 1.0, 4.0))
    T = 30

    def run(sp):
        E = BatchEngine(sp, max_sub=4 * T + 16, maxc=64)
        R.rollout_and_sweep(E, T)
        flags = E.get("tp_flags")
        return (E.get("pose").copy(), E.get("vel").copy(), E.get("nsub").copy(), E.be.to_numpy(E.adj["g_prm"]).copy(),
                E.be.to_numpy(E.adj["g_mass"]).copy(), (flags & 1).sum(axis=0))

    P, V, N, G, GM, toc = run(spec)
    assert len(set(N.tolist())) > 3, "the scenes were meant to take different numbers of sub-steps"
    assert (toc > 0).sum() >= nS // 2, "most scenes were meant to go through a time-of-contact event"
    for s in range(nS):
        one = {k: (v[s:s + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (nS,) else v) for k, v in spec.items()}
        p, v, n, g, gm, _ = run(one)
        assert n[0] == N[s] and np.array_equal(p[0], P[s]) and np.array_equal(v[0], V[s]), s
        assert np.array_equal(g[0], G[s]) and np.array_equal(gm[0], GM[s]), (s, g[0], G[s])


def test_tape_overflow_is_a_capacity_error():
    """More accepted sub-steps than tape slots (max_sub): the engine raises instead of dropping records that a reverse
    sweep would then read past the tape."""
    from diffsdfsim_amd import scenes
    from diffsdfsim_amd.engine import BatchEngine
    E = BatchEngine(scenes.sphere_drop(3, seed=5, floor_dims=(4.0, 1.0, 4.0)), max_sub=4, maxc=64)
    with pytest.raises(RuntimeError, match="max_sub"):
        for _ in range(8):
            E.step()


def test_escape_from_endless_halving_keeps_the_penetrating_contacts_like_the_reference():
    """strict_no_penetration=False and a sphere too fast for any halving of dt to land in the contact band: once
    dt < dt / 2^10 the reference goes on with the contacts as they are (world.py:345-347) -- every contact of the penetrating
    direction, unthinned (here 6 where the thinned set would be smaller), none from the reverse direction, no time-of-contact
    bookkeeping, and no gradient through their geometry (they were computed under no_grad)."""
    g, E = make("rollout_fast_sphere", 2, max_sub=32)
    assert not bool(g["strict_no_pen"])
    R.rollout_and_sweep(E, 3)
    assert (E.get("nsub") == len(g["traj_t"])).all(), E.get("nsub")
    k = len(g["traj_t"]) - 1
    assert np.abs(E.get("pose")[0] - g["traj_p"][k]).max() < 1e-8 and np.abs(E.get("vel")[0] - g["traj_v"][k]).max() < 1e-7
    tnc, tg, tb, tf = E.get("tp_nc"), E.get("tp_geom"), E.get("tp_body"), E.get("tp_face")
    for j in range(1, k + 1):
        n = int(g["traj_nc"][j - 1])
        assert int(tnc[j, 0]) == n, (j, int(tnc[j, 0]), n)
        if n:
            assert (tg[j, 0][9, :n] > float(g["tol"])).any(), "the kept contacts penetrate"
            assert [tuple(r) for r in tb[j, 0][:, :n].T] == [tuple(r) for r in g["traj_body"][j - 1][:n]]
            assert (tf[j, 0][:n] < 0).all(), "contacts of a penetrating direction carry no geometry adjoint"
            a = np.sort(tg[j, 0][3:6, :n].T, axis=0); b = np.sort(g["traj_geom"][j - 1][:n, 3:6], axis=0)
            assert np.abs(a - b).max() < 1e-7
    R.check_gradients(E, g, tol=1e-5)


def test_config3_scene_at_full_batch_replicas_are_bit_identical_and_match_the_reference():
    """BASELINE configs[2]'s own scene (floor + 7 stacked boxes, 123-128 contacts) replicated B = 1024 times: every replica
    bit-identical to the first (poses, velocities, contact counts, gradients), the first within the single-scene
    tolerances of the reference golden.  The whole batch machinery (work lists of the persistent narrow phase over 14 k
    items, one LCP wavefront per scene, the reverse sweep's per-scene scratch) at the size the metric is quoted on."""
    g, E = make("rollout_stack7", 1024, max_sub=16, maxc=128)
    R.rollout_and_sweep(E, 3)
    assert int(E.get("overflow").max()) == 0 and (E.get("nsub") == len(g["traj_t"])).all()
    k = len(g["traj_t"]) - 1
    pose, vel, nc = E.get("pose"), E.get("vel"), E.get("nc")
    assert np.abs(pose[0] - g["traj_p"][k]).max() < 1e-7 and np.abs(vel[0] - g["traj_v"][k]).max() < 1e-6
    assert (pose == pose[:1]).all() and (vel == vel[:1]).all() and (nc == nc[0]).all()
    gp, gm = E.be.to_numpy(E.adj["g_prm"]), E.be.to_numpy(E.adj["g_mass"])
    assert np.isfinite(gp).all() and (gp == gp[:1]).all() and (gm == gm[:1]).all()
    for s in (0, 511, 1023):
        # (one pair may hold one contact more or less than the reference's: the corner tie, rollout_helpers.check_contacts)
        assert R.check_contacts(E, s, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]), tol=1e-5, corner_ties=True) <= 1


@pytest.mark.parametrize("name", ["rollout_boxdrop_stop_contact", "rollout_boxdrop_stop_friction", "rollout_boxdrop_detach_b2"])
def test_gradient_switches_of_world3d_match_reference(name):
    """World3D(stop_contact_grad / stop_friction_grad / detach_contact_b2) (sdf_physics/physics3d/world.py:33-37, 59-62, 77-80;
    contacts.py:175-178): the tilted box drop -- same trajectory as without the switch, and d sum|pos_T|^2 / d dims equal to
    the reference's autograd value with that switch (which differs from the plain one in every component) to 1e-5."""
    g, E = make(name, 2, max_sub=96)
    assert int(E.W.grad_flags) == int(g["grad_flags"]) != 0
    R.rollout_and_sweep(E, 12)
    k = len(g["traj_t"]) - 1
    assert (E.get("nsub") == len(g["traj_t"])).all()
    assert np.abs(E.get("pose")[0] - g["traj_p"][k]).max() < 1e-8
    plain = R.load_rollout("rollout_boxdrop")
    assert np.abs(plain["traj_p"][k] - g["traj_p"][k]).max() == 0.0          # the switches act on the reverse sweep only
    assert np.abs(plain["grad_0"] - g["grad_0"]).max() > 1e-2
    R.check_gradients(E, g, tol=1e-5)


def test_world3d_accepts_the_gradient_switches():
    from diffsdfsim_amd.physics3d import Gravity3D, SDFBox, TotalConstraint3D, World3D
    import torch
    floor = SDFBox([0, -0.5, 0], [4.0, 1.0, 4.0], custom_mesh=True, custom_inertia=True)
    dims = torch.tensor([0.5, 0.4, 0.3], dtype=torch.float64, requires_grad=True)
    b = SDFBox([0.0, 0.3, 0.0], dims, vel=[0.3, 0.1, 0, 0.2, 0, 0], custom_mesh=True, custom_inertia=True)
    b.add_force(Gravity3D())
    w = World3D([floor, b], [TotalConstraint3D(floor)], stop_contact_grad=True, stop_friction_grad=True, detach_contact_b2=True)
    assert int(w.engine.W.grad_flags) == 7
    for _ in range(6):
        w.step(fixed_dt=True)
    (b.p[4:] ** 2).sum().backward()
    assert torch.isfinite(dims.grad).all()
    with pytest.raises(NotImplementedError):
        World3D([floor, b], [TotalConstraint3D(floor)], post_stab=True)
