"""GPU: contact stepping, forward and backward, for a neural SDF body on the shapenet network (latent 4, 8 x 256): the latent
code comes from the latent table DssWorld.igr_latent, its adjoint lands in DssAdjoint.g_latent.

Reference: rollouts recorded from the reference's own ``SDF3D.query_sdfs`` / ``FWContactHandler`` / ``World3D``
(tools/gen_igr_shapenet_golden.py) on seeded geometric-init weights (tests/implicit_net.py; trained shapenet weights are not
available offline, so the network itself stays parity-unpinned -- the STEPPER around it is pinned here).  Tolerances are those
of tests/test_igr_stepper_gpu.py for the 128-wide network: contact pairs exact, poses 1e-7 / 1e-6, gradients 1e-5 relative."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import igr_helpers as H
import implicit_net as IN
import rollout_helpers as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def golden(name):
    return R.load_rollout(name)


@functools.lru_cache(None)
def packed(name):
    """The network a golden was recorded with, packed for the device (256-wide goldens name their shape; the 128-wide ones
    are the seeded network of oracle/igr_oracle.py)."""
    from diffsdfsim_amd.igr import pack_weights
    g = golden(name)
    if "igr_width" not in g:
        return pack_weights(*H.seeded_weights(g))
    assert (int(g["igr_width"]), int(g["igr_latent_size"])) == (256, 4)
    return pack_weights(*IN.geometric_init(seed=int(g["igr_seed"]), radius_init=float(g["igr_radius"]), **IN.SHAPENET))


def spec256(name, copies, g=None):
    g = golden(name) if g is None else g
    spec = H.spec_from_golden(g, copies, packed=packed(name))
    spec["igr_latent"] = np.repeat(g["igr_latent"][None], copies, axis=0)
    # Query-list capacity (a size, like max_cand): the first attempt of the second step moves the body 4 mm INTO the floor before
    # it is rejected and its dt halved (as in the reference), and ~1400 of this finer mesh's faces (scale 1) become tentative
    # contacts of that attempt, each with 6 Laplacian probes: 8478 values per scene in one round, above the default of 8192.
    spec["igr_qcap"] = 16384 * copies
    assert not spec["shape_prm"][:, int(g["igr_body"])].any()
    return spec


def run_like_run_world(step, t, run_time):
    n = 0
    while t() < run_time:
        step()
        n += 1
        assert n < 500
    return n


def test_rollout_matches_reference():
    from diffsdfsim_amd.engine import BatchEngine
    g = golden("rollout_igr256_small")
    E = BatchEngine(spec256("rollout_igr256_small", 2), **H.engine_kwargs(g, max_sub=128))
    assert int(E.get("overflow").max()) == 0
    R.check_contacts(E, 0, g["init_body"], g["init_geom"], len(g["init_body"]))
    run_like_run_world(E.step_once, lambda: float(E.get("t")[0]), float(g["run_time"]))
    assert int(E.get("overflow").max()) == 0
    nsub = E.get("nsub")
    assert (nsub == len(g["traj_t"])).all(), (nsub, len(g["traj_t"]))
    k = len(g["traj_t"]) - 1
    pose, vel = E.get("pose"), E.get("vel")
    tp, tnc, tb = E.get("tp_pose"), E.get("tp_nc"), E.get("tp_body")
    for j in range(1, k + 1):
        assert np.abs(tp[j, 0] - g["traj_p"][j - 1]).max() < 1e-7, j
        n = int(g["traj_nc"][j - 1])
        assert int(tnc[j, 0]) == n, (j, int(tnc[j, 0]), n)
        assert [tuple(r) for r in tb[j, 0][:, :n].T] == [tuple(r) for r in g["traj_body"][j - 1][:n]], j
    scale = max(1.0, np.abs(g["traj_p"][k]).max())
    assert np.abs(pose[0] - g["traj_p"][k]).max() < 1e-7 * scale and np.abs(vel[0] - g["traj_v"][k]).max() < 1e-6
    assert (pose == pose[:1]).all() and (vel == vel[:1]).all(), "replicated scenes diverged"
    for s in (0, 1):
        R.check_contacts(E, s, g["traj_body"][k], g["traj_geom"][k], int(g["traj_nc"][k]))
    assert int((g["traj_nc"] > 0).sum()) >= 5      # (the golden is not a free flight)


def test_latent_gradient_matches_reference_autograd():
    """d loss / d latent (4 numbers) of the demo's loss through the whole rollout, three ways as in the reference: the network's
    value at the contact points (reverse sweep -> g_latent), the level-set mesh (vertex adjoint -> MeshSDF backward) and the
    inertia integrated over it.  The mesh is the device's own, so poses agree to ~1e-9 rather than bit for bit."""
    from diffsdfsim_amd import mass_properties, meshsdf
    from diffsdfsim_amd.physics3d import BatchWorld3D
    name = "rollout_igr256_small"
    g, P = golden(name), packed(name)
    k, nb = int(g["igr_body"]), len(g["mass"])
    assert float(g["igr_scale"]) == 1.0 and float(g["mass"][k]) == 1.0
    latent = torch.tensor(g["latent"], dtype=torch.float64, requires_grad=True)
    v, f = meshsdf.igr_mesh(latent, P, res=128)
    assert tuple(g["meshsize_%d" % k]) == (len(v), len(f))
    J = mass_properties.mesh_inertia_diff(v, f, torch.tensor(1.0, dtype=torch.float64)).cpu()
    g2 = dict(g)
    g2["verts_%d" % k], g2["faces_%d" % k] = v.detach().cpu().numpy(), f.cpu().numpy()
    spec = spec256(name, 1, g2)
    spec["inertia"][0, k] = J.detach().numpy()
    table = torch.cat([torch.zeros(1, k, 4, dtype=torch.float64), latent.reshape(1, 1, 4), torch.zeros(1, nb - k - 1, 4, dtype=torch.float64)], 1)
    inertia = torch.cat([torch.tensor(spec["inertia"][:, :k]), J.reshape(1, 1, 3, 3), torch.tensor(spec["inertia"][:, k + 1:])], 1)
    verts = torch.cat([torch.as_tensor(m[0], dtype=torch.float64).to(v.device) if i != k else v for i, m in enumerate(spec["meshes"])])
    w = BatchWorld3D(spec, params=dict(igr_latent=table, inertia=inertia, verts=verts), dt=float(g["dt"]), eps=float(g["eps"]),
                     tol=float(g["tol"]), fric_dirs=int(g["fric_dirs"]), strict_no_penetration=bool(g["strict_no_pen"]),
                     max_substeps=128, maxc=64, max_cand=4096, max_pc=64)
    n = run_like_run_world(lambda: w.step(fixed_dt=False, keep_undo=False), lambda: float(w.t[0]), float(g["run_time"]))
    assert n == len(g["traj_t"])
    pose = w.pose[0, k]
    assert np.abs(pose.detach().cpu().numpy() - g["traj_p"][-1][k]).max() < 1e-6
    loss = (pose[4:] - torch.tensor(g["target"], device=pose.device)).norm() ** 2 + 0.05 * latent.norm() ** 2
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    loss.backward()
    got, want = latent.grad.cpu().numpy(), g["grad_latent"]
    print("d loss / d latent: got %s want %s" % (got, want))
    assert want.shape == (4,) and np.abs(want).min() >= 1e-3 * np.abs(want).max()
    assert np.abs(got - want).max() < 1e-5 * np.abs(want).max(), (got, want)


def test_push_scene_gradients_match_reference_autograd():
    """experiments.push_world on the shapenet network, 8 fixed steps: the reference's trajectory, and d sum_t |pos_t - target_t|^2
    / d (push, mass, friction coefficient, latent code) equal to its autograd values."""
    from diffsdfsim_amd.experiments import push_world
    name = "rollout_igr256_push"
    g, P = golden(name), packed(name)
    latent = torch.tensor(g["latent"][None], dtype=torch.float64, requires_grad=True)
    force = torch.tensor(g["force"][None], dtype=torch.float64, requires_grad=True)
    mass = torch.tensor([float(g["mass_push"])], dtype=torch.float64, requires_grad=True)
    fric = torch.tensor([float(g["fric_push"])], dtype=torch.float64, requires_grad=True)
    w = push_world(latent, P, force, mass, fric, int(g["nsteps"]))
    assert tuple(g["meshsize_1"]) == (int(w.engine.get("mesh_nv")[1]), int(w.engine.get("mesh_nf")[1]))
    assert np.abs(w.engine.get("pose")[0] - g["pose0"]).max() < 1e-7      # (the start height comes from the mesh)
    loss = 0.0
    for k in range(int(g["nsteps"])):
        w.step(fixed_dt=True, keep_undo=False)
        loss = loss + ((torch.tensor(g["target"][k], device=w.pose.device) - w.pose[0, 1, 4:]) ** 2).sum()
    E = w.engine
    nsub = int(E.get("nsub")[0])
    assert nsub == len(g["traj_t"])
    tp, tnc = E.get("tp_pose"), E.get("tp_nc")
    for j in range(1, nsub):
        assert np.abs(tp[j, 0] - g["traj_p"][j - 1]).max() < 1e-6, j
        assert int(tnc[j, 0]) == int(g["traj_nc"][j - 1]), j
    assert np.abs(w.pose[0].detach().cpu().numpy() - g["traj_p"][-1]).max() < 1e-6
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-7
    loss.backward()
    for key, t in (("grad_force", force), ("grad_mass", mass), ("grad_fric", fric), ("grad_latent", latent)):
        got, want = t.grad.cpu().numpy().reshape(-1), g[key].reshape(-1)
        print(key, "got", got, "want", want)
        assert np.abs(got - want).max() < 1e-5 * np.abs(want).max(), (key, got, want)


def sdf_path_disagreement(name, steps=4):
    """The push scene of golden `name` with mesh and inertia frozen (the golden's mesh, constants of the spec) and only the
    latent code where the SDF queries read it differentiable: the reverse sweep's d loss / d latent against central differences
    of the same run.  The base code and its 2 L perturbed copies are the scenes of ONE batch (scenes never read each other).
    Returns max_k |g_k - fd_k| / max_k |fd_k|."""
    from diffsdfsim_amd import mass_properties
    from diffsdfsim_amd.experiments import push_world
    g, P = golden(name), packed(name)
    base = np.asarray(g["latent"], np.float64)
    L = len(base)
    key = "igr_latent" if L == 4 else "shape_prm"
    v, f = g["verts_1"], g["faces_1"]
    J = np.asarray(mass_properties.mesh_inertia(v, f, 1.0).cpu())
    mass0, fric0 = (float(g["mass_push"]), float(g["fric_push"])) if "mass_push" in g else (float(g["mass"]), float(g["fric"]))
    dt = float(g["dt"])
    ngold = int((g["traj_t"] < steps * dt - 1e-9).sum())      # the golden's sub-steps inside the first `steps` outer steps
    for h in (1e-4, 1e-5, 1e-6):
        lats = np.stack([base] + [base + sg * h * np.eye(L)[k] for k in range(L) for sg in (1, -1)])
        B = len(lats)
        one = torch.ones(B, dtype=torch.float64)
        w = push_world(lats, P, torch.tensor(g["force"], dtype=torch.float64).expand(B, 2), mass0 * one, fric0 * one, steps,
                       mesh_cache={tuple(l): (v, f, J) for l in lats})
        E = w.engine
        t = E.arr[key].clone().requires_grad_()
        w.params[key] = t
        loss = 0.0
        for k in range(steps):
            w.step(fixed_dt=True, keep_undo=False)
            loss = loss + ((torch.tensor(g["target"][k], device=w.pose.device) - w.pose[:, 1, 4:]) ** 2).sum(dim=1)
        nsub, tnc, tb = E.get("nsub"), E.get("tp_nc"), E.get("tp_body")
        # scene 0 is the golden's run: its contact counts (and pairs, where the golden stores them) at every sub-step
        assert int(nsub[0]) == ngold, (nsub, ngold)
        for j in range(1, ngold):
            n = int(g["traj_nc"][j - 1])
            assert int(tnc[j, 0]) == n, (j, int(tnc[j, 0]), n)
            if "traj_body" in g:
                assert [tuple(r) for r in tb[j, 0][:, :n].T] == [tuple(r) for r in g["traj_body"][j - 1][:n]], j
        assert int(E.get("nc")[0]) == int(g["traj_nc"][ngold - 1])
        # every perturbed run has the same contact pairs at every sub-step, or h shrinks
        same = (nsub == nsub[0]).all() and (E.get("nc") == E.get("nc")[0]).all() and \
            all(np.array_equal(tnc[:ngold, s], tnc[:ngold, 0]) and
                all(np.array_equal(tb[j, s][:, :tnc[j, 0]], tb[j, 0][:, :tnc[j, 0]]) for j in range(ngold)) for s in range(1, B))
        if not same:
            print("%s: h = %g changes the contact pairs of a perturbed run" % (name, h))
            continue
        loss[0].backward()
        got = t.grad[0, 1, :L].cpu().numpy()
        lv = loss.detach().cpu().numpy()
        fd = np.array([(lv[1 + 2 * k] - lv[2 + 2 * k]) / (2 * h) for k in range(L)])
        assert not t.grad[1:].any() and np.abs(fd).max() > 0
        err = float(np.abs(got - fd).max() / np.abs(fd).max())
        print("%s: h = %g  reverse sweep %s  central differences %s  disagreement %.3e" % (name, h, got, fd, err))
        return err
    raise AssertionError("%s: no step h keeps the contact pairs of the perturbed runs" % name)


def test_sdf_path_latent_adjoint_against_central_differences():
    """The yardstick is the same test body on the (128, 2) network with rollout_igr_push's scene, a path that exists without the
    latent table: the 256-wide network sums twice as many terms per layer and its contact points differ, so it is allowed
    10 x that disagreement.  Central differences see the whole dependence of the run on the code (the normal, the point the
    Frank-Wolfe search lands on); the reverse sweep is the reference's autograd model, where the normal and the barycentrics
    are constants (SDF3D.query_sdfs, bodies.py:727-745), so the two differ by far more than rounding on BOTH networks and only
    their ratio is bounded.  Measured on an MI355X: 3.3e2 (128 / 2, h = 1e-6) and 7.6e2 (256 / 4, h = 1e-5); DESIGN.md section 2."""
    e128 = sdf_path_disagreement("rollout_igr_push")
    e256 = sdf_path_disagreement("rollout_igr256_push")
    print("disagreement with central differences: 128 / 2 network %.3e, 256 / 4 network %.3e" % (e128, e256))
    assert e256 <= 10 * e128, (e256, e128)


def test_missing_latent_table_is_an_argument_error():
    """A (256, 4) network without the table, or the table without g_latent: DSS_E_BADARG from the three entry points, nothing
    launched (the state is untouched and the device is healthy afterwards)."""
    from diffsdfsim_amd import world_abi as abi
    from diffsdfsim_amd.engine import BatchEngine
    g = golden("rollout_igr256_small")
    E = BatchEngine(spec256("rollout_igr256_small", 1), **H.engine_kwargs(g, max_sub=16))
    E.step_once()
    E._adjoint()
    L, W, A = E.be.lib, E.W, E.A
    before = {k: E.get(k).copy() for k in ("pose", "vel", "nc", "nsub", "t", "c_geom")}
    BADARG = -1
    table = W.igr_latent
    assert table and A.g_latent and W.igr.latent == 4 and W.igr.width == 256
    W.igr_latent = None
    try:
        assert L.dss_find_contacts(ctypes.byref(W), E.be.stream()) == BADARG
        assert L.dss_step_attempt(ctypes.byref(W), E.be.ptr(E.lcp_ws), E.lcp_ws_bytes, E.be.stream()) == BADARG
        assert L.dss_step_backward(ctypes.byref(W), ctypes.byref(A), E.be.stream()) == BADARG
    finally:
        W.igr_latent = table
    g_latent = A.g_latent
    A.g_latent = None
    try:
        assert L.dss_step_backward(ctypes.byref(W), ctypes.byref(A), E.be.stream()) == BADARG
    finally:
        A.g_latent = g_latent
    torch.cuda.synchronize()
    for k, a in before.items():
        assert np.array_equal(E.get(k), a), k
    assert abi.ABI_VERSION == L.dss_abi_version() == 4
    E.step_once()      # and the engine goes on
    assert int(E.get("nsub")[0]) == 2


def test_latent_table_with_the_128_wide_network_is_refused():
    from diffsdfsim_amd.engine import BatchEngine
    g = golden("rollout_igr_small")
    spec = H.spec_from_golden(g, 1, packed=packed("rollout_igr_small"))
    spec["igr_latent"] = np.zeros((1, len(g["mass"]), 4))
    with pytest.raises(ValueError, match="igr_latent"):
        BatchEngine(spec, **H.engine_kwargs(g))
    spec = spec256("rollout_igr256_small", 1)
    del spec["igr_latent"]
    with pytest.raises(ValueError, match="igr_latent"):
        BatchEngine(spec, **H.engine_kwargs(golden("rollout_igr256_small")))


def test_free_running_reproduces_lock_step():
    """Four copies of rollout_igr256_small with the neural body started at four heights, 6 outer steps with BatchEngine.run and
    with step(): every array is identical bit for bit."""
    from diffsdfsim_amd.engine import BatchEngine
    g = golden("rollout_igr256_small")
    out = []
    for free in (False, True):
        spec = spec256("rollout_igr256_small", 4)
        mv = int(g["igr_body"])
        f = spec["fext"][0, mv, 3:]
        up = -f / np.linalg.norm(f)
        for s, dz in enumerate((0.0, 0.011, 0.023, 0.037)):
            spec["pose"][s, mv, 4:] += dz * up
        E = BatchEngine(spec, **H.engine_kwargs(g, max_sub=128))
        rounds = E.run(6) if free else sum(E.step() for _ in range(6))
        assert int(E.get("overflow").max()) == 0
        out.append((rounds, {k: E.get(k).copy() for k in ("pose", "vel", "t", "nsub", "nc", "c_geom", "tp_pose", "tp_vel", "tp_dt", "tp_nc", "tp_lam")}))
    (r0, a), (r1, b) = out
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    print("attempt rounds: lock-step %d, free-running %d; sub-steps per scene %s" % (r0, r1, a["nsub"]))
    assert len(set(a["nsub"])) > 1, "the scenes were meant to differ"
    assert r1 <= r0
