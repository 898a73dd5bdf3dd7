"""Generate the `rollout_general_*` goldens: d(general terminal loss) / d(EVERY physical leaf) from the reference's CPU path.

Run in the build container only:  python -m oracle.gen.gen_general_golden [case ...]   (default: all; ~2 minutes)

The rollout goldens of gen_rollout_golden.py record d sum|pos_T|^2 / d shape only.  Here every quantity the reverse sweep
(csrc/step_bwd.hip) produces has a reference value: the scenes are built with tensor LEAVES for the mass, friction
coefficient and restitution of every body (the pinned floor too), for the start pose (the 7-number `p` handed to
`Body3D.set_p`, so that the quaternion rows have a reference value), the start velocity, a constant wrench applied through
`ExternalForce3D` next to gravity, and the shape parameters; the loss

    sum_b  cp_b . p_b + cv_b . v_b + 0.5 |p_b|^2        (moving bodies b; p_b the final 7-number pose, v_b the final velocity)

seeds every row of the sweep's incoming adjoint (cp, cv: seeded normal vectors, stored).  Per leaf `grad_<leaf>` (run A) and
`gradB_<leaf>` (the 1e-13-nudged run B, see gen_rollout_golden.branch_b_grads); with `parts`, also `grad_quatonly_<leaf>`
(loss = the quaternion rows' terms alone) and `grad_velonly_<leaf>` (loss = sum cv_b . v_b).  Leaf names: mass_<b>, fric_<b>,
rest_<b>, pose_<b>, vel_<b>, wrench_<b> (b = body index) and shape_<i> (i = index in rollout_helpers.param_grads' list).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.gen import gen_rollout_golden as G  # noqa: E402  (installs the stand-ins and the contact recorder)
from oracle.gen.gen_rollout_golden import World3D, contact_record, MAXC  # noqa: E402

GRAVITY = 10.0      # Gravity3D's default g (forces.py:74)
DEAD_RATIO = 1e-3   # every compared leaf carries at least this fraction of the scene's largest leaf gradient; the leaves
#                     listed as dead (the pinned floor's mass: it multiplies a velocity the constraint holds at zero, and the
#                     reference's graph returns rounding residue of ~1e-40 for it) must stay below 1e-12 of it


def _leaf(x):
    return torch.tensor(x, dtype=torch.double, requires_grad=True)


def _scene(floor_phys, movers, joints=(), walls=(), gravity=GRAVITY):
    """floor_phys = (mass, fric, rest), or None for a scene without floor; movers = [(kind, pos6, shape, vel6, (mass, fric, rest),
    wrench6)], kind in box / sphere / cylinder; joints = [(constraint class name, body index)] on top of the floor's and the walls'
    TotalConstraint3D; walls = [(pos6, dims, (mass, fric, rest))]: further pinned boxes, numbered after the floor and before the
    movers.  Returns (bodies, joints, leaves) with `leaves` an ordered {name: tensor}."""
    from sdf_physics.physics3d import constraints as C
    from sdf_physics.physics3d.bodies import SDFBox, SDFCylinder, SDFSphere
    from sdf_physics.physics3d.constraints import TotalConstraint3D
    from sdf_physics.physics3d.forces import ExternalForce3D, Gravity3D
    L = {}

    def phys(b, vals):
        for k, x in zip(("mass", "fric", "rest"), vals):
            L["%s_%d" % (k, b)] = _leaf(float(x))
        return dict(mass=L["mass_%d" % b], fric_coeff=L["fric_%d" % b], restitution=L["rest_%d" % b], custom_mesh=True, custom_inertia=True)
    bodies, shapes = [], []
    if floor_phys is not None:
        bodies.append(SDFBox([0, -0.5, 0], [4.0, 1.0, 4.0], **phys(0, floor_phys)))
    for pos, dims, ph in walls:
        bodies.append(SDFBox(list(pos), list(dims), **phys(len(bodies), ph)))
    pinned = list(bodies)
    for b, (kind, pos, shape, vel, ph, wrench) in enumerate(movers, start=len(bodies)):
        L["vel_%d" % b] = _leaf(list(vel))
        kw = dict(vel=L["vel_%d" % b], **phys(b, ph))
        if kind == "box":
            shapes.append(_leaf(list(shape)))
            body = SDFBox(list(pos), shapes[-1], **kw)
        elif kind == "sphere":
            shapes.append(_leaf(float(shape)))
            body = SDFSphere(list(pos), shapes[-1], **kw)
        else:
            shapes += [_leaf(float(shape[0])), _leaf(float(shape[1]))]
            body = SDFCylinder(list(pos), shapes[-2], shapes[-1], **kw)
        L["pose_%d" % b] = body.p.detach().clone().requires_grad_()
        body.set_p(L["pose_%d" % b])
        L["wrench_%d" % b] = _leaf(list(wrench))
        if gravity:
            body.add_force(Gravity3D(gravity))
        body.add_force(ExternalForce3D(lambda t, w=L["wrench_%d" % b]: w, multiplier=1.0))
        bodies.append(body)
    for i, s in enumerate(shapes):
        L["shape_%d" % i] = s
    return bodies, [TotalConstraint3D(b) for b in pinned] + [getattr(C, name)(bodies[b]) for name, b in joints], L


def boxdrop():
    """The tilted box of scenes.box_drop(seed=7): same dims, tilt, height and linear start velocity."""
    g = torch.Generator().manual_seed(7)
    dims = 0.5 + 0.2 * torch.rand(3, generator=g, dtype=torch.double)
    ang = 0.3 * (torch.rand(3, generator=g, dtype=torch.double) - 0.5)
    pos = ang.tolist() + [0.0, 0.25 + 0.5 * dims.max().item(), 0.0]
    return _scene((1.0, 0.55, 0.15), [("box", pos, dims.tolist(), [0.2, -0.1, 0.3, 0.8, -0.5, 0.2], (1.3, 0.3, 0.45),
                                       [0.05, -0.08, 0.06, 0.3, 0.2, -0.25])])


def sphere_on_box():
    """scenes.sphere_on_box's bodies with per-body physical parameters; the box is set down sliding (its friction against the
    floor saturates: the coefficients of floor and box carry a gradient) and sinking (a normal approach speed for the
    restitution of the floor-box contacts to act on); the sphere comes down on it spinning and against its motion, smooth
    enough to slide at the impact."""
    return _scene((1.0, 0.5, 0.1), [
        ("box", [0.0, 0.2005, 0.0], [0.8, 0.4, 0.7], [0, 0.3, 0, 0.8, -1.0, 0.3], (1.6, 0.2, 0.25), [0.02, 0.03, -0.02, 0.8, -0.3, 0.4]),
        ("sphere", [0.1, 0.4 + 0.2 + 0.15, 0.05], 0.2, [3.0, -0.3, 2.0, -1.5, -1.0, 0.1], (0.7, 0.05, 0.4), [0.01, -0.02, 0.015, -0.2, 0.1, 0.15])])


def cylinder():
    """scenes.cylinder_drop(seed=9)'s cylinder, spinning about its own axis (body z) as well."""
    g = torch.Generator().manual_seed(9)
    rad = 0.25 + 0.1 * torch.rand(1, generator=g, dtype=torch.double).item()
    height = 0.6 + 0.2 * torch.rand(1, generator=g, dtype=torch.double).item()
    # body z after the tilt of 1.2 rad about x points along (0, -sin 1.2, cos 1.2): 8 rad/s about it on top of the scene's spin
    spin = 8.0 * np.array([0.0, -np.sin(1.2), np.cos(1.2)])
    vel = (np.array([0.0, 0.2, 0.5]) + spin).tolist() + [0.4, -0.3, 0.1]
    return _scene((1.0, 0.1, 0.2), [("cylinder", [1.2, 0.3, 0.1, 0.0, 0.55, 0.0], (rad, height), vel, (0.8, 0.05, 0.4),
                                     [0.03, 0.02, -0.04, 0.2, 0.1, -0.15])])


def sphere():
    """scenes.sphere_drop(seed=1)'s sphere with per-body physical parameters, spinning against its motion on a smooth floor
    (it slides at every bounce: the friction coefficients carry a gradient)."""
    g = torch.Generator().manual_seed(1)
    r = (0.4 + 0.2 * torch.rand(1, generator=g, dtype=torch.double)).item()
    y = (0.7 + 0.5 * torch.rand(1, generator=g, dtype=torch.double)).item()
    v = torch.rand(1, generator=g, dtype=torch.double).item()
    return _scene((1.0, 0.1, 0.6), [("sphere", [0.1, -0.2, 0.15, 0.0, y, 0.0], r, [0.5, 0.3, 6.0, v, 0.0, 0.2], (1.4, 0.04, 0.4),
                                     [0.02, -0.03, 0.025, 0.8, 0.5, -0.6])])


# ---- scenes whose equality rows are not "six rows on body 0" (tests/test_step_constraints_gpu.py) ----
def rotlocked_box():
    """The tilted box of boxdrop() under RotConstraint3D (three unit rows on its angular velocity: neq = 9): it keeps its tilt,
    comes down on one corner through a time-of-contact event and slides on it (friction saturated)."""
    g = torch.Generator().manual_seed(7)
    dims = 0.5 + 0.2 * torch.rand(3, generator=g, dtype=torch.double)
    ang = 0.3 * (torch.rand(3, generator=g, dtype=torch.double) - 0.5)
    pos = ang.tolist() + [0.0, 0.25 + 0.5 * dims.max().item(), 0.0]
    return _scene((1.0, 0.55, 0.15), [("box", pos, dims.tolist(), [0.0, 0.0, 0.0, 1.5, -0.5, 0.6], (1.3, 0.3, 0.45),
                                       [0.05, -0.08, 0.06, 0.3, 0.2, -0.25])], joints=[("RotConstraint3D", 1)])


def planar_sphere():
    """A small sphere under ZConstraint (one unit row on its z velocity: neq = 7), spinning about all three axes against its
    motion on a smooth floor.  (Radius 0.45 rested on up to seven mesh contacts and the reference's own two runs were 1.7e-3
    apart; with 0.25 they agree to 1e-12.)"""
    return _scene((1.0, 0.1, 0.6), [("sphere", [0.1, -0.2, 0.15, 0.0, 0.5, 0.0], 0.25, [0.5, 0.3, 6.0, 0.7, 0.0, 0.0], (1.4, 0.04, 0.4),
                                     [0.02, -0.03, 0.025, 0.8, 0.5, -0.6])], joints=[("ZConstraint", 1)])


def two_pinned():
    """Floor and a pinned wall box (bodies 0 and 1: neq = 12, n = 18 + 12); a sphere thrown into the corner they form hits
    both.  The wall hangs 0.06 above the floor (standing on it, the two pinned bodies had 9-15 contacts with each other) and is
    smooth enough for the sphere to slide along it."""
    return _scene((1.0, 0.3, 0.3), [("sphere", [0.1, -0.2, 0.15, 0.0, 0.5, 0.0], 0.3, [1.0, 0.5, 3.0, 2.5, -1.0, 0.4], (1.4, 0.2, 0.4),
                                     [0.02, -0.03, 0.025, 0.6, 0.3, -0.4])],
                  walls=[([0, 0, 0, 1.0, 0.56, 0.0], [0.5, 1.0, 3.0], (2.0, 0.03, 0.5))])


def three_free():
    """No floor, no joint, no gravity (nb = 3, neq = 0: n = 18 without equality rows): a sphere and a second sphere fly at a
    slowly tumbling box from two sides."""
    return _scene(None, [
        ("sphere", [0.1, -0.2, 0.15, -0.75, 0.05, 0.0], 0.25, [1.0, 2.0, -1.5, 2.0, 0.3, 0.1], (0.9, 0.3, 0.4), [0.02, -0.03, 0.025, 0.2, 0.1, -0.1]),
        ("box", [0.2, -0.1, 0.15, 0.0, 0.0, 0.0], [0.6, 0.5, 0.7], [0.3, -0.2, 0.4, 0.0, 0.1, 0.0], (1.5, 0.4, 0.3), [0.03, 0.02, -0.04, -0.1, 0.2, 0.15]),
        ("sphere", [-0.1, 0.3, 0.2, 0.85, -0.05, 0.1], 0.3, [-2.0, 6.0, 5.0, -3.0, 0.2, -0.3], (1.1, 0.03, 0.5), [0.01, -0.02, 0.015, -0.2, 0.1, 0.15])],
        gravity=0.0)


LOSSES = ("", "quatonly_", "velonly_")


def losses(bodies, cp, cv, parts, fixed=(0,)):
    """The general terminal loss and, with `parts`, its quaternion-rows-only and velocity-only pieces."""
    mv = [(i, b) for i, b in enumerate(bodies) if i not in fixed]
    tcp, tcv = torch.as_tensor(cp), torch.as_tensor(cv)
    full = sum((tcp[i] * b.p).sum() + (tcv[i] * b.v).sum() + 0.5 * (b.p ** 2).sum() for i, b in mv)
    if not parts:
        return [full]
    quat = sum((tcp[i, :4] * b.p[:4]).sum() + 0.5 * (b.p[:4] ** 2).sum() for i, b in mv)
    velo = sum((tcv[i] * b.v).sum() for i, b in mv)
    return [full, quat, velo]


def rollout(make, nsteps, cp, cv, parts, jitter=0.0, fixed=(0,), **world_kw):
    bodies, joints, L = make()
    if jitter:
        with torch.no_grad():
            bodies[-1].v[3] += jitter
    w = World3D(bodies, joints, **world_kw)
    init = (G.contacts_arrays(w.contacts), contact_record.lookup(w.contacts, MAXC))
    for _ in range(nsteps):
        w.step(fixed_dt=True)
    ls = losses(bodies, cp, cv, parts, fixed)
    grads = []
    for l in ls:
        gr = torch.autograd.grad(l, list(L.values()), allow_unused=True, retain_graph=True)
        grads.append({k: (np.zeros_like(t.detach().numpy()) if g is None else g.numpy()) for (k, t), g in zip(L.items(), gr)})
    return bodies, w, L, init, [float(l) for l in ls], grads


def joint_rows(bodies, joints):
    """The equality rows as World3D stacks them: every joint's J() in the columns of its body."""
    nb = len(bodies)
    Je = np.zeros((sum(j.num_constraints for j in joints), 6 * nb))
    r = 0
    for j in joints:
        J1 = j.J()[0].detach().numpy()
        b = [k for k, o in enumerate(bodies) if o is j.body1][0]
        Je[r:r + len(J1), 6 * b:6 * b + 6] = J1
        r += len(J1)
    return Je


def run(name, make, nsteps, seed, toc=True, parts=False, dead=("mass_0",), fixed=(0,), gravity=GRAVITY, store_Je=False):
    bodies, joints, L = make()
    nb = len(bodies)
    d = G.describe(bodies)
    rng = np.random.default_rng(seed)
    cp, cv = rng.standard_normal((nb, 7)), rng.standard_normal((nb, 6))
    for b in fixed:
        cp[b] = 0.0; cv[b] = 0.0      # the pinned bodies are not part of the loss
    if store_Je:      # (rollout_helpers.spec_from_golden: otherwise six identity rows per body of `fixed`)
        d["Je"] = joint_rows(bodies, joints)
    bodies, w, L, (init_c, init_s), ls, grads = rollout(make, nsteps, cp, cv, parts, fixed=fixed, time_of_contact_diff=toc)
    d["dt"], d["eps"], d["tol"], d["fric_dirs"], d["toc_diff"] = w.dt, w.eps, w.tol, w.fric_dirs, int(toc)
    d["fixed"] = np.array(list(fixed), np.int32)
    d["strict_no_pen"], d["grad_flags"] = int(w.strict_no_pen), 0
    d["gravity"], d["loss_cp"], d["loss_cv"] = gravity, cp, cv
    d["init_body"], d["init_geom"] = init_c
    d["init_stable"], d["init_lap"] = init_s
    T = len(w.trajectory)
    d["traj_t"] = np.array([float(e[0]) for e in w.trajectory])
    d["traj_p"] = np.stack([e[1].detach().numpy().reshape(nb, 7) for e in w.trajectory])
    d["traj_v"] = np.stack([e[2].detach().numpy().reshape(nb, 6) for e in w.trajectory])
    nc = np.array([len(e[3]) for e in w.trajectory], np.int32)
    cb = np.zeros((T, MAXC, 2), np.int32); cg = np.zeros((T, MAXC, 10))
    for k, e in enumerate(w.trajectory):
        b, g = G.contacts_arrays(e[3])
        cb[k, :len(b)] = b; cg[k, :len(b)] = g
    d["traj_nc"], d["traj_body"], d["traj_geom"] = nc, cb, cg
    d["traj_stable"], d["traj_lap"] = G.stable_arrays(w.trajectory)
    d["t_final"], d["loss"] = float(w.t), ls[0]
    d["leaves"] = np.array(list(L))
    d["dead_leaves"] = np.array(list(dead))
    for k, t in L.items():
        d["leaf_" + k] = t.detach().numpy()
    for tag, gr in zip(LOSSES, grads):
        for k, v in gr.items():
            d["grad_%s%s" % (tag, k)] = v
    _b, wB, _L, (_ic, init_sB), _ls, gradsB = rollout(make, nsteps, cp, cv, parts, jitter=1e-13, fixed=fixed, time_of_contact_diff=toc)
    stB = G.stable_arrays(wB.trajectory)[0]
    d["init_stableB"] = init_sB[0]
    d["traj_stableB"] = stB if stB.shape == d["traj_stable"].shape else np.full_like(d["traj_stable"], -1)
    for tag, gr in zip(LOSSES, gradsB):
        for k, v in gr.items():
            d["gradB_%s%s" % (tag, k)] = v
    print("| `%s` | %d | %d-%d | %s |" % (name, T, nc.min(), nc.max(), ", ".join("%s %.3g" % (k, np.abs(v).max()) for k, v in grads[0].items())))
    for tag, gr in list(zip(LOSSES, grads))[1:]:
        print("|   (%s) | | | %s |" % (tag.rstrip("_"), ", ".join("%s %.3g" % (k, np.abs(v).max()) for k, v in gr.items())))
    spread = max(np.abs(grads[0][k] - gradsB[0][k]).max() / max(np.abs(grads[0][k]).max(), 1e-300) for k in grads[0] if k not in dead)
    print("|   (run A vs run B, worst leaf, relative) | | | %.1e |" % spread)
    # the condition on the inputs: no compared leaf is dead under any of the recorded losses
    for tag, gr in zip(LOSSES, grads):
        top = max(np.abs(v).max() for v in gr.values())
        for k, v in gr.items():
            if k in dead:
                assert np.abs(v).max() < 1e-12 * top, (name, tag, k, "listed as dead but carries a gradient")
            else:
                assert np.abs(v).max() >= DEAD_RATIO * top, (name, tag, k, np.abs(v).max(), top, "dead leaf: change the scene")
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **d)


CASES = {
    "rollout_general_boxdrop": (boxdrop, dict(nsteps=12, seed=101, parts=True)),
    "rollout_general_sphere_on_box": (sphere_on_box, dict(nsteps=12, seed=102)),
    "rollout_general_cylinder": (cylinder, dict(nsteps=10, seed=103)),
    "rollout_general_sphere_notoc": (sphere, dict(nsteps=24, seed=104, toc=False)),
    "rollout_general_rotlocked_box": (rotlocked_box, dict(nsteps=12, seed=105, store_Je=True)),
    "rollout_general_planar_sphere": (planar_sphere, dict(nsteps=16, seed=106, store_Je=True)),
    "rollout_general_two_pinned": (two_pinned, dict(nsteps=16, seed=117, store_Je=True, fixed=(0, 1), dead=("mass_0", "mass_1"))),
    "rollout_general_three_free": (three_free, dict(nsteps=14, seed=108, store_Je=True, fixed=(), dead=(), gravity=0.0)),
}


def main():
    """python -m oracle.gen.gen_general_golden [case ...]   (default: all)"""
    os.makedirs(G.OUT, exist_ok=True)
    print("| golden | sub-steps | contacts | max abs grad per leaf (run A) |\n|---|---|---|---|")
    for name in (sys.argv[1:] or list(CASES)):
        make, kw = CASES[name]
        run(name, make, **kw)


if __name__ == "__main__":
    main()
