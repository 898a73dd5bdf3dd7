"""Golden rollouts of a neural-SDF body on the shapenet network (latent 4, 8 x 256, skip into layer 4) through the reference's
own ``SDF3D.query_sdfs`` / ``FWContactHandler`` / ``World3D``, in the .npz layout of oracle/gen/gen_igr_golden.py.

Run on the CPU, in the build container only (it needs the reference tree):  python tools/gen_igr_shapenet_golden.py [name ...]

The network is ``tests/implicit_net.geometric_init(seed, radius_init, **SHAPENET)`` held by ``implicit_net.torch_module``
(trained shapenet weights are not available offline); the forward pass around those layers is the stand-in class of
oracle/refshim/fake_igr.py.  The neural body's latent code is stored as ``igr_latent [nb][4]`` (its shape_prm row stays
zero), the network shape as ``igr_width`` / ``igr_latent_size`` next to seed and radius.

  rollout_igr256_small   an analytic floor, the neural body (scale 1) released 0.03 above it, moving down and sideways,
                         run_time 0.4; the demo's loss (demo_meshsdf.py:89) and d loss / d latent from torch.autograd
  rollout_igr256_push    the scene of experiments/system_identification/optim_sysid.py:104-131, 8 fixed steps; gradients
                         w.r.t. push, mass, friction coefficient and the latent code

The generator asserts what keeps the tests from passing vacuously: contacts in at least 5 recorded sub-steps, both normal
choices (traj_stable) present, every component of the latent gradient at least 1e-3 of its largest.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
import implicit_net as IN  # noqa: E402
from oracle.refshim import fake_igr  # noqa: E402
from oracle.gen import gen_igr_golden as G128  # noqa: E402  (installs the hook that records the normal choice: _STABLE)
from oracle.gen.gen_rollout_golden import contacts_arrays, MAXC  # noqa: E402
from sdf_physics.physics3d.bodies import SDF3D, SDFBox  # noqa: E402
from sdf_physics.physics3d.constraints import TotalConstraint3D  # noqa: E402
from sdf_physics.physics3d.forces import ExternalForce3D, Gravity3D  # noqa: E402
from sdf_physics.physics3d.utils import Defaults3D, decode_igr, get_tensor  # noqa: E402
from sdf_physics.physics3d.world import World3D  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED, RADIUS = 126, 0.6                       # tests/test_igr_shapenet_gpu.py
LATENT = (0.05, -0.08, 0.06, -0.04)


def network(seed, radius):
    Ws, bs = IN.geometric_init(seed=seed, radius_init=radius, **IN.SHAPENET)
    net = fake_igr.ImplicitNet(d_in=IN.SHAPENET["d_in"], dims=IN.SHAPENET["dims"], skip_in=IN.SHAPENET["skip_in"],
                               geometric_init=False, beta=100).double()
    net.load_state_dict(IN.torch_module(Ws, bs).state_dict())
    net.eval()
    return net


def describe(w, bodies, obj, latent0, seed, radius, fixed):
    nb, k = len(bodies), bodies.index(obj)
    d = dict(igr_seed=seed, igr_radius=radius, igr_width=IN.SHAPENET["dims"][0], igr_latent_size=len(latent0),
             latent=np.array(latent0), igr_body=k, igr_scale=float(obj.scale), dt=w.dt, eps=w.eps, tol=w.tol, fric_dirs=w.fric_dirs,
             toc_diff=1, strict_no_pen=int(w.strict_no_pen), fixed=np.array(fixed, np.int32))
    d["kind"] = np.array([0 if isinstance(b, SDFBox) else 6 for b in bodies], np.int32)
    d["shape_prm"] = np.stack([b.dims.detach().numpy() if isinstance(b, SDFBox) else np.zeros(3) for b in bodies])
    lat = np.zeros((nb, 4)); lat[k] = latent0
    d["igr_latent"] = lat
    d["custom_mesh"] = np.array([int(isinstance(b, SDFBox)) for b in bodies])
    d["no_contact"] = np.array([[int(o.geom in b.geom.no_contact) for o in bodies] for b in bodies], np.uint8)
    d["pose0"] = np.stack([b.p.detach().numpy() for b in bodies])
    d["vel0"] = np.stack([b.v.detach().numpy() for b in bodies])
    d["mass"] = np.array([float(b.mass) for b in bodies])
    d["inertia"] = np.stack([b.ang_inertia.detach().numpy() for b in bodies])
    d["restitution"] = np.array([float(b.restitution) for b in bodies])
    d["fric"] = np.array([float(b.fric_coeff) for b in bodies])
    d["fext"] = np.stack([b.apply_forces(0.0).detach().numpy() for b in bodies])
    for i, b in enumerate(bodies):
        d["meshsize_%d" % i] = np.array([len(b.verts), len(b.faces)])
    d["verts_%d" % k] = obj.verts.detach().numpy()
    d["faces_%d" % k] = obj.faces.numpy().astype(np.int32)
    d["init_body"], d["init_geom"] = contacts_arrays(w.contacts)
    return d


def record_trajectory(w, d, stab):
    """Every entry of world.trajectory (one per accepted sub-step) with its ordered contacts and their normal choice; `stab`
    has one array per world.step() call, which is one trajectory entry only when stepping like run_world."""
    nb, T = d["pose0"].shape[0], len(w.trajectory)
    d["traj_t"] = np.array([float(e[0]) for e in w.trajectory])
    d["traj_p"] = np.stack([e[1].detach().numpy().reshape(nb, 7) for e in w.trajectory])
    d["traj_v"] = np.stack([e[2].detach().numpy().reshape(nb, 6) for e in w.trajectory])
    nc = np.array([len(e[3]) for e in w.trajectory], np.int32)
    cb = np.zeros((T, MAXC, 2), np.int32); cg = np.zeros((T, MAXC, 10)); cs = np.full((T, MAXC), -1, np.int8)
    for j, e in enumerate(w.trajectory):
        b, g = contacts_arrays(e[3])
        cb[j, :len(b)] = b; cg[j, :len(b)] = g
        cs[j, len(b):] = 0
        if stab is not None and len(stab[j]) == len(b):
            cs[j, :len(b)] = stab[j]
    d["traj_nc"], d["traj_body"], d["traj_geom"], d["traj_stable"] = nc, cb, cg, cs
    d["t_final"] = float(w.t)
    return nc


def check(name, d, nc, grad):
    assert int((nc > 0).sum()) >= 5, (name, "sub-steps with contacts", nc.tolist())
    used = d["traj_stable"][d["traj_stable"] >= 0]
    live = np.concatenate([d["traj_stable"][j, :n] for j, n in enumerate(nc)])
    assert (live == 0).any() and (live == 1).any(), (name, "traj_stable values", np.unique(used))
    assert np.abs(grad).min() >= 1e-3 * np.abs(grad).max(), (name, "latent gradient", grad)


def run_small(name="rollout_igr256_small", run_time=0.4, gap=0.03, vel=(0, 0, 0.3, 0.4, -1.0, 0.1), target=(0.0, 0.5, 0.0),
              seed=SEED, radius=RADIUS, latent0=LATENT):
    t0 = time.time()
    net = network(seed, radius)
    latent = torch.tensor(latent0, dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        v0, _f0 = SDF3D._diff_marching_cubes(decode_igr(net))(latent.detach())
    fr = 0.3
    floor = SDFBox([0, -0.5, 0], [6.0, 1.0, 6.0], fric_coeff=fr, restitution=0.2, custom_mesh=True, custom_inertia=True)
    obj = SDF3D(pos=[0, float(-v0[:, 1].min()) + gap, 0], scale=1, sdf_func=decode_igr(net), params=[latent], vel=list(vel),
                fric_coeff=fr, restitution=0.2)
    obj.add_force(Gravity3D())
    bodies = [floor, obj]
    w = World3D(bodies, [TotalConstraint3D(floor)])
    print(name, "world built in %.1f s; meshes" % (time.time() - t0), [len(b.faces) for b in bodies], flush=True)
    d = describe(w, bodies, obj, latent0, seed, radius, (0,))
    d["run_time"], d["target"] = run_time, np.array(target)
    stab = []
    while w.t < run_time:
        del G128._STABLE[:]
        ts = time.time()
        w.step()
        stab.append(np.concatenate(G128._STABLE) if G128._STABLE else np.zeros(0, bool))
        print("  t=%.4f nc=%d (%.1f s)" % (w.t, len(w.contacts), time.time() - ts), flush=True)
    nc = record_trajectory(w, d, stab)
    loss = (obj.pos - get_tensor(list(target))).norm() ** 2 + 0.05 * latent.norm() ** 2      # demo_meshsdf.py:89
    g, = torch.autograd.grad(loss, [latent])
    d["loss"], d["grad_latent"] = float(loss), g.numpy()
    print(name, "steps", len(nc), "nc", nc.tolist(), "loss", float(loss), "d loss/d latent", g.numpy(), "%.0f s" % (time.time() - t0))
    check(name, d, nc, g.numpy())
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)


def run_push(name="rollout_igr256_push", nsteps=8, seed=SEED, radius=RADIUS, latent0=LATENT, force0=(3.0, 2.5), mass0=1.0, fric0=0.1):
    t0 = time.time()
    net = network(seed, radius)
    latent = torch.tensor(latent0, dtype=torch.float64, requires_grad=True)
    force = torch.tensor(force0, dtype=torch.float64, requires_grad=True)
    mass = torch.tensor([mass0], dtype=torch.float64, requires_grad=True)
    fric = torch.tensor([fric0], dtype=torch.float64, requires_grad=True)

    def force_func(t):
        fv = get_tensor([0, 0, 0, 0, 0, 0])
        fv[[-3, -1]] = force
        return fv
    floor = SDFBox([0, -.5, 0], [20, 1, 20], fric_coeff=fric, restitution=0.0, custom_mesh=True, custom_inertia=True)
    obj = SDF3D([0, 0, 0], scale=1, sdf_func=decode_igr(net), params=[latent], mass=mass, fric_coeff=fric, restitution=0.0)
    obj_pos = get_tensor([0, 0, 0])
    obj_pos[1] = -obj.verts.detach().min(dim=0)[0][1] + 2 * Defaults3D.EPSILON
    obj.set_p(torch.cat([obj_pos.new_ones(1), obj_pos.new_zeros(3), obj_pos]))
    obj.add_force(Gravity3D())
    obj.add_force(ExternalForce3D(force_func))
    bodies = [floor, obj]
    w = World3D(bodies, [TotalConstraint3D(floor)], time_of_contact_diff=True, strict_no_penetration=False, fric_dirs=8)
    print(name, "world built in %.1f s; body mesh" % (time.time() - t0), len(obj.verts), len(obj.faces), "contacts", len(w.contacts), flush=True)
    d = describe(w, bodies, obj, latent0, seed, radius, (0,))
    d.update(force=np.array(force0), mass_push=mass0, fric_push=fric0, nsteps=nsteps)
    target = np.stack([obj.p.detach().numpy()[4:] + np.array([0.02, 0.0, 0.015]) * (k + 1) for k in range(nsteps)])
    loss = 0.0
    for k in range(nsteps):
        w.step(fixed_dt=True)
        loss = loss + ((get_tensor(target[k].tolist()) - obj.pos) ** 2).sum()
        print("  t=%.4f nc=%d" % (w.t, len(w.contacts)), flush=True)
    d["target"] = target
    nc = record_trajectory(w, d, None)
    gf, gm, gc, gl = torch.autograd.grad(loss, [force, mass, fric, latent])
    d["loss"], d["grad_force"], d["grad_mass"], d["grad_fric"], d["grad_latent"] = float(loss), gf.numpy(), gm.numpy(), gc.numpy(), gl.numpy()
    print(name, "sub-steps", len(nc), "nc", nc.tolist(), "loss", float(loss), "grads", gf.numpy(), gm.numpy(), gc.numpy(), gl.numpy(),
          "%.0f s" % (time.time() - t0))
    assert int((nc > 0).sum()) >= 5, (name, nc.tolist())
    assert np.abs(gl.numpy()).min() >= 1e-3 * np.abs(gl.numpy()).max(), (name, gl.numpy())
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)


CASES = {"rollout_igr256_small": run_small, "rollout_igr256_push": run_push}

if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](name)
