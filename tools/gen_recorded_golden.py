"""Generate tests/golden/recorded_fit.npz: what the reference's recorded-sequence experiment computes on small inputs.

    python tools/gen_recorded_golden.py      (needs the reference checkout that oracle/refshim imports)
experiments/trajectory_fitting/optim_pointcloud_real.py is imported through oracle/refshim; what the shim lacks for this script
(pytorch3d's axis_angle_to_quaternion, restated here from its documentation, and matplotlib / pyrender / tensorboard where they
are not installed) is put in place by this file.  The file holds data only:
  (a) plane_*      the poses make_world gives the plane boxes, for six plane sets (tilted floors, a wall, negative d, a
                   normal within 1e-3 of +y)
  (b) cloud_*      match_pointcloud's loss and sample count on three 24 x 18 organised clouds with labels (sphere, cube,
                   sphere with non-finite points)
  (c) roll_*       a sphere thrown over a tilted floor towards a wall, 12 frames, one bounce: make_world's trajectory
                   (run_world_fixed_dt), trajectory_loss against a stored organised cloud, autograd's gradient w.r.t. rad, pos,
                   rot, vel, fric and restitution; and the frames run_world_fixed_dt(detach_2nd_bounce=True) steps twice.
The worlds are built with custom_mesh = custom_inertia = True (analytic meshes and inertias), as every golden of this project."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from oracle.refshim import fake_pytorch3d  # noqa: E402


def axis_angle_to_quaternion(axis_angle):
    """pytorch3d.transforms.axis_angle_to_quaternion as documented: (cos(a / 2), axis_angle sin(a / 2) / a), a = |axis_angle|,
    with sin(a / 2) / a ~ 1/2 - a^2 / 48 for a < 1e-6."""
    a = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    small = a.abs() < 1e-6
    s = torch.where(small, 0.5 - a * a / 48, torch.sin(0.5 * a) / torch.where(small, torch.ones_like(a), a))
    return torch.cat([torch.cos(0.5 * a), axis_angle * s], dim=-1)


refshim.install()
if not hasattr(fake_pytorch3d, "axis_angle_to_quaternion"):
    fake_pytorch3d.axis_angle_to_quaternion = axis_angle_to_quaternion
for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.image", "pyrender"):
    try:
        __import__(name)
    except Exception:
        m = types.ModuleType(name)
        m.__getattr__ = lambda item: None
        sys.modules[name] = m
import optim_pointcloud_real as ref_exp  # noqa: E402
from pytorch3d.transforms import quaternion_to_matrix  # noqa: E402
from sdf_physics.physics3d.bodies import SDFBoxRounded, SDFSphere  # noqa: E402

D = torch.double
W, H, F = 24, 18, 19.3125      # the experiment's 515 at 24 / 640 of its width
WORLD = dict(use_toc_diff=True, use_gravity=True, custom_mesh=True, custom_inertia=True, strict_no_penetration=True)


def organised_cloud(centre, r, seed, nonfinite=False, W=W, H=H):
    """What a depth sensor at the origin (looking along -z) reports of a sphere in front of a plane of depth 2: the point each
    pixel sees (coordinates on a grid of 2^-24, which halves the stored file), the label image (the sphere 4, the plane 1, a
    patch of 2)."""
    rng = np.random.default_rng(seed)
    F = globals()["F"] * W / 24
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(col + 0.5 - (W - 1) / 2) / F, -(row + 0.5 - (H - 1) / 2) / F, -np.ones((H, W))], -1)
    a, b = (d * d).sum(-1), d @ centre
    disc = b * b - a * (centre @ centre - r * r)
    hit = disc > 0
    t = np.where(hit, (b - np.sqrt(np.maximum(disc, 0))) / a, 2.0)
    pcs = np.round((d * t[..., None] + 1e-3 * rng.standard_normal((H, W, 3))) * 2.0 ** 24) / 2.0 ** 24
    segs = np.where(hit, 4, 1).astype(np.int32)
    segs[:3, :4] = 2
    if nonfinite:
        y, x = np.nonzero(hit)
        pcs[y[1], x[1], 0] = np.nan; pcs[y[5], x[5], 2] = np.inf; pcs[y[7], x[7], 1] = -np.inf
        pcs[0, 0] = np.nan
    return pcs, segs


def planes_part(out):
    n3 = lambda v: list(np.asarray(v) / np.linalg.norm(v))
    sets = [
        [[0.0, 1.0, 0.0 + 1e-9, 0.3], [-1.0, 0.0, 1e-9, 0.4]],
        [n3([0.05, 1.0, -0.03]) + [0.45], n3([-1.0, 0.04, 0.02]) + [0.7]],
        [n3([0.2, 0.9, 0.3]) + [-0.6], n3([0.0, 0.1, 1.0]) + [1.2]],            # negative d
        [n3([6e-4, 1.0, -5e-4]) + [0.5], n3([1.0, 0.0, 0.3]) + [-0.8]],          # within 1e-3 of +y
        [[0.1, 1.9, -0.2, 0.25], [-2.0, 0.3, 0.1, 0.9]],                         # not normalised
        [n3([0.3, -0.9, 0.1]) + [0.4], n3([-0.5, 0.5, 0.7]) + [0.33]],           # a ceiling
    ]
    poses = []
    for pl in sets:
        world, _ = ref_exp.make_world(torch.tensor(0.05, dtype=D), torch.tensor(pl, dtype=D), torch.tensor(0.15, dtype=D), torch.tensor(0.7, dtype=D),
                                      sphere_pose=torch.tensor([1.0, 0, 0, 0, 0, 5.0, 0], dtype=D), shape="sphere", **WORLD)
        poses.append(torch.stack([b.p.detach() for b in world.bodies[:-1]]).numpy())
    out["plane_sets"], out["plane_poses"] = np.array(sets), np.array(poses)


def clouds_part(out):
    r = np.random.default_rng(3)
    res = dict(pcs=[], segs=[], kind=[], prm=[], pose=[], loss=[], count=[])
    for k, (kind, nonfinite) in enumerate(((1, False), (3, False), (1, True))):
        centre, rad = np.array([0.05 * k - 0.05, 0.02, -0.6]), 0.1
        pcs, segs = organised_cloud(centre, rad, 10 + k, nonfinite)
        z = [0, 0, 0]
        est_r = 0.12
        body = SDFSphere(z, est_r, custom_mesh=True, custom_inertia=True) if kind == 1 else \
            SDFBoxRounded(z, torch.tensor([2 * est_r] * 3, dtype=D), 0.02)
        q = r.standard_normal(4) if kind == 3 else np.array([1.0, 0, 0, 0])
        q /= np.linalg.norm(q)
        pos = centre + r.uniform(-0.02, 0.02, 3)
        loss, count = ref_exp.match_pointcloud(torch.tensor(pcs, dtype=D), torch.tensor(segs), body, torch.tensor(pos, dtype=D),
                                               quaternion_to_matrix(torch.tensor(q, dtype=D)))
        print("cloud %d kind %d: labelled %d, in the cube %d, loss %.6e" % (k, kind, int((segs == 4).sum()), int(count), float(loss)))
        assert np.isfinite(float(loss))
        for key, v in zip(("pcs", "segs", "kind", "prm", "pose", "loss", "count"),
                          (pcs, segs, kind, [est_r, 0, 0, 0] if kind == 1 else [2 * est_r] * 3 + [0.02], np.concatenate([q, pos]), float(loss), int(count))):
            res[key].append(v)
    for k, v in res.items():
        out["cloud_" + k] = np.array(v, np.int32 if k in ("segs", "kind") else (np.int64 if k == "count" else np.float64))


def rollout_part(out):
    n3 = lambda v: list(np.asarray(v) / np.linalg.norm(v))
    planes = torch.tensor([n3([0.04, 1.0, -0.03]) + [0.3], n3([-1.0, 0.03, 0.02]) + [0.4]], dtype=D)
    T, g = 12, 9.81
    leaf = lambda v: torch.tensor(v, dtype=D, requires_grad=True)
    rad, rot, pos = leaf(0.1), leaf([1.0, 0, 0, 0]), leaf([-0.25, -0.05, -0.6])
    vel, fric, rest = leaf([0.0, 0, 0, 1.2, 0.5, 0.1]), leaf(0.15), leaf(0.7)

    def world(rest=rest):
        return ref_exp.make_world(rad, planes, fric, rest, sphere_pose=torch.cat([rot, pos]), sphere_vel=vel, g=g, shape="sphere", **WORLD)
    w, sphere = world()
    frames = torch.zeros(T, 1)      # (run_world_fixed_dt reads pcs.shape[0] alone)
    traj = ref_exp.run_world_fixed_dt(w, frames, detach_2nd_bounce=False)
    tp = torch.stack(traj).detach().numpy()
    # the observation: a slightly larger sphere a little off the reference trajectory, seen from the origin
    pcs, segs = [], []
    for i in range(T):
        c = tp[min(i, T - 2), 4:] + np.array([0.004, -0.003, 0.005])
        p, s = organised_cloud(c, 0.105, 100 + i, W=16, H=12)      # (no non-finite point: autograd there turns one into NaN gradients)
        pcs.append(p); segs.append(s)
    pcs, segs = np.array(pcs), np.array(segs, np.int32)
    obs = dict(pcs=torch.tensor(pcs, dtype=D), segs=torch.tensor(segs))
    loss = ref_exp.trajectory_loss(traj, sphere, obs)[0]
    loss.backward()
    bounce = [i for i in range(1, T - 1) if tp[i, 5] - tp[i - 1, 5] > 0 > tp[i - 1, 5] - tp[max(i - 2, 0), 5]]
    print("rollout: %d entries, loss %.6e, the height turns upwards at entries %s" % (len(traj), float(loss), bounce))
    out.update(roll_planes=planes.numpy(), roll_g=g, roll_rad=float(rad), roll_pose=torch.cat([rot, pos]).detach().numpy(), roll_vel=vel.detach().numpy(),
               roll_fric=float(fric), roll_restitution=float(rest), roll_traj=tp, roll_pcs=pcs, roll_segs=segs, roll_loss=float(loss),
               roll_g_rad=float(rad.grad), roll_g_pos=pos.grad.numpy(), roll_g_rot=rot.grad.numpy(), roll_g_vel=vel.grad.numpy(),
               roll_g_fric=float(fric.grad), roll_g_restitution=float(rest.grad))
    # the frames the script steps twice with detach_2nd_bounce, for a ball that stays down after it lands (restitution 0.05)
    w2, _ = world(torch.tensor(0.05, dtype=D))
    undone = []
    undo = w2.undo_step

    def logged():
        undone.append(len(traj2_len))
        return undo()
    traj2_len = []
    w2.undo_step = logged
    step = w2.step

    def counted(*a, **k):
        traj2_len.append(0)
        return step(*a, **k)
    w2.step = counted
    traj2 = ref_exp.run_world_fixed_dt(w2, frames, detach_2nd_bounce=True)
    # call number c (1-based) that was undone stepped frame c - (undone calls before it); frames count from 1
    repeated = [c - k for k, c in enumerate(undone)]
    print("detach_2nd_bounce: %d step calls, frames stepped twice %s" % (len(traj2_len), repeated))
    out.update(roll_detach_restitution=0.05, roll_repeated=np.array(repeated, np.int64), roll_traj_detach=torch.stack(traj2).detach().numpy())


def main():
    torch.manual_seed(0)
    out = {}
    planes_part(out)
    clouds_part(out)
    rollout_part(out)
    path = os.path.join(ROOT, "tests", "golden", "recorded_fit.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
