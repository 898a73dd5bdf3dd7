"""Batched experiment drivers: the optimisation loops of the reference's `experiments/`, for a whole
batch of independent scenes at once, without sacred / tensorboard / pyrender.

trajectory fitting  (experiments/trajectory_fitting/optim_sphere.py)
    bounce_world(radii, ...)                      floor + wall + sphere thrown at the wall (:77-111), one scene per radius
    run_world_fixed_dt(world, run_time, detach_2nd_bounce)   fixed outer steps until every scene has reached run_time; with
                                                  detach_2nd_bounce the second step in a row that ends in contact is undone
                                                  and redone with poses and velocities cut from the graph (:163-177), per scene
    trajectory_loss(traj, traj_target)            mean over a scene's entries of |pos - pos_target|^2 at the nearest target time (:114-160)
    chamfer(a, b)                                 symmetric mean squared nearest-neighbour distance (pytorch3d.loss.chamfer_distance, :244)
    fit_sphere_radius(...)                        the gradient-descent loop (:210-270) for B (target, start) pairs; radius_error_table()
                                                  prints min / mean / max |r - r*| like RESULTS.md:14-47
trajectory fitting in shape space  (experiments/trajectory_fitting/optim_shapespace.py)
    bounce_world_latent(latents, packed, ...)     the same scene with a neural-SDF body in place of the sphere (:90-124)
    fit_trajectory_latent(...)                    the loop over the latent code
inertia fitting  (experiments/inertia_fitting/optim_shapespace.py)
    spin_world(latents, torque_dirs, net)         one neural-SDF body per scene, translation locked (X/Y/Z constraints), torque for
                                                  t < 0.3 (:71-92); inertia from the body's level-set mesh, differentiable w.r.t. the latent
    fit_inertia_latent(...)                       the loop of :136-250: loss = |v_T - v_T*|^2 + reg |latent|^2
inertia fitting of primitives  (experiments/inertia_fitting/optim_primitives.py)
    primitive_spin_world(kind, dims)              the same scene for an SDFBox / SDFSphere / SDFCylinder per row of dimensions (:95-115)
    fit_inertia_primitive(kind, ...)              the loop of :160-240 (Adam, dimensions clamped to [0.5, 2])

trajectory fitting to point clouds  (experiments/trajectory_fitting/optim_pointcloud.py)
    pointcloud_observations(world_target, cam)    the target body's camera-facing mesh vertices per frame (no renderer, no occlusion)
                                                  or, observe='depth', what a 640 x 480 depth camera sees of it past the wall and
                                                  the floor (depth_camera.py: ray-cast images, eroded segment, back-projection)
    pointcloud_frame_loss / pointcloud_trajectory_loss   match_pointcloud (:166-201) over observed frames: one dss_pointcloud_loss call
    fit_pointcloud(shape='sphere'|'cube', ...)    first-frame fit, then trajectory fit, of the half size and the start pose (:356-668)

trajectory fitting to recorded RGB-D sequences  (experiments/trajectory_fitting/optim_pointcloud_real.py)
    plane_pose(planes) / plane_world(rad, planes, fric, restitution, pose, vel, g, shape)   the fitted planes as pinned boxes and the
                                                  thrown ball or rounded cube (`make_world`, :98-148)
    run_world_frames(world, nframes, detach_2nd_bounce)   one entry per recorded frame (`run_world_fixed_dt`, :199-223)
    recorded_observations / recorded_trajectory_loss      the labelled points of every frame (recorded.py: csrc/cloud_select.hip) and
                                                  entry i against frame i (:170-196)
    fit_recorded(recordings, shape, ...)          first-frame fit, then trajectory fit over rad, start pose, start velocity, friction and
                                                  restitution (:326-557); synthesize_recording(...) makes recordings with the depth camera

system identification  (experiments/system_identification/optim_sysid.py)
    push_world(latents, packed, force, mass, fric, ...)   the floor and a neural-SDF body pushed along it (:104-131), per scene its own
                                                  push, mass and friction coefficient (torch tensors that may require grad)
    fit_sysid(goal, ...)                          the loop of :184-300 for goal in ('mass', 'force', 'friction')

    python -m diffsdfsim_amd.experiments sphere --scenes 64 --iters 100
    python -m diffsdfsim_amd.experiments shapespace --scenes 4 --iters 10
    python -m diffsdfsim_amd.experiments inertia --scenes 8 --iters 10
    python -m diffsdfsim_amd.experiments primitives --kind box --scenes 8 --iters 50
    python -m diffsdfsim_amd.experiments sysid --goal mass --scenes 8 --iters 20
    python -m diffsdfsim_amd.experiments pointcloud --shape sphere --scenes 8 --iters 20
    python -m diffsdfsim_amd.experiments pointcloud --shape igr --net bob_spot --scenes 2 --iters 10
    python -m diffsdfsim_amd.experiments pointcloud --shape grid --res 33 --scenes 2 --iters 100
    python -m diffsdfsim_amd.experiments recorded --file real_world_data.pkl [--shape cube]      (or --synthetic)
"""
import argparse
import math

import numpy as np
import torch

from . import chamfer as chamfer_hip
from . import mass_properties, meshes, meshsdf, scenes
from . import world_abi as abi
from .physics3d import BatchWorld3D
from .physics3d.utils import Defaults3D


# ---- rollouts ------------------------------------------------------------------------------------------------------------
def rollout(world, steps):
    """`steps` fixed outer steps of every scene -> poses [T,B,nb,7], velocities [T,B,nb,6] (autograd-connected)."""
    P, V = [], []
    for _ in range(steps):
        world.step()
        P.append(world.pose)
        V.append(world.vel)
    return torch.stack(P), torch.stack(V)


def run_world_fixed_dt(world, run_time, detach_2nd_bounce=False, max_steps=10000):
    """`run_world_fixed_dt` (optim_sphere.py:163-177) per scene of a batch.  Returns the trajectory as the reference's
    `world.trajectory` holds it, as a dict of t [K,B], pose [K,B,nb,7], vel [K,B,nb,6], valid [K,B]: ONE ENTRY PER ACCEPTED
    SUB-STEP (a step that halves dt or goes through a time-of-contact event adds several), stamped with the time at the START
    of the sub-step and holding the state after it (world.py:373-379: the entry is appended before `self.t += dt`); every entry
    keeps its graph.  An undone step (detach_2nd_bounce) leaves the list -- except its first entry: `undo_step` pops
    `while self.trajectory[-1][0] > self.t` (world.py:114-116) and that entry's stamp EQUALS self.t, so it stays, un-detached,
    as it does in the reference."""
    B, dev = world.B, world.device
    world.record_substeps = True
    num_contact = np.zeros(B, np.int64)
    T, P, V, OK = [], [], [], []
    for _ in range(max_steps):
        t = world.t
        mask = t < run_time
        if not mask.any():
            break
        had = np.asarray(world.step(mask=mask)) & mask
        sub, pose_end, vel_end = world.substeps, world.pose, world.vel
        redo = np.zeros(B, bool)
        if detach_2nd_bounce:
            num_contact += had
            redo = had & (num_contact > 1)
            if redo.any():
                world.undo_step(redo)
                world.detach_state(redo)
                num_contact[redo] = 0
        m_t = torch.as_tensor(mask, device=dev); r_t = torch.as_tensor(redo, device=dev)
        K = int(sub["pose"].shape[0])
        for k in range(K):           # the sub-steps inside this outer step
            T.append(sub["t"][k]); P.append(sub["pose"][k]); V.append(sub["vel"][k])
            OK.append(sub["valid"][k] & m_t & (~r_t if k > 0 else torch.ones_like(r_t)))
        # the last sub-step's entry = the state the step ended in; of an undone step it survives only if it is the step's FIRST entry
        first_is_last = ~sub["valid"][0] if K > 0 else torch.ones(B, dtype=torch.bool, device=dev)
        T.append(sub["last_t"]); P.append(pose_end); V.append(vel_end)
        OK.append(m_t & (~r_t | first_is_last))
    return dict(t=torch.stack(T), pose=torch.stack(P), vel=torch.stack(V), valid=torch.stack(OK))


def trajectory_loss(traj, target, body=-1):
    """optim_sphere.py:114-160: every entry of a scene's trajectory is compared with the target entry nearest in time (position
    of the last body); the sum over the scene's entries divided by their number.  Of two target entries equally near the LATER
    one is taken (`if diff <= min_diff`, :131).  -> [B]"""
    tw, tt = traj["t"], target["t"].to(traj["t"])
    diff = (tw[:, None, :] - tt[None, :, :]).abs()                                                             # [Kw, Kt, B]
    diff = torch.where(target["valid"].to(tw.device)[None, :, :], diff, torch.full_like(diff, float("inf")))
    Kt = diff.shape[1]
    j = Kt - 1 - diff.flip(1).argmin(dim=1)                                                                     # [Kw, B], last of the minima
    pos_t = target["pose"][:, :, body, 4:].to(traj["pose"])
    near = torch.gather(pos_t, 0, j[:, :, None].expand(-1, -1, 3))
    d = traj["pose"][:, :, body, 4:] - near
    w = traj["valid"].to(d.dtype)
    return ((d * d).sum(dim=2) * w).sum(dim=0) / w.sum(dim=0).clamp_min(1.0)


def chamfer(a, b):
    """pytorch3d.loss.chamfer_distance of two point sets a [Na,3], b [Nb,3] (defaults: squared distances, mean over the points of
    each set, the two directions summed)."""
    # on the device, a block of rows at a time: level-set meshes have 10^4 - 10^5 vertices
    dev = torch.device("cuda") if torch.cuda.is_available() and not a.is_cuda else a.device
    a, b = a.to(dev), b.to(dev)
    to_b = torch.full((b.shape[0],), float("inf"), dtype=a.dtype, device=dev)
    to_a = a.new_zeros(())
    for i in range(0, a.shape[0], 4096):
        d = torch.cdist(a[i:i + 4096], b) ** 2
        to_a = to_a + d.min(dim=1).values.sum()
        to_b = torch.minimum(to_b, d.min(dim=0).values)
    return to_a / a.shape[0] + to_b.mean()


def _chamfer_series(verts, target_cloud):
    """The report's `chamfer_dist` of one iteration, [B] numpy: the fitted bodies' mesh vertices (a list of [N_s,3] arrays or
    tensors) against the targets', packed once by chamfer.pack; one batched call (csrc/chamfer.hip), one read-back."""
    with torch.no_grad():
        a, a_off = chamfer_hip.pack(verts, target_cloud[0].device)
        return chamfer_hip.chamfer_packed(a, a_off, *target_cloud).cpu().numpy()


# ---- trajectory fitting: a sphere thrown at a wall (optim_sphere.py) --------------------------------------------------------
def bounce_world(radii, use_toc_diff=True, use_friction=True, use_wall=True, use_floor=True, use_gravity=True,
                 sphere_pos=(0.0, 5.0, 0.0), sphere_vel=(5.0, 0.0, 0.0), run_time=1.5, dt=Defaults3D.DT, device=None,
                 shape="sphere", corner_r=0.2, init_pose=None, res=128):
    """optim_sphere.py:77-111 for one scene per radius: floor 20 x 1 x 20, wall [5,5,0] 1 x 10 x 10 (both pinned, no contact
    with each other), a sphere of the scene's radius at (0,5,0) thrown with (5,0,0); restitution 0.5, friction 0.25 (0 without).
    Analytic meshes and inertias (the reference's custom_mesh / custom_inertia); shape and inertia are functions of `radii`.
    shape='cube' (optim_pointcloud.py:152-155): an SDFBoxRounded of dims 2 rad (1,1,1) and corner radius `corner_r` in the
    sphere's place, with its level-set mesh (marching cubes at `res`) and that mesh's inertia, both functions of `radii`.
    init_pose [B,7] (quaternion wxyz + position; a tensor that may require grad): the thrown body's start pose, in place of
    the identity rotation at `sphere_pos`; the world's `pose` is then connected to it."""
    rad = np.asarray(radii.detach().cpu() if torch.is_tensor(radii) else radii, np.float64).reshape(-1)
    B = len(rad)
    fixed = [n for n, on in (("floor", use_floor), ("wall", use_wall)) if on]
    nb = len(fixed) + 1
    mu = 0.25 if use_friction else 0.0
    spec, cache = scenes._base(B, nb), {}
    spec["Je"] = np.zeros((B, 6 * len(fixed), 6 * nb))
    nocon = np.zeros((nb, nb), np.uint8)
    for k, name in enumerate(fixed):
        dims, pos = ((20.0, 1.0, 20.0), (0.0, -0.5, 0.0)) if name == "floor" else ((1.0, 10.0, 10.0), (5.0, 5.0, 0.0))

        def make(dims=dims):
            v, f, tie = meshes.box_mesh(np.asarray(dims))
            return v, f, 0.5 * tie
        spec["mesh_id"][:, k] = scenes._add_mesh(spec, cache, ("box",) + tuple(dims), make)
        spec["pose"][:, k, 4:] = pos
        spec["shape_prm"][:, k] = dims
        spec["inertia"][:, k] = scenes.box_inertia(1.0, np.asarray(dims))
        spec["fric"][:, k] = mu
        spec["restitution"][:, k] = Defaults3D.RESTITUTION
        spec["Je"][:, 6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.eye(6)
    if len(fixed) == 2:
        nocon[0, 1] = nocon[1, 0] = 1
    spec["no_contact"] = nocon
    s_ = nb - 1
    if shape == "cube":
        return _bounce_world_cube(spec, radii, rad, s_, mu, corner_r, init_pose, sphere_pos, sphere_vel, use_gravity, use_toc_diff,
                                  run_time, dt, res, device)
    uv, uf = meshes.icosphere(4)
    for s in range(B):
        spec["mesh_id"][s, s_] = scenes._add_mesh(spec, cache, ("sphere", float(rad[s])), lambda r=float(rad[s]): (uv * r, uf, uv.copy()))
    spec["shape_type"][:, s_] = abi.SHAPE_SPHERE
    spec["shape_prm"][:, s_, 0] = rad
    spec["pose"][:, s_, 4:] = sphere_pos
    if init_pose is not None:
        spec["pose"][:, s_] = init_pose.detach().cpu().numpy()
    spec["vel"][:, s_, 3:] = sphere_vel
    spec["inertia"][:, s_] = 0.4 * rad[:, None, None] ** 2 * np.eye(3)
    spec["fric"][:, s_] = mu
    spec["restitution"][:, s_] = Defaults3D.RESTITUTION
    if use_gravity:
        spec["fext"][:, s_, 4] = -10.0
    params = {}
    if torch.is_tensor(radii) and radii.requires_grad:
        r = radii.to(torch.float64).reshape(-1)
        prm = torch.tensor(spec["shape_prm"], dtype=torch.float64)
        prm = torch.cat([prm[:, :s_], torch.stack([r, torch.zeros_like(r), torch.zeros_like(r)], 1)[:, None].to(prm)], 1)
        inertia = torch.tensor(spec["inertia"], dtype=torch.float64)
        ball = (0.4 * r * r)[:, None, None].to(inertia) * torch.eye(3, dtype=torch.float64)      # 2/5 m r^2 (bodies.py:993-994)
        params = dict(shape_prm=prm, inertia=torch.cat([inertia[:, :s_], ball[:, None]], 1))
    steps = int(math.ceil(run_time / dt)) + 2
    w = BatchWorld3D(spec, params=params, dt=dt, time_of_contact_diff=use_toc_diff, max_substeps=8 * steps + 64, device=device)
    if init_pose is not None:
        _connect_start_pose(w, s_, init_pose)
    w.body_meshes = [(uv * float(x), uf) for x in rad]      # the thrown body's mesh per scene (pointcloud_observations)
    return w


def _connect_start_pose(w, body, init_pose):
    """The world's state tensor with `body`'s row taken from init_pose [B,7] (values already in the engine): the first step's
    adjoint of the pose then reaches init_pose."""
    w.pose = torch.cat([w.pose[:, :body], init_pose.to(w.pose)[:, None], w.pose[:, body + 1:]], 1)


def _bounce_world_cube(spec, radii, rad, s_, mu, corner_r, init_pose, pos, vel, use_gravity, use_toc_diff, run_time, dt, res, device):
    """bounce_world's scene with the rounded cube of optim_pointcloud.py:152-155: level-set mesh and mesh inertia per scene,
    differentiable w.r.t. the half side `radii` as bounce_world_latent's body is w.r.t. its latent code."""
    B, nb = spec["pose"].shape[:2]
    r_t = radii.to(torch.float64).reshape(-1).cpu() if torch.is_tensor(radii) else torch.tensor(rad)
    spec["shape_aux"] = np.zeros((B, nb))
    spec["shape_aux"][:, s_] = corner_r
    spec["shape_type"][:, s_] = abi.SHAPE_BOX_ROUNDED
    spec["shape_prm"][:, s_] = 2.0 * rad[:, None]
    one = torch.tensor(1.0, dtype=torch.float64)
    vts, Is, body_meshes = [torch.as_tensor(m[0], dtype=torch.float64) for m in spec["meshes"]], [], []
    for s in range(B):
        scale = 1.5 * r_t[s]                                              # max(dims) * 1.5 / 2
        unit = torch.stack([2.0 * r_t[s], 2.0 * r_t[s], 2.0 * r_t[s], torch.tensor(corner_r, dtype=torch.float64)]) / scale
        v, f = meshsdf.primitive_mesh(abi.SHAPE_BOX_ROUNDED, unit, res=res)
        v = v * scale.to(v.device)
        Is.append(mass_properties.mesh_inertia_diff(v, f, one).cpu())
        spec["meshes"].append((v.detach().cpu().numpy(), f.cpu().numpy())); spec["mesh_vgrad"].append(np.zeros((v.shape[0], 3)))
        spec["mesh_id"][s, s_] = len(spec["meshes"]) - 1
        body_meshes.append(spec["meshes"][-1])
        vts.append(v)
    spec["pose"][:, s_, 4:] = pos
    if init_pose is not None:
        spec["pose"][:, s_] = init_pose.detach().cpu().numpy()
    spec["vel"][:, s_, 3:] = vel
    spec["inertia"][:, s_] = torch.stack(Is).detach().numpy()
    spec["fric"][:, s_] = mu
    spec["restitution"][:, s_] = Defaults3D.RESTITUTION
    if use_gravity:
        spec["fext"][:, s_, 4] = -10.0
    params = {}
    if r_t.requires_grad:
        prm = torch.tensor(spec["shape_prm"], dtype=torch.float64)
        inertia = torch.tensor(spec["inertia"], dtype=torch.float64)
        dev = vts[-1].device
        params = dict(shape_prm=torch.cat([prm[:, :s_], (2.0 * r_t)[:, None, None].expand(B, 1, 3)], 1),
                      inertia=torch.cat([inertia[:, :s_], torch.stack(Is)[:, None]], 1), verts=torch.cat([v.to(dev) for v in vts]))
    steps = int(math.ceil(run_time / dt)) + 2
    # (a flat face of the level-set mesh landing on the floor makes every one of its ~10^4 vertices a contact candidate)
    w = BatchWorld3D(spec, params=params, dt=dt, time_of_contact_diff=use_toc_diff, max_substeps=8 * steps + 64, device=device,
                     maxc=256, max_cand=32768, max_pc=128)
    if init_pose is not None:
        _connect_start_pose(w, s_, init_pose)
    w.body_meshes = body_meshes
    return w


def fit_sphere_radius(target_radii, start_radii, run_time=1.5, max_iter=100, lr=0.1, conv_thresh=1e-5, min_dim=0.4, max_dim=2.0,
                      detach_2nd_bounce=True, log=None, **scene):
    """The loop of optim_sphere.py:210-270 for B scenes at once: plain gradient descent on the radius, a new world from the
    current estimate in every iteration, a scene stops when its loss changes by less than conv_thresh (its radius is frozen:
    the scenes of the batch are independent optimisations).  Returns dict(radius [B], history)."""
    target_radii = torch.as_tensor(np.asarray(target_radii, np.float64))
    with torch.no_grad():
        wt = bounce_world(target_radii, run_time=run_time, **scene)
        target = run_world_fixed_dt(wt, run_time)
        tgt_cloud = chamfer_hip.pack([m[0] for m in wt.body_meshes])
    rad = torch.tensor(np.asarray(start_radii, np.float64), requires_grad=True)
    B = rad.numel()
    done = np.zeros(B, bool)
    last = np.full(B, 1e10)
    hist = []
    for e in range(max_iter):
        if rad.grad is not None:
            rad.grad = None
        world = bounce_world(rad, run_time=run_time, **scene)
        traj = run_world_fixed_dt(world, run_time, detach_2nd_bounce=detach_2nd_bounce)
        loss = trajectory_loss(traj, target)
        loss.sum().backward()
        l = loss.detach().cpu().numpy()
        done |= np.abs(last - l) < conv_thresh
        d = _chamfer_series([m[0] for m in world.body_meshes], tgt_cloud)
        hist.append(dict(iter=e, loss=l.copy(), radius=rad.detach().numpy().copy(), grad=rad.grad.numpy().copy(), done=done.copy(), chamfer=d))
        if log:
            log("iter %3d  mean loss %.3e  mean chamfer %.3e  mean |r - r*| %.4f  converged %d / %d" %
                (e, float(l.mean()), float(d.mean()), float((rad.detach() - target_radii).abs().mean()), int(done.sum()), B))
        if done.all():
            break
        with torch.no_grad():
            step = lr * rad.grad
            step[torch.as_tensor(done)] = 0.0
            rad -= step
            rad.clamp_(min_dim, max_dim)
        last = l
    return dict(radius=rad.detach().numpy().copy(), target=target_radii.numpy(), history=hist)


def radius_error_table(results):
    """min / mean / max of |r - r*| per variant, the numbers of RESULTS.md:14-47."""
    rows = []
    for name, r in results.items():
        err = np.abs(r["radius"] - r["target"])
        rows.append("%-22s min %.1e  mean %.4f  max %.4f   (%d scenes)" % (name, err.min(), err.mean(), err.max(), len(err)))
    return "\n".join(rows)


# ---- trajectory fitting to point clouds (trajectory_fitting/optim_pointcloud.py) -------------------------------------------
def camera_pose():
    """The experiment's camera (optim_pointcloud.py:408-415): 20 back along z, then Ry(pi/4) Rx(-pi/4); 4 x 4, camera to world."""
    g = t = math.pi / 4
    Ry = np.array([[math.cos(g), 0, math.sin(g), 0], [0, 1, 0, 0], [-math.sin(g), 0, math.cos(g), 0], [0, 0, 0, 1.0]])
    Rx = np.array([[1, 0, 0, 0], [0, math.cos(-t), -math.sin(-t), 0], [0, math.sin(-t), math.cos(-t), 0], [0, 0, 0, 1.0]])
    T = np.eye(4); T[2, 3] = 20.0
    return Ry @ Rx @ T


def _vertex_normals(v, f):
    n = np.zeros_like(v)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


CAMERA = dict(fx=515.0, fy=515.0, cx=319.5, cy=239.5, size=(640, 480), znear=0.1, zfar=100.0)      # optim_pointcloud.py:86-89, 407


def _depth_observations(world_target, cam_pose, noise, every, run_time, seed, body, max_bytes):
    """pointcloud_observations(observe='depth'): the same frames and stamps, each seen by the depth camera."""
    from . import depth_camera
    B, E = world_target.B, world_target.engine
    world_target.record_substeps = True
    poses, times, scene = [], [], []

    def frame(pose, stamp, mask):
        idx = np.nonzero(mask)[0]
        poses.append(pose[torch.as_tensor(idx, device=pose.device)])
        times.extend(float(stamp[s]) for s in idx); scene.extend(int(s) for s in idx)
    with torch.no_grad():
        frame(world_target.pose.detach(), np.full(B, -world_target.dt), np.ones(B, bool))
        k = 0
        while True:
            mask = world_target.t < run_time
            if not mask.any():
                break
            world_target.step(mask=mask, keep_undo=False)
            k += 1
            if k % every == 0:
                frame(world_target.pose.detach(), world_target.substeps["last_t"].cpu().numpy(), mask)
        sc = torch.as_tensor(np.asarray(scene, np.int64), device=world_target.device)
        aux = E.arr["shape_aux"] if "shape_aux" in E.arr else torch.zeros_like(E.arr["shape_prm"][..., 0])
        prm = torch.cat([E.arr["shape_prm"], aux[..., None]], 2)[sc]
        grid_kw = {}
        if "grid_data" in E.arr:      # the world's spec carries voxel grids: the camera sees those bodies through them
            from .grids import GridTable
            grid_kw = dict(grids=GridTable.from_pooled(E.arr["grid_dims"], E.arr["grid_data"]), grid_id=E.arr["grid_id"][sc])
        pts, off = depth_camera.observe(torch.cat(poses), E.arr["shape_type"][sc], prm, body % world_target.nb, cam_pose, noise=noise,
                                        seed=seed, max_bytes=max_bytes, **grid_kw, **CAMERA)
    return dict(pts=pts, seg_off=off, time=np.asarray(times), scene=np.asarray(scene, np.int64))


def pointcloud_observations(world_target, cam_pose, noise=0.0, every=1, run_time=1.5, seed=0, body=-1, observe="vertices",
                            max_bytes=256 << 20):
    """What the experiment's depth camera records of the target body (Recorder3D with record_points, optim_pointcloud.py:420-423),
    without a renderer: `world_target` (a fresh bounce_world with `body_meshes`) is stepped to run_time and, for the start
    state and after every `every`-th outer step, the body's mesh vertices that face the camera -- normal . (vertex - camera) < 0,
    exact for the two convex shapes of the experiment -- are taken as the observed points of that frame, in the world frame.
    OCCLUSION BY THE WALL AND THE FLOOR IS IGNORED AND NOTHING IS RASTERISED: every camera-facing vertex is seen.
    noise: the reference's depth_noise_factor -- a point at depth d along the optical axis is moved along its ray by
    N(0, (noise d^2)^2).  Returns dict(pts [N,3] on the world's device, seg_off [nseg+1], time [nseg], scene [nseg]); segment 0..B-1
    are the start states (time -dt: no trajectory entry carries that stamp), the others are stamped like run_world_fixed_dt's
    entries, with the time at the start of the (last sub-step of the) outer step whose end state they show.
    observe='depth': the frames are instead rendered by the experiment's depth camera (CAMERA: 640 x 480, fx = fy = 515) with ALL
    the world's bodies, so the wall and the floor hide what they hide; the body's segment is eroded by one pixel and back-projected
    as match_pointcloud does (depth_camera.observe, at most max_bytes of images at a time; noise: depth += N(0, (noise depth^2)^2) per
    pixel, from a device generator seeded with `seed`).  Same dict, same stamps.  Boxes, spheres, cylinders and rounded boxes only."""
    if observe == "depth":
        return _depth_observations(world_target, cam_pose, noise, every, run_time, seed, body, max_bytes)
    if observe != "vertices":
        raise ValueError("observe: 'vertices' or 'depth', got %r" % (observe,))
    B = world_target.B
    cam = np.asarray(cam_pose, np.float64)
    c, axis = cam[:3, 3], -cam[:3, 2]                       # OpenGL convention: the camera looks along its -z
    rng = np.random.default_rng(seed)
    world_target.record_substeps = True
    normals = [_vertex_normals(np.asarray(v, np.float64), np.asarray(f)) for v, f in world_target.body_meshes]
    pts, off, times, scene = [], [0], [], []

    def frame(pose, stamp, mask):
        for s in range(B):
            if not mask[s]:
                continue
            v = np.asarray(world_target.body_meshes[s][0], np.float64)
            r_, i, j, k = pose[s, :4]
            ts = 2.0 / (pose[s, :4] ** 2).sum()
            R = np.array([[1 - ts * (j * j + k * k), ts * (i * j - k * r_), ts * (i * k + j * r_)], [ts * (i * j + k * r_), 1 - ts * (i * i + k * k), ts * (j * k - i * r_)],
                          [ts * (i * k - j * r_), ts * (j * k + i * r_), 1 - ts * (i * i + j * j)]])
            x = v @ R.T + pose[s, 4:]
            seen = x[((normals[s] @ R.T) * (x - c)).sum(1) < 0]
            if noise > 0:
                ray = seen - c
                d = ray @ axis
                seen = c + ray * (1.0 + rng.standard_normal(len(seen)) * noise * d)[:, None]      # (d + N(0, noise d^2)) / d
            pts.append(seen); off.append(off[-1] + len(seen)); times.append(float(stamp[s])); scene.append(s)
    with torch.no_grad():
        frame(world_target.pose[:, body].cpu().numpy(), np.full(B, -world_target.dt), np.ones(B, bool))
        k = 0
        while True:
            mask = world_target.t < run_time
            if not mask.any():
                break
            world_target.step(mask=mask, keep_undo=False)
            k += 1
            if k % every == 0:
                frame(world_target.pose[:, body].cpu().numpy(), world_target.substeps["last_t"].cpu().numpy(), mask)
    return dict(pts=torch.as_tensor(np.concatenate(pts)).to(world_target.device), seg_off=np.asarray(off, np.int64),
                time=np.asarray(times), scene=np.asarray(scene, np.int64))


def _cloud_prm(shape, rad, corner_r):
    """Shape type and parameter rows [B,4] of the estimate: sphere (rad, 0, 0, 0), cube (2 rad, 2 rad, 2 rad, corner_r)."""
    z = torch.zeros_like(rad)
    if shape == "sphere":
        return abi.SHAPE_SPHERE, torch.stack([rad, z, z, z], 1)
    return abi.SHAPE_BOX_ROUNDED, torch.stack([2 * rad, 2 * rad, 2 * rad, z + corner_r], 1)


def pointcloud_frame_loss(obs, segs, pose, rad, shape, corner_r=0.2, match=None, packed=None, latent=None, scale=1.0):
    """sum / max(1, count) per scene of the point-cloud loss over the segments `segs` of `obs`, segment i seen from the pose
    pose[i] [7] of scene obs['scene'][segs[i]] with half size rad[scene] (optim_pointcloud.py:198-201, 284-285).  -> [B] on the
    device.  match: the loss of the segments (default pointcloud.match_pointcloud, the HIP kernel).
    shape='igr': a neural estimate -- `packed` (pack_weights), `latent` [B, L] (one code per scene, differentiable) and `scale`;
    `rad` is not read."""
    from . import pointcloud
    match = match or pointcloud.match_pointcloud
    dev = obs["pts"].device
    sc = torch.as_tensor(obs["scene"][segs], device=dev)
    off = obs["seg_off"]
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in segs]) if len(segs) else np.zeros(0, np.int64)
    loc = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in segs])]).astype(np.int64)
    if shape == "igr":
        if packed is None or latent is None:
            raise ValueError("shape='igr' needs packed= and latent= [B, L]")
        B = latent.shape[0]
        prm = torch.zeros(len(segs), 4, dtype=torch.float64, device=dev)
        prm[:, 3] = scale
        s, n = match(obs["pts"][torch.as_tensor(idx, device=dev)], loc, pose.to(dev), torch.full((len(segs),), abi.SHAPE_IGR, dtype=torch.int32),
                     prm, igr=packed, latent=latent.to(dev), latent_id=sc)
    else:
        B = rad.numel()
        kind, prm = _cloud_prm(shape, rad.to(dev), corner_r)
        s, n = match(obs["pts"][torch.as_tensor(idx, device=dev)], loc, pose.to(dev), torch.full((len(segs),), kind, dtype=torch.int32), prm[sc])
    tot = torch.zeros(B, dtype=torch.float64, device=dev).index_add(0, sc, s)
    cnt = torch.zeros(B, dtype=torch.float64, device=dev).index_add(0, sc, n.to(torch.float64))
    return tot / cnt.clamp_min(1.0)


def pointcloud_trajectory_loss(traj, obs, rad, shape, corner_r=0.2, body=-1, match=None, packed=None, latent=None, scale=1.0):
    """trajectory_loss of optim_pointcloud.py:204-290, its point-cloud part: every valid trajectory entry whose stamp is within
    1e-5 of an observation's time is compared with that observation's points; per scene sum / max(1, count).  -> [B]"""
    t, ok = traj["t"].cpu().numpy(), traj["valid"].cpu().numpy()
    segs, ent = [], []
    for i in range(len(obs["time"])):
        s = obs["scene"][i]
        hit = np.nonzero(ok[:, s] & (np.abs(t[:, s] - obs["time"][i]) <= 1e-5))[0]
        for k in hit:
            segs.append(i); ent.append((k, s))
    dev = traj["pose"].device
    ent = np.asarray(ent, np.int64).reshape(-1, 2)
    pose = traj["pose"][torch.as_tensor(ent[:, 0], device=dev), torch.as_tensor(ent[:, 1], device=dev), body]
    return pointcloud_frame_loss(obs, np.asarray(segs, np.int64), pose, rad, shape, corner_r, match, packed, latent, scale)


def fit_pointcloud(shape="sphere", target_rad=(1.0,), start_rad=(1.3,), target_pose=None, start_pose=None, run_time=1.5, max_iter=200,
                   lr=0.1, optimizer="GD", conv_thresh=1e-5, conv_thresh_shape=1e-3, min_dim=0.5, max_dim=2.5, noise=0.0, every=1,
                   detach_2nd_bounce=True, fit_first_frame=True, fit_trajectory=True, optimize_pose=True, corner_r=0.2, seed=0,
                   log=None, observe="vertices", **scene):
    """optim_pointcloud.py:356-668 for B scenes at once, shape 'sphere' (SDFSphere of radius rad) or 'cube' (SDFBoxRounded of
    dims 2 rad (1,1,1), r = 0.2).  The target's points come from pointcloud_observations (observe: 'vertices', its camera-facing mesh
    vertices, or 'depth', what the depth camera sees of it past the wall and the floor); the estimate's half
    size `rad` [B] and, with optimize_pose, its start pose [B,7] are fitted in two stages with the same variables:
      first frame   the loss of observation 0 seen from the start pose (:428-522),
      trajectory    the scene rolled out with run_world_fixed_dt(..., detach_2nd_bounce) and compared at the observed frames
                    (pointcloud_trajectory_loss; :545-633).
    GD or Adam; after a step rad is clamped to [min_dim, max_dim] and the quaternion renormalised; a scene whose loss moved by
    less than conv_thresh and its rad by less than conv_thresh_shape is frozen (the scenes are independent optimisations).
    Returns dict(rad, pose, target_rad, target_pose, history: {'frame': [...], 'trajectory': [...]})."""
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    target_rad = T(target_rad).reshape(-1)
    B = target_rad.numel()
    ident = torch.tensor([1.0, 0, 0, 0, 0.0, 5.0, 0.0], dtype=torch.float64).repeat(B, 1)
    target_pose = ident.clone() if target_pose is None else T(target_pose).reshape(B, 7)
    with torch.no_grad():
        wt = bounce_world(target_rad, run_time=run_time, shape=shape, corner_r=corner_r, init_pose=target_pose, **scene)
        tgt_cloud = chamfer_hip.pack([m[0] for m in wt.body_meshes])
        obs = pointcloud_observations(wt, camera_pose(), noise=noise, every=every, run_time=run_time, seed=seed, observe=observe)
    rad = T(start_rad).reshape(-1).clone().requires_grad_()
    start_pose = target_pose.clone() if start_pose is None else T(start_pose).reshape(B, 7)
    rot, pos = start_pose[:, :4].clone().requires_grad_(optimize_pose), start_pose[:, 4:].clone().requires_grad_(optimize_pose)
    var = [rad] + ([rot, pos] if optimize_pose else [])
    first = np.nonzero(obs["time"] < 0)[0]
    hist = {}
    for stage in [n for n, on in (("frame", fit_first_frame), ("trajectory", fit_trajectory)) if on]:
        opt = torch.optim.Adam(var, lr=lr) if optimizer == "Adam" else torch.optim.SGD(var, lr=lr)
        done, last, last_rad, h = np.zeros(B, bool), np.full(B, 1e10), np.full(B, 1e10), []
        for e in range(max_iter):
            opt.zero_grad()
            pose0 = torch.cat([rot, pos], 1)
            if stage == "frame":
                loss = pointcloud_frame_loss(obs, first, pose0[obs["scene"][first]], rad, shape, corner_r)
            else:
                world = bounce_world(rad, run_time=run_time, shape=shape, corner_r=corner_r, init_pose=pose0, **scene)
                traj = run_world_fixed_dt(world, run_time, detach_2nd_bounce=detach_2nd_bounce)
                loss = pointcloud_trajectory_loss(traj, obs, rad, shape, corner_r)
            loss.sum().backward()
            l, r_now = loss.detach().cpu().numpy(), rad.detach().numpy().copy()
            done |= (np.abs(last - l) < conv_thresh) & (np.abs(last_rad - r_now) < conv_thresh_shape)
            h.append(dict(iter=e, loss=l.copy(), rad=r_now, pose=pose0.detach().numpy().copy(), grad_rad=rad.grad.numpy().copy(), done=done.copy()))
            cd = ""
            if stage == "trajectory":      # (the first-frame stage builds no world, so it has no mesh of the estimate at hand)
                h[-1]["chamfer"] = _chamfer_series([m[0] for m in world.body_meshes], tgt_cloud)
                cd = "  mean chamfer %.3e" % float(h[-1]["chamfer"].mean())
            if log:
                log("[%s] iter %3d  mean loss %.3e%s  mean |rad - rad*| %.4f  mean |pos - pos*| %.4f  converged %d / %d" %
                    (stage, e, float(l.mean()), cd, float(np.abs(r_now - target_rad.numpy()).mean()),
                     float((pos.detach() - target_pose[:, 4:]).norm(dim=1).mean()), int(done.sum()), B))
            if done.all():
                break
            frozen = torch.as_tensor(done)
            for v in var:
                v.grad[frozen] = 0.0
            keep = [v.detach().clone() for v in var]
            opt.step()
            with torch.no_grad():
                for v, k in zip(var, keep):      # (Adam's momentum would still move a frozen scene)
                    v[frozen] = k[frozen]
                rad.clamp_(min_dim, max_dim)
                if optimize_pose:
                    rot /= rot.norm(dim=1, keepdim=True)
            last, last_rad = l, r_now
        hist[stage] = h
    return dict(rad=rad.detach().numpy().copy(), pose=torch.cat([rot, pos], 1).detach().numpy().copy(), target_rad=target_rad.numpy(),
                target_pose=target_pose.numpy(), history=hist, observations=obs)


# ---- a voxel body fitted to what the camera sees (no counterpart in the reference: its grid samples carry no gradient) -----------
def orbit_camera_poses(extra=2):
    """The experiment's camera and `extra` more, turned about the world's vertical axis in equal steps (the body stands on that
    axis, so each of them sees it from another side at the same distance and height)."""
    out = []
    for k in range(extra + 1):
        a = 2.0 * math.pi * k / (extra + 1)
        Ry = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1.0]])
        out.append(Ry @ camera_pose())
    return out


def _pose_points(v, pose):
    """Body-frame points v [N,3] (numpy) in the world frame of pose [7] (raw quaternion normalised by 2 / (q.q))."""
    r_, i, j, k = pose[:4]
    ts = 2.0 / (pose[:4] ** 2).sum()
    R = np.array([[1 - ts * (j * j + k * k), ts * (i * j - k * r_), ts * (i * k + j * r_)], [ts * (i * j + k * r_), 1 - ts * (i * i + k * k), ts * (j * k - i * r_)],
                  [ts * (i * k - j * r_), ts * (j * k + i * r_), 1 - ts * (i * i + j * j)]])
    return np.asarray(v, np.float64) @ R.T + pose[4:]


def eikonal_residual(sdf):
    """mean (|grad s| - 1)^2 of unit-frame samples sdf [B,n0,n1,n2] (over [-1,1]^3), per grid: forward differences over the
    cells' edges, each cell's gradient taken at its low corner.  Plain torch; differentiable."""
    h = [2.0 / (n - 1) for n in sdf.shape[1:]]
    gx = (sdf[:, 1:, :-1, :-1] - sdf[:, :-1, :-1, :-1]) / h[0]
    gy = (sdf[:, :-1, 1:, :-1] - sdf[:, :-1, :-1, :-1]) / h[1]
    gz = (sdf[:, :-1, :-1, 1:] - sdf[:, :-1, :-1, :-1]) / h[2]
    return ((torch.sqrt(gx * gx + gy * gy + gz * gz + 1e-12) - 1.0) ** 2).mean(dim=(1, 2, 3))


def fit_pointcloud_grid(shape="sphere", target_rad=(1.0,), start_rad=(1.3,), target_pose=None, start_pose=None, res=17, scale=None,
                        max_iter=100, lr=0.02, eik_reg=1e-2, optimize_pose=False, extra_cameras=2, noise=0.0, max_points=None, corner_r=0.2,
                        seed=0, log=None, observe="vertices", mesh_res=128, target_mesh=None, **scene):
    """The first-frame stage of fit_pointcloud for a voxel body (SDFGrid3D's field: res^3 samples over the cube of half side
    `scale`, default 1.5 max(target_rad)).  B scenes; scene s has a target sphere or rounded cube of half size target_rad[s] at
    target_pose[s].  Observations: pointcloud_observations of the start frame (either `observe` mode) from the experiment's camera
    and `extra_cameras` more around the vertical axis (orbit_camera_poses), at most max_points of each view (a seeded choice);
    mesh_res: the resolution of a target cube's level-set mesh (bounce_world's `res`).
    The grids start as the samples of a sphere of radius start_rad[s]; Adam moves the samples (and, with optimize_pose, the pose)
    down   loss[s] = sum phi^2 / max(1, count) over the scene's views  +  eik_reg * eikonal_residual(samples)[s]
    where the first term is match_pointcloud on the grids (its gradient w.r.t. the samples: dss_pointcloud_loss_grids_adjoint).
    The regulariser is needed: sum phi^2 alone is also least for samples that are all zero.
    There is no trajectory stage -- the stepper has no adjoint for a grid's samples.
    target_mesh=(verts, faces): the target is instead a closed triangle mesh of the user's (meshes.load_obj), the same in every
    scene: it is voxelised by SDFGrid3D.from_mesh (65^3 samples, centroid at the target pose's position) and the level-set mesh of
    that body stands where the sphere's did -- its camera-facing vertices are the observations (observe='vertices' only, which
    is exact for convex meshes), its vertices the chamfer distance's target; target_rad is then the mesh's largest |coordinate|.
    Returns dict(sdf [B,res,res,res] unit-frame samples, pose, scale, history [dict(iter, loss, data)], loss_start, loss_final,
    chamfer_start, chamfer_final [B]: chamfer distance (chamfer.py) between the marching-cubes mesh of the grid, in the world frame of
    the estimate's pose, and the target's mesh in its own; observations)."""
    from . import meshsdf, pointcloud
    from .grids import GridTable
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    target_rad, start_rad = T(target_rad).reshape(-1), T(start_rad).reshape(-1)
    if target_mesh is not None:
        if observe != "vertices":
            raise ValueError("target_mesh: observe='vertices' (the depth camera of this driver sees primitives only)")
        from .physics3d.bodies import SDFGrid3D
        mesh_body = SDFGrid3D.from_mesh((0.0, 0.0, 0.0), *target_mesh, res=65)
        target_rad = torch.full_like(start_rad, float(np.abs(mesh_body.verts_np).max()))
    B = target_rad.numel()
    scale = float(1.5 * target_rad.max()) if scale is None else float(scale)
    ident = torch.tensor([1.0, 0, 0, 0, 0.0, 5.0, 0.0], dtype=torch.float64).repeat(B, 1)
    target_pose = ident.clone() if target_pose is None else T(target_pose).reshape(B, 7)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        wt = bounce_world(target_rad, run_time=0.0, shape=shape, corner_r=corner_r, init_pose=target_pose, res=mesh_res, **scene)
        dev = wt.device
        if target_mesh is not None:      # (run_time 0: the world is never stepped, only its thrown body's mesh and pose are read)
            wt.body_meshes = [(mesh_body.verts_np, mesh_body.faces_np)] * B
        tgt_cloud = chamfer_hip.pack([_pose_points(m[0], target_pose[s].numpy()) for s, m in enumerate(wt.body_meshes)], dev)
        pts, off, scene_of = [], [0], []
        for cam in orbit_camera_poses(extra_cameras):      # run_time 0: the start frame alone, one segment per scene and view
            o = pointcloud_observations(wt, cam, noise=noise, run_time=0.0, seed=seed, observe=observe)
            so = np.asarray(o["seg_off"].cpu() if torch.is_tensor(o["seg_off"]) else o["seg_off"], np.int64)
            for i in range(len(so) - 1):
                idx = np.arange(so[i], so[i + 1])
                if max_points is not None and len(idx) > max_points:
                    idx = np.sort(rng.choice(idx, max_points, replace=False))
                pts.append(o["pts"][torch.as_tensor(idx, device=o["pts"].device)].to(dev)); off.append(off[-1] + len(idx)); scene_of.append(int(o["scene"][i]))
    obs = dict(pts=torch.cat(pts), seg_off=np.asarray(off, np.int64), scene=np.asarray(scene_of, np.int64))
    sc = torch.as_tensor(obs["scene"], device=dev)
    g = torch.linspace(-1.0, 1.0, res, dtype=torch.float64)
    norm = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), 3).norm(dim=3)
    sdf = (norm[None] - (start_rad / scale)[:, None, None, None]).to(dev).requires_grad_()
    start_pose = target_pose.clone() if start_pose is None else T(start_pose).reshape(B, 7)
    rot, pos = start_pose[:, :4].clone().requires_grad_(optimize_pose), start_pose[:, 4:].clone().requires_grad_(optimize_pose)
    opt = torch.optim.Adam([sdf] + ([rot, pos] if optimize_pose else []), lr=lr)
    types = torch.full((len(scene_of),), abi.SHAPE_GRID, dtype=torch.int32)
    prm = torch.zeros(len(scene_of), 4, dtype=torch.float64, device=dev)
    prm[:, 3] = scale

    def losses():
        pose0 = torch.cat([rot, pos], 1).to(dev)
        s, n = pointcloud.match_pointcloud(obs["pts"], obs["seg_off"], pose0[sc], types, prm, grids=GridTable(list(sdf), dev), grid_id=sc)
        tot = torch.zeros(B, dtype=torch.float64, device=dev).index_add(0, sc, s)
        cnt = torch.zeros(B, dtype=torch.float64, device=dev).index_add(0, sc, n)
        data = tot / cnt.clamp_min(1.0)
        return data + eik_reg * eikonal_residual(sdf), data

    def chamfer_now():
        with torch.no_grad():
            pose0 = torch.cat([rot, pos], 1).detach().numpy()
            verts = []
            for s in range(B):
                v, _ = meshsdf.marching_cubes(sdf[s].detach(), 0.0)
                verts.append(_pose_points((v.cpu().numpy() / (res - 1) * 2.0 - 1.0) * scale, pose0[s]))
            return _chamfer_series(verts, tgt_cloud)

    chamfer_start, hist = chamfer_now(), []
    for e in range(max_iter + 1):      # (the last pass only evaluates)
        opt.zero_grad()
        loss, data = losses()
        hist.append(dict(iter=e, loss=loss.detach().cpu().numpy().copy(), data=data.detach().cpu().numpy().copy()))
        if log:
            log("[grid] iter %3d  mean loss %.3e  (points %.3e)" % (e, float(hist[-1]["loss"].mean()), float(hist[-1]["data"].mean())))
        if e == max_iter:
            break
        loss.sum().backward()
        opt.step()
        if optimize_pose:
            with torch.no_grad():
                rot /= rot.norm(dim=1, keepdim=True)
    return dict(sdf=sdf.detach().cpu().numpy().copy(), pose=torch.cat([rot, pos], 1).detach().numpy().copy(), scale=scale, history=hist,
                loss_start=hist[0]["loss"], loss_final=hist[-1]["loss"], chamfer_start=chamfer_start, chamfer_final=chamfer_now(),
                target_rad=target_rad.numpy(), target_pose=target_pose.numpy(), observations=obs)


# ---- fitting to depth images through the differentiable depth camera (depth_camera.render_depth_diff) ---------------------------
def depth_residual_loss(depth, seg, obs_depth, obs_seg, body):
    """The mean squared depth difference over the pixels where both images show body index `body`, per view: [nview] (0 for a view
    without such a pixel).  depth, seg: a render of the estimate (render_depth_diff: the graph runs through `depth`); obs_depth,
    obs_seg: the observation.  The residual acts on the surface the estimate presents to the camera; where only one of the two
    images shows the body nothing pulls (the camera's derivative does not model silhouettes)."""
    both = ((seg == body) & (obs_seg == body)).to(depth.dtype)
    return (both * (depth - obs_depth.detach()) ** 2).sum(dim=(1, 2)) / both.sum(dim=(1, 2)).clamp_min(1.0)


def _sample_sdf(shape, rad, corner_r, res, scale):
    """Unit-frame samples [res]^3 of a sphere of radius rad or a rounded cube of half size rad over the cube of half side scale."""
    g = torch.linspace(-1.0, 1.0, res, dtype=torch.float64) * scale
    p = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), 3)
    if shape == "sphere":
        return (p.norm(dim=3) - rad) / scale
    q = p.abs() - (rad - corner_r)
    return (q.clamp_min(0.0).norm(dim=3) + q.max(dim=3).values.clamp_max(0.0) - corner_r) / scale


def fit_depth(shape="sphere", target_rad=(1.0,), start_rad=(1.3,), target_pose=None, start_pose=None, res=17, scale=None, max_iter=100,
              lr=None, optimizer="Adam", eik_reg=1e-2, extra_cameras=2, size=(80, 60), corner_r=0.2, mesh_res=33, min_cos=1e-3, log=None,
              target_latents=None, start_latents=None, packed=None, latent_reg=1e-4):
    """A first-frame fit to depth images, the counterpart of the first stage of fit_pointcloud / fit_pointcloud_grid with a residual
    between a rendered and an observed depth image in place of the point-cloud loss.  B scenes at once; scene s shows the
    experiment's floor and wall and a target sphere (or rounded cube, shape="cube") of half size target_rad[s] at target_pose[s],
    seen by the experiment's camera and `extra_cameras` more (orbit_camera_poses) at `size` pixels with the experiment's field of
    view.  One view per (scene, camera).
    shape "sphere" / "cube": the pose and the half size are fitted from start_pose / start_rad.  shape "grid": a voxel body of
    res^3 samples over the cube of half side `scale` (default 1.5 max target_rad) at the target's pose, started as a sphere of
    radius start_rad[s]; the samples are fitted (to a target sphere), with eik_reg * eikonal_residual as in fit_pointcloud_grid.
    shape "igr": the thrown body is a neural body of the network `packed` (igr.pack_weights) and of size `scale` (default 2) at the
    target's pose, seen through its value grid of res^3 samples (depth_camera.body_grid); the observations are rendered from
    target_latents [B,L], and the latent code is fitted from start_latents [B,L] (igr.igr_lattice_values carries the samples'
    gradient on to the code), with latent_reg |latent|^2 added as in fit_pointcloud_latent; target_rad and start_rad are not used.
    loss[s] = the mean over the scene's views of depth_residual_loss of the thrown body.  optimizer: "GD" or "Adam".
    Chamfer distances (chamfer.py) are between the level-set meshes (marching cubes at mesh_res, or of the fitted grid) of the
    estimate and of the target, each in its world frame.
    Returns dict(rad, pose, sdf (grid only), latent and target_latents (igr only), history [dict(iter, loss)], loss_start, loss_final,
    chamfer_start, chamfer_final [B], dropped [views,3] of the last backward pass)."""
    from . import depth_camera, meshsdf
    from .grids import GridTable
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    grid, neural = shape == "grid", shape == "igr"
    level = grid or neural      # the estimate is a level-set body seen through a grid
    if neural:
        from . import igr
        if packed is None or target_latents is None or start_latents is None:
            raise ValueError('fit_depth("igr"): give target_latents, start_latents and packed')
        nlat = igr.packed_shape(packed)[1]
        target_lat, start_lat = T(target_latents).reshape(-1, nlat), T(start_latents).reshape(-1, nlat)
        target_rad = start_rad = torch.ones(target_lat.shape[0], dtype=torch.float64)
        scale = 2.0 if scale is None else scale
    target_rad, start_rad = T(target_rad).reshape(-1), T(start_rad).reshape(-1)
    B, dev = target_rad.numel(), torch.device("cuda")
    ident = torch.tensor([1.0, 0, 0, 0, 0.0, 5.0, 0.0], dtype=torch.float64).repeat(B, 1)
    target_pose = ident.clone() if target_pose is None else T(target_pose).reshape(B, 7)
    start_pose = target_pose.clone() if start_pose is None or level else T(start_pose).reshape(B, 7)
    scale = float(1.5 * target_rad.max()) if scale is None else float(scale)
    W, H = int(size[0]), int(size[1])
    intr = (515.0 * W / 640.0, 515.0 * W / 640.0, W / 2.0 - 0.5, H / 2.0 - 0.5)
    cams = orbit_camera_poses(extra_cameras)
    kind = abi.SHAPE_SPHERE if shape in ("sphere", "grid") else abi.SHAPE_BOX_ROUNDED
    floor = torch.tensor([1.0, 0, 0, 0, 0.0, -0.5, 0.0], dtype=torch.float64)
    wall = torch.tensor([1.0, 0, 0, 0, 5.0, 5.0, 0.0], dtype=torch.float64)
    fixed_prm = torch.tensor([[20.0, 1.0, 20.0, 0.0], [1.0, 10.0, 10.0, 0.0]], dtype=torch.float64, device=dev)

    def scene(pose, rad, est):
        """-> pose [B,3,7], types [B,3], prm [B,3,4] of floor, wall and the thrown body (est and grid / igr: a voxel / neural body)."""
        ps = torch.stack([floor.to(dev).expand(B, 7), wall.to(dev).expand(B, 7), pose.to(dev)], 1)
        if est and level:
            body = torch.tensor([0.0, 0.0, 0.0, scale], dtype=torch.float64, device=dev).expand(B, 4)
            types = [abi.SHAPE_BOX, abi.SHAPE_BOX, abi.SHAPE_GRID if grid else abi.SHAPE_IGR]
        else:
            r = rad.to(dev)
            z = torch.zeros_like(r)
            body = torch.stack([r, z, z, z], 1) if kind == abi.SHAPE_SPHERE else torch.stack([2 * r, 2 * r, 2 * r, z + corner_r], 1)
            types = [abi.SHAPE_BOX, abi.SHAPE_BOX, kind]
        return ps, torch.tensor(types, dtype=torch.int32).repeat(B, 1), torch.cat([fixed_prm.expand(B, 2, 4), body[:, None]], 1)

    gid = torch.tensor([-1, -1, 0], dtype=torch.int32).repeat(B, 1) + torch.tensor([0, 0, 1], dtype=torch.int32) * torch.arange(B, dtype=torch.int32)[:, None]
    with torch.no_grad():
        tp, tt, tq = scene(target_pose, target_rad, neural)
        tvals = igr.igr_lattice_values(target_lat, packed, res) if neural else None
        ttable = GridTable(list(tvals), dev) if neural else None
        obs = [depth_camera.render_depth(tp, tt, tq, cam, *intr, size=(W, H), grids=ttable, grid_id=gid if neural else None) for cam in cams]
        tshape = "sphere" if kind == abi.SHAPE_SPHERE else "cube"
        tgt = []
        for s in range(B if neural else 0):      # the level set of the target's value grid
            v, _ = meshsdf.marching_cubes(tvals[s], 0.0)
            tgt.append(_pose_points((v.cpu().numpy() / (res - 1) * 2.0 - 1.0) * scale, target_pose[s].numpy()))
        for s in range(0 if neural else B):
            sc_t = 1.5 * float(target_rad[s])
            v, _ = meshsdf.marching_cubes(_sample_sdf(tshape, float(target_rad[s]), corner_r, mesh_res, sc_t).to(dev), 0.0)
            tgt.append(_pose_points((v.cpu().numpy() / (mesh_res - 1) * 2.0 - 1.0) * sc_t, target_pose[s].numpy()))
        tgt_cloud = chamfer_hip.pack(tgt, dev)
    rot, pos = start_pose[:, :4].clone().requires_grad_(not level), start_pose[:, 4:].clone().requires_grad_(not level)
    rad = start_rad.clone().requires_grad_(not level)
    lat = start_lat.clone().requires_grad_() if neural else None
    sdf = torch.stack([_sample_sdf("sphere", float(r), corner_r, res, scale) for r in start_rad]).to(dev).requires_grad_() if grid else None
    params = [sdf] if grid else [lat] if neural else [rot, pos, rad]
    lr = (0.02 if grid else 0.01 if neural else 0.05) if lr is None else lr
    opt = torch.optim.Adam(params, lr=lr) if optimizer == "Adam" else torch.optim.SGD(params, lr=lr)
    last = {}

    def losses():
        ps, ty, pq = scene(torch.cat([rot, pos], 1), rad, True)
        if neural:      # the value grids of all scenes, one network pass forward and one compacted pass backward
            last["vals"] = igr.igr_lattice_values(lat, packed, res)
        table = GridTable(list(sdf if grid else last["vals"]), dev) if level else None
        tot = 0.0
        for cam, (od, os_) in zip(cams, obs):
            d, sg, dr = depth_camera.render_depth_diff(ps, ty, pq, cam, *intr, size=(W, H), grids=table, grid_id=gid if level else None,
                                                       min_cos=min_cos, return_dropped=True)
            tot = tot + depth_residual_loss(d, sg, od, os_, 2)
            last["dropped"] = dr
        data = tot / len(cams)
        if neural:
            return data + latent_reg * (lat.to(dev) ** 2).sum(dim=1), data
        return (data + eik_reg * eikonal_residual(sdf), data) if grid else (data, data)

    def chamfer_now():
        with torch.no_grad():
            pose0, verts = torch.cat([rot, pos], 1).detach().numpy(), []
            fields = sdf if grid else igr.igr_lattice_values(lat.detach(), packed, res) if neural else None
            for s in range(B):
                if level:
                    field, n, sc_e = fields[s].detach(), res, scale
                else:
                    sc_e = 1.5 * float(rad[s])
                    field, n = _sample_sdf(tshape, float(rad[s]), corner_r, mesh_res, sc_e).to(dev), mesh_res
                v, _ = meshsdf.marching_cubes(field, 0.0)
                verts.append(_pose_points((v.cpu().numpy() / (n - 1) * 2.0 - 1.0) * sc_e, pose0[s]))
            return _chamfer_series(verts, tgt_cloud)

    chamfer_start, hist = chamfer_now(), []
    for e in range(max_iter + 1):      # (the last pass only evaluates)
        opt.zero_grad()
        loss, data = losses()
        hist.append(dict(iter=e, loss=loss.detach().cpu().numpy().copy(), data=data.detach().cpu().numpy().copy()))
        if neural:
            hist[-1]["latent"] = lat.detach().numpy().copy()
        if log:
            log("[depth %s] iter %3d  mean loss %.3e  (depth %.3e)%s" % (shape, e, float(hist[-1]["loss"].mean()), float(hist[-1]["data"].mean()),
                "  mean |latent - target| %.4f" % float((lat.detach() - target_lat).abs().mean()) if neural else ""))
        if e == max_iter:
            break
        loss.sum().backward()
        opt.step()
        with torch.no_grad():
            if not level:
                rot /= rot.norm(dim=1, keepdim=True)
                rad.clamp_(min=0.05)
    return dict(latent=None if lat is None else lat.detach().numpy().copy(), target_latents=target_lat.numpy() if neural else None,
                rad=rad.detach().numpy().copy(), pose=torch.cat([rot, pos], 1).detach().numpy().copy(), scale=scale,
                sdf=None if sdf is None else sdf.detach().cpu().numpy().copy(), history=hist, loss_start=hist[0]["data"], loss_final=hist[-1]["data"],
                chamfer_start=chamfer_start, chamfer_final=chamfer_now(), target_rad=target_rad.numpy(), target_pose=target_pose.numpy(),
                dropped=None if "dropped" not in last else last["dropped"].cpu().numpy())


# ---- trajectory fitting to recorded RGB-D sequences (trajectory_fitting/optim_pointcloud_real.py) ----------------------------
PLANE_DIMS = (1.5, 1.0, 1.5)      # :104
BALL_MASS = 0.058                 # :135


def plane_pose(planes, dims_y=PLANE_DIMS[1]):
    """Poses [...,7] of the boxes that stand for the fitted planes [...,4] (rows n, d: the plane n . x + d = 0 seen from the
    origin), optim_pointcloud_real.py:106-118: the rotation by angle = acos(n . e_y / |n|) about -(n x e_y) / |n x e_y| as a
    quaternion, and the centre -sign(d) n (|d| + dims_y / 2), n as given (not normalised, as there).  Where n is parallel to e_y,
    |n x e_y| < 1e-12, the reference divides by zero; here the rotation is then the identity (angle 0) or the half turn about x
    (angle pi)."""
    pl = torch.as_tensor(np.asarray(planes.detach().cpu() if torch.is_tensor(planes) else planes, np.float64))
    n, d = pl[..., :3], pl[..., 3]
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand_as(n)
    angle = torch.arccos((n * up).sum(-1) / n.norm(dim=-1))
    axis = torch.cross(n, up, dim=-1)
    an = axis.norm(dim=-1, keepdim=True)
    par = an < 1e-12
    axis = axis / torch.where(par, torch.ones_like(an), an)
    half = (0.5 * angle)[..., None]
    q = torch.cat([torch.cos(half), -axis * torch.sin(half)], -1)
    flat = torch.where(angle[..., None] < 0.5 * math.pi, torch.tensor([1.0, 0, 0, 0], dtype=torch.float64), torch.tensor([0.0, 1, 0, 0], dtype=torch.float64))
    q = torch.where(par, flat, q)
    pos = -torch.sign(d)[..., None] * n * (d.abs() + 0.5 * dims_y)[..., None]
    return torch.cat([q, pos], -1)


def plane_world(rad, planes, fric, restitution, pose, vel, g=10.0, shape="sphere", corner_r=0.2, res=128, max_steps=128, device=None):
    """`make_world` of optim_pointcloud_real.py:98-148 for B scenes: P boxes of PLANE_DIMS posed by plane_pose(planes [B,P,4]),
    pinned and mutually no_contact, and the thrown body -- shape 'sphere': an SDFSphere of radius rad and mass 0.058, 'cube': an
    SDFBoxRounded of dims 2 rad (1,1,1), r = corner_r and mass 1 -- at pose [B,7] with velocity vel [B,6] (angular, linear)
    under gravity g ([B] or a number) along -y; every body has the scene's fric [B] and restitution [B].
    strict_no_penetration and the time-of-contact differential are on.  rad, fric, restitution, pose and vel are torch tensors
    that may require grad.  Analytic meshes and inertias for the boxes and the sphere (the reference's custom_mesh /
    custom_inertia), the cube's level-set mesh and its inertia as in bounce_world."""
    T = lambda x: x.to(torch.float64).cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float64))
    rad, fric, restitution, pose, vel = T(rad).reshape(-1), T(fric).reshape(-1), T(restitution).reshape(-1), T(pose), T(vel)
    B = rad.numel()
    pl = np.asarray(T(planes).detach(), np.float64)
    pl = np.array(np.broadcast_to(pl, (B,) + pl.shape[-2:]))
    P, nb = pl.shape[1], pl.shape[1] + 1
    s_ = P
    gv = np.broadcast_to(np.asarray(T(g).detach(), np.float64).reshape(-1), (B,))
    spec, cache = scenes._base(B, nb), {}
    spec["Je"] = np.zeros((B, 6 * P, 6 * nb))
    spec["pose"][:, :P] = plane_pose(pl).numpy()
    nocon = np.zeros((nb, nb), np.uint8)
    nocon[:P, :P] = 1 - np.eye(P, dtype=np.uint8)
    spec["no_contact"] = nocon

    def make():
        v, f, tie = meshes.box_mesh(np.asarray(PLANE_DIMS))
        return v, f, 0.5 * tie
    for k in range(P):
        spec["mesh_id"][:, k] = scenes._add_mesh(spec, cache, ("box",) + PLANE_DIMS, make)
        spec["shape_prm"][:, k] = PLANE_DIMS
        spec["inertia"][:, k] = scenes.box_inertia(1.0, np.asarray(PLANE_DIMS))
        spec["Je"][:, 6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.eye(6)
    r_np = rad.detach().numpy()
    one = torch.tensor(1.0, dtype=torch.float64)
    verts = None
    if shape == "sphere":
        mass = BALL_MASS
        uv, uf = meshes.icosphere(4)
        for s in range(B):
            spec["mesh_id"][s, s_] = scenes._add_mesh(spec, cache, ("sphere", float(r_np[s])), lambda r=float(r_np[s]): (uv * r, uf, uv.copy()))
        spec["shape_type"][:, s_] = abi.SHAPE_SPHERE
        z = torch.zeros_like(rad)
        prm_body = torch.stack([rad, z, z], 1)
        I_body = (0.4 * mass * rad * rad)[:, None, None] * torch.eye(3, dtype=torch.float64)      # 2/5 m r^2 (bodies.py:993-994)
    elif shape == "cube":
        mass = 1.0
        spec["shape_aux"] = np.zeros((B, nb))
        spec["shape_aux"][:, s_] = corner_r
        spec["shape_type"][:, s_] = abi.SHAPE_BOX_ROUNDED
        vts, Is = [torch.as_tensor(m[0], dtype=torch.float64) for m in spec["meshes"]], []
        for s in range(B):      # (the level-set mesh and its inertia per scene, as _bounce_world_cube builds them)
            scale = 1.5 * rad[s]
            unit = torch.stack([2.0 * rad[s], 2.0 * rad[s], 2.0 * rad[s], torch.tensor(corner_r, dtype=torch.float64)]) / scale
            v, f = meshsdf.primitive_mesh(abi.SHAPE_BOX_ROUNDED, unit, res=res)
            v = v * scale.to(v.device)
            Is.append(mass_properties.mesh_inertia_diff(v, f, one).cpu())
            spec["meshes"].append((v.detach().cpu().numpy(), f.cpu().numpy())); spec["mesh_vgrad"].append(np.zeros((v.shape[0], 3)))
            spec["mesh_id"][s, s_] = len(spec["meshes"]) - 1
            vts.append(v)
        prm_body = (2.0 * rad)[:, None].expand(B, 3)
        I_body = torch.stack(Is)
        if rad.requires_grad:
            verts = torch.cat([v.to(vts[-1].device) for v in vts])
    else:
        raise ValueError("shape: 'sphere' or 'cube', got %r" % (shape,))
    spec["mass"][:, s_] = mass
    spec["fext"][:, s_, 4] = -gv * mass
    prm0, I0 = torch.tensor(spec["shape_prm"], dtype=torch.float64), torch.tensor(spec["inertia"], dtype=torch.float64)
    params = dict(shape_prm=torch.cat([prm0[:, :s_], prm_body[:, None]], 1), inertia=torch.cat([I0[:, :s_], I_body[:, None]], 1),
                  fric=fric[:, None].expand(B, nb), restitution=restitution[:, None].expand(B, nb))
    if verts is not None:
        params["verts"] = verts
    for k, v in params.items():
        if k != "verts":
            spec[k] = v.detach().numpy().copy()
    spec["pose"][:, s_] = pose.detach().numpy()
    spec["vel"][:, s_] = vel.detach().numpy()
    big = dict(maxc=256, max_cand=32768, max_pc=128) if shape == "cube" else {}
    w = BatchWorld3D(spec, params=params, dt=Defaults3D.DT, time_of_contact_diff=True, strict_no_penetration=True,
                     max_substeps=8 * int(max_steps) + 64, device=device, **big)
    _connect_start_pose(w, s_, pose)
    w.vel = torch.cat([w.vel[:, :s_], vel.to(w.vel)[:, None], w.vel[:, s_ + 1:]], 1)
    return w


def run_world_frames(world, nframes, detach_2nd_bounce=False, body=-1):
    """`run_world_fixed_dt` of optim_pointcloud_real.py:199-223 per scene: entry 0 is the body's start pose, then one entry per
    outer step of Defaults3D.DT, nframes - 1 entries in all (the last observed frame has none, as there).  nframes: a number or
    [B]; a scene whose frames have ended is masked out of the steps.  detach_2nd_bounce: the second step in a row (since the last
    cut) that ends in contact is undone, its scene's poses and velocities are cut from the graph, the entry before it is
    replaced by the cut state (the script pops it and appends it again) and the frame is stepped once more.
    -> dict(pose [K,B,7] with its graph, valid [K,B], repeated: per scene the frames stepped twice)."""
    B, dev = world.B, world.device
    T = np.broadcast_to(np.asarray(nframes, np.int64).reshape(-1), (B,))
    K = max(int(T.max()) - 1, 1)
    entries = [world.pose[:, body]] + [None] * (K - 1)
    frame, num_contact, repeated = np.ones(B, np.int64), np.zeros(B, np.int64), [[] for _ in range(B)]
    while True:
        mask = frame < T - 1
        if not mask.any():
            break
        had = np.asarray(world.step(mask=mask)) & mask
        redo = np.zeros(B, bool)
        if detach_2nd_bounce:
            num_contact += had
            redo = had & (num_contact > 1)
            if redo.any():
                world.undo_step(redo)
                world.detach_state(redo)
                num_contact[redo] = 0
                for s in np.nonzero(redo)[0]:
                    repeated[s].append(int(frame[s]))
        cur = world.pose[:, body]
        at = frame - redo
        for k in np.unique(at[mask]):
            sel = torch.as_tensor(mask & (at == k), device=dev)[:, None]
            entries[k] = torch.where(sel, cur, entries[k] if entries[k] is not None else torch.zeros_like(cur))
        frame = frame + (mask & ~redo)
    pose = torch.stack([e if e is not None else torch.zeros_like(entries[0]) for e in entries])
    valid = torch.as_tensor(np.arange(K)[:, None] < np.maximum(T - 1, 1)[None, :], device=dev)
    return dict(pose=pose, valid=valid, repeated=repeated)


def recorded_observations(recordings, label=4):
    """The thrown body's points of B recordings (dicts with pcs [T,H,W,3], segs [T,H,W] on the device: recorded.load_recording,
    synthesize_recording) as one set of segments, recording after recording, frame after frame (recorded.select_points), with
    their statistics (recorded.segment_stats).  -> dict(pts, seg_off, scene [nseg], frame [nseg], first [B] (a scene's first
    segment), nframes [B], stats)."""
    from . import recorded
    pts, off, scene, frame, first = [], [np.zeros(1, np.int64)], [], [], []
    for b, rec in enumerate(recordings):
        p, o = recorded.select_points(rec["pcs"], rec["segs"], label)
        first.append(len(scene))
        pts.append(p); off.append(o[1:] + off[-1][-1])
        scene.extend([b] * (len(o) - 1)); frame.extend(range(len(o) - 1))
    pts, off = torch.cat(pts), np.concatenate(off)
    return dict(pts=pts, seg_off=off, scene=np.asarray(scene, np.int64), frame=np.asarray(frame, np.int64), first=np.asarray(first, np.int64),
                nframes=np.asarray([r["segs"].shape[0] for r in recordings], np.int64), stats=recorded.segment_stats(pts, off))


def recorded_trajectory_loss(traj, obs, rad, shape, corner_r=0.2, match=None):
    """`trajectory_loss` of optim_pointcloud_real.py:170-196: entry i of a scene's trajectory (run_world_frames) is compared with
    the points of its frame i; per scene sum / max(1, count).  -> [B]"""
    ok = traj["valid"].cpu().numpy()
    ent = np.argwhere(ok & (np.arange(ok.shape[0])[:, None] < obs["nframes"][None, :]))      # (entry, scene)
    dev = traj["pose"].device
    pose = traj["pose"][torch.as_tensor(ent[:, 0], device=dev), torch.as_tensor(ent[:, 1], device=dev)]
    return pointcloud_frame_loss(obs, obs["first"][ent[:, 1]] + ent[:, 0], pose, rad, shape, corner_r, match)


def fit_recorded(recordings, shape="sphere", lr=0.1, max_iter=200, optimizer="GD", conv_thresh=1e-7, conv_thresh_shape=1e-5,
                 detach_2nd_bounce=True, optimize_init_pose=True, fit_first_frame=True, fit_trajectory=True, start_rad=None,
                 start_pose0=None, start_pose1=None, corner_r=0.2, label=4, log=None, device=None, res=128):
    """optim_pointcloud_real.py:326-557 for B recordings at once (dicts of pcs, segs, planes [P,4], g; the same number of planes in
    each).  From the statistics of the labelled points of frames 0 and 1: diam0 = the largest side of frame 0's bounding box,
    start radius diam0 / 2, start positions = the two centroids pushed diam0 / 2 away from the origin (:326-336); start_rad [B],
    start_pose0 / start_pose1 [B,7] replace them.
      first frame   rad, and with optimize_init_pose the poses of frames 0 and 1, on the loss of those two frames (:366-445)
      trajectory    rad, rot, pos, vel [6] = (0, (pos1 - pos0) / DT + g DT e_y), fric (0.15), restitution (0.7): plane_world,
                    run_world_frames(detach_2nd_bounce), recorded_trajectory_loss (:468-556)
    GD or Adam; as in fit_pointcloud a scene whose loss moved by less than conv_thresh and its rad by less than conv_thresh_shape
    is frozen; after a step the start rotation is renormalised (frame 1's is not, as in the script).
    -> (first_frame, trajectory): the script's two result dicts, arrays with a leading [B]."""
    obs = recorded_observations(recordings, label)
    B, DT = len(recordings), Defaults3D.DT
    st = {k: v.cpu() for k, v in obs["stats"].items()}
    f0, f1 = torch.as_tensor(obs["first"]), torch.as_tensor(obs["first"] + 1)
    if bool((st["count"][f0] < 1).any() or (st["count"][f1] < 1).any()):
        raise ValueError("a recording shows no point of label %d in its first two frames" % label)
    diam0 = (st["max"][f0] - st["min"][f0]).max(dim=1).values
    push = lambda c: c + c / c.norm(dim=1, keepdim=True) * diam0[:, None] / 2
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    ident = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64).repeat(B, 1)
    pose0 = torch.cat([ident, push(st["mean"][f0])], 1) if start_pose0 is None else T(start_pose0).reshape(B, 7)
    pose1 = torch.cat([ident, push(st["mean"][f1])], 1) if start_pose1 is None else T(start_pose1).reshape(B, 7)
    start = (diam0 / 2 if start_rad is None else T(start_rad).reshape(B)).clone()
    rad = start.clone().requires_grad_()
    leaf = lambda x: x.clone().requires_grad_(optimize_init_pose)
    rot0, pos0, rot1, pos1 = leaf(pose0[:, :4]), leaf(pose0[:, 4:]), leaf(pose1[:, :4]), leaf(pose1[:, 4:])
    planes = torch.stack([T(r["planes"].cpu() if torch.is_tensor(r["planes"]) else r["planes"]).reshape(-1, 4) for r in recordings])
    g = T([float(r["g"]) for r in recordings])

    def descend(stage, var, loss_fn):
        opt = torch.optim.Adam(var, lr=lr) if optimizer == "Adam" else torch.optim.SGD(var, lr=lr)
        done, last, last_rad = np.zeros(B, bool), np.full(B, 1e10), np.full(B, 1e10)
        h = dict(loss_hist=[], rad_hist=[], init_pose_hist=[])
        for e in range(max_iter):
            opt.zero_grad()
            loss = loss_fn()
            loss.sum().backward()
            l, r_now = loss.detach().cpu().numpy(), rad.detach().numpy().copy()
            done |= (np.abs(last - l) < conv_thresh) & (np.abs(last_rad - r_now) < conv_thresh_shape)
            h["loss_hist"].append(l.copy()); h["rad_hist"].append(r_now); h["init_pose_hist"].append(torch.cat([rot0, pos0], 1).detach().numpy().copy())
            if log:
                log("[%s] iter %3d  mean loss %.3e  mean rad %.5f  converged %d / %d" % (stage, e, float(l.mean()), float(r_now.mean()), int(done.sum()), B))
            if done.all():
                break
            frozen = torch.as_tensor(done)
            for v in var:
                if v.grad is None:
                    v.grad = torch.zeros_like(v)
                v.grad[frozen] = 0.0
            keep = [v.detach().clone() for v in var]
            opt.step()
            with torch.no_grad():
                for v, k in zip(var, keep):      # (Adam's momentum would still move a frozen scene)
                    v[frozen] = k[frozen]
                if rot0.requires_grad:
                    rot0.div_(rot0.norm(dim=1, keepdim=True))
            last, last_rad = l, r_now
        h["final_loss"] = h["loss_hist"][-1]
        return h

    first_frame = traj_out = None
    if fit_first_frame:
        segs = np.concatenate([obs["first"], obs["first"] + 1])
        h = descend("first frame", [rad] + ([rot0, rot1, pos0, pos1] if optimize_init_pose else []),
                    lambda: pointcloud_frame_loss(obs, segs, torch.cat([torch.cat([rot0, pos0], 1), torch.cat([rot1, pos1], 1)]), rad, shape, corner_r))
        first_frame = dict(start_rad=start.numpy().copy(), final_rad=rad.detach().numpy().copy(), final_pose=torch.cat([rot0, pos0], 1).detach().numpy().copy(),
                           init_pose1=torch.cat([rot1, pos1], 1).detach().numpy().copy(), **h)
    if fit_trajectory:
        rot0.requires_grad_(True); pos0.requires_grad_(True)
        lin = ((pos1 - pos0) / DT).detach() + torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) * (g * DT)[:, None]
        vel = torch.cat([torch.zeros(B, 3, dtype=torch.float64), lin], 1).requires_grad_()
        fric = torch.full((B,), 0.15, dtype=torch.float64, requires_grad=True)
        rest = torch.full((B,), 0.7, dtype=torch.float64, requires_grad=True)

        def traj_loss():
            world = plane_world(rad, planes, fric, rest, torch.cat([rot0, pos0], 1), vel, g, shape, corner_r, res, int(obs["nframes"].max()) + 8, device)
            return recorded_trajectory_loss(run_world_frames(world, obs["nframes"], detach_2nd_bounce), obs, rad, shape, corner_r)
        h = descend("trajectory", [rad, rot0, pos0, vel, fric, rest], traj_loss)
        traj_out = dict(start_rad=start.numpy().copy(), final_rad=rad.detach().numpy().copy(), final_pose=torch.cat([rot0, pos0], 1).detach().numpy().copy(),
                        init_vel=vel.detach().numpy().copy(), friction=fric.detach().numpy().copy(), restitution=rest.detach().numpy().copy(), **h)
    return first_frame, traj_out


def recording_camera(W=640, H=480):
    """The pinhole camera of synthesize_recording: at the origin of the recording's frame, looking along -z, +y up; 515 pixels of
    focal length at 640 x 480 (CAMERA), scaled with the width."""
    f = CAMERA["fx"] * W / 640.0
    return dict(fx=f, fy=f, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, size=(W, H), znear=0.05, zfar=100.0)


def synthesize_recording(rad=(0.1,), planes=((0.0, 1.0, 0.0, 0.3), (-1.0, 0.0, 0.0, 0.4)), pos=(-0.25, -0.05, -0.6), vel=(1.2, 0.5, 0.0),
                         fric=0.15, restitution=0.7, g=9.81, nframes=12, size=(80, 60), shape="sphere", noise=0.0, seed=0, device=None):
    """Recordings without a camera: plane_world with the given truth rolled out for nframes frames, every frame rendered by
    depth_camera.render_depth from the origin (recording_camera) and every pixel back-projected to the organised cloud, as a
    depth sensor's driver does.  Labels: the thrown body 4, plane k -> k + 1, nothing hit 0 (its point is NaN, as a sensor
    reports a pixel without depth).  One recording per entry of `rad`; planes [P,4] or [B,P,4].
    -> list of dicts(pcs, segs, planes, grav_dir, g, rgbs=None, truth=dict(rad, pose [nframes,7], vel0, fric, restitution))."""
    from . import depth_camera
    rad = torch.as_tensor(np.asarray(rad, np.float64)).reshape(-1)
    B = rad.numel()
    pl = np.array(np.broadcast_to(np.asarray(planes, np.float64), (B,) + np.asarray(planes).shape[-2:]))
    P = pl.shape[1]
    pose0 = torch.tensor([1.0, 0, 0, 0] + list(pos), dtype=torch.float64).repeat(B, 1)
    vel0 = torch.tensor([0.0, 0, 0] + list(vel), dtype=torch.float64).repeat(B, 1)
    full = lambda x: torch.full((B,), float(x), dtype=torch.float64)
    cam = recording_camera(*size)
    W, H = cam["size"]
    with torch.no_grad():
        w = plane_world(rad, pl, full(fric), full(restitution), pose0, vel0, g, shape, max_steps=nframes + 8, device=device)
        poses = [w.pose]
        for _ in range(nframes - 1):
            w.step(keep_undo=False)
            poses.append(w.pose)
        poses = torch.stack(poses, 1)                                           # [B,nframes,nb,7]
        E = w.engine
        aux = E.arr["shape_aux"] if "shape_aux" in E.arr else torch.zeros_like(E.arr["shape_prm"][..., 0])
        prm = torch.cat([E.arr["shape_prm"], aux[..., None]], 2)
        dev = poses.device
        col = (torch.arange(W, dtype=torch.float64, device=dev) + 0.5 - cam["cx"]) / cam["fx"]
        row = (torch.arange(H, dtype=torch.float64, device=dev) + 0.5 - cam["cy"]) / cam["fy"]
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        lab = torch.tensor(list(range(1, P + 1)) + [4, 0], dtype=torch.int32, device=dev)      # body index -> label; -1 (nothing) -> 0
        out = []
        for b in range(B):
            depth, seg = depth_camera.render_depth(poses[b], E.arr["shape_type"][b:b + 1].expand(nframes, -1).contiguous(),
                                                   prm[b:b + 1].expand(nframes, -1, -1).contiguous(), np.eye(4), **cam)
            if noise > 0:
                depth = depth + torch.randn(depth.shape, dtype=depth.dtype, device=dev, generator=gen) * noise * depth ** 2
            hit = seg >= 0
            d = torch.where(hit, depth, torch.full_like(depth, float("nan")))
            pcs = torch.stack([col[None, None, :] * d, -row[None, :, None] * d, -d], 3).contiguous()      # the camera frame is the world frame
            segs = lab[torch.where(hit, seg, torch.full_like(seg, P + 1)).long()].contiguous()
            out.append(dict(pcs=pcs, segs=segs, planes=torch.as_tensor(pl[b].copy()), grav_dir=torch.tensor([0.0, -float(g), 0.0], dtype=torch.float64),
                            g=float(g), rgbs=None,
                            truth=dict(rad=float(rad[b]), pose=poses[b, :, -1].cpu().numpy(), vel0=vel0[b].numpy(), fric=float(fric), restitution=float(restitution))))
    return out


# ---- trajectory fitting in shape space: a neural-SDF body thrown at a wall (trajectory_fitting/optim_shapespace.py) ----------
def bounce_world_latent(latents, packed, use_toc_diff=True, use_friction=True, use_wall=True, use_floor=True, use_gravity=False,
                        obj_pos=(0.0, 5.0, 0.0), obj_vel=(5.0, 0.0, 0.0), run_time=1.5, dt=Defaults3D.DT, res=128, device=None):
    """trajectory_fitting/optim_shapespace.py:90-124 for one scene per latent code: floor 50 x 1 x 50, wall [5,5,0] 1 x 10 x 10
    (pinned, no contact with each other), the neural-SDF body (scale 1, mass 1) at (0,5,0) thrown with (5,0,0); restitution
    0.5, friction 0.25; no gravity by default, strict_no_penetration=False.  `latents` [B, 2] with a `packed` of the bob_spot
    shape, [B, 4] with one of the shapenet shape (scenes.set_latents).  With `latents` a tensor that requires grad the
    scene is differentiable w.r.t. it three ways, as the reference's is: the SDF the contacts query, the level-set mesh
    (MeshSDF) the contact candidates come from, and the inertia integrated over that mesh."""
    lat_t = torch.as_tensor(latents, dtype=torch.float64)
    lat = lat_t.detach().cpu().numpy()
    B = lat.shape[0]
    fixed = [n for n, on in (("floor", use_floor), ("wall", use_wall)) if on]
    nb = len(fixed) + 1
    mu = 0.25 if use_friction else 0.0
    spec, cache = scenes._base(B, nb), {}
    spec["Je"] = np.zeros((B, 6 * len(fixed), 6 * nb))
    nocon = np.zeros((nb, nb), np.uint8)
    for k, name in enumerate(fixed):
        dims, pos = ((50.0, 1.0, 50.0), (0.0, -0.5, 0.0)) if name == "floor" else ((1.0, 10.0, 10.0), (5.0, 5.0, 0.0))

        def make(dims=dims):
            v, f, tie = meshes.box_mesh(np.asarray(dims))
            return v, f, 0.5 * tie
        spec["mesh_id"][:, k] = scenes._add_mesh(spec, cache, ("box",) + tuple(dims), make)
        spec["pose"][:, k, 4:] = pos
        spec["shape_prm"][:, k] = dims
        spec["inertia"][:, k] = scenes.box_inertia(1.0, np.asarray(dims))
        spec["fric"][:, k] = mu
        spec["restitution"][:, k] = Defaults3D.RESTITUTION
        spec["Je"][:, 6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.eye(6)
    if len(fixed) == 2:
        nocon[0, 1] = nocon[1, 0] = 1
    spec["no_contact"] = nocon
    s_ = nb - 1
    spec["shape_aux"] = np.zeros((B, nb))
    spec["igr_net"] = packed
    spec["shape_type"][:, s_] = abi.SHAPE_IGR
    spec["shape_aux"][:, s_] = 1.0
    one = torch.tensor(1.0, dtype=torch.float64)
    vts, Is = [torch.as_tensor(m[0], dtype=torch.float64) for m in spec["meshes"]], []
    for s in range(B):
        v, f = meshsdf.igr_mesh(lat_t[s], packed, res=res)
        Is.append(mass_properties.mesh_inertia_diff(v, f, one).cpu())
        spec["meshes"].append((v.detach().cpu().numpy(), f.cpu().numpy())); spec["mesh_vgrad"].append(np.zeros((v.shape[0], 3)))
        spec["mesh_id"][s, s_] = len(spec["meshes"]) - 1
        vts.append(v)
    scenes.set_latents(spec, s_, lat, packed)
    spec["pose"][:, s_, 4:] = obj_pos
    spec["vel"][:, s_, 3:] = obj_vel
    spec["inertia"][:, s_] = torch.stack(Is).detach().numpy()
    spec["fric"][:, s_] = mu
    spec["restitution"][:, s_] = Defaults3D.RESTITUTION
    if use_gravity:
        spec["fext"][:, s_, 4] = -10.0
    params = {}
    if lat_t.requires_grad:
        # the code where the SDF queries read it: two numbers in the body's shape_prm row, four in its row of the latent table
        key, width = ("igr_latent", abi.IGR_LATENT_MAX) if "igr_latent" in spec else ("shape_prm", 3)
        prm = torch.tensor(spec[key], dtype=torch.float64)
        mine = torch.cat([lat_t.cpu(), torch.zeros(B, width - lat.shape[1], dtype=torch.float64)], 1)[:, None]
        inertia = torch.tensor(spec["inertia"], dtype=torch.float64)
        dev = vts[-1].device
        params = {key: torch.cat([prm[:, :s_], mine], 1), "inertia": torch.cat([inertia[:, :s_], torch.stack(Is)[:, None]], 1),
                  "verts": torch.cat([v.to(dev) for v in vts])}
    steps = int(math.ceil(run_time / dt)) + 2
    w = BatchWorld3D(spec, params=params, dt=dt, time_of_contact_diff=use_toc_diff, strict_no_penetration=False,
                     max_substeps=8 * steps + 64, device=device, maxc=256, max_cand=8192, max_pc=128)
    w.body_meshes = spec["meshes"][-B:]      # the thrown body's mesh per scene, as bounce_world keeps it
    return w


def fit_trajectory_latent(target_latents, start_latents, packed, run_time=1.0, max_iter=100, lr=1e-3, conv_thresh=1e-5,
                          latent_reg=1e-4, optimizer="Adam", detach_2nd_bounce=True, log=None, **scene):
    """trajectory_fitting/optim_shapespace.py:232-320 for B scenes at once (its settings: Adam, lr 1e-3, run_time 1,
    latent_reg 1e-4): the latent code is fitted so that the thrown body's trajectory (its positions at the nearest target
    times, trajectory_loss) matches the target's; loss = trajectory_loss + latent_reg |latent|^2."""
    with torch.no_grad():
        wt = bounce_world_latent(torch.as_tensor(np.asarray(target_latents, np.float64)), packed, run_time=run_time, **scene)
        target = run_world_fixed_dt(wt, run_time)
        tgt_cloud = chamfer_hip.pack([m[0] for m in wt.body_meshes])
    lat = torch.tensor(np.asarray(start_latents, np.float64), requires_grad=True)
    opt = torch.optim.Adam([lat], lr=lr) if optimizer == "Adam" else torch.optim.SGD([lat], lr=lr)
    hist, last = [], None
    for e in range(max_iter):
        opt.zero_grad()
        world = bounce_world_latent(lat, packed, run_time=run_time, **scene)
        traj = run_world_fixed_dt(world, run_time, detach_2nd_bounce=detach_2nd_bounce)
        loss = trajectory_loss(traj, target)
        loss = loss + latent_reg * (lat.to(loss.device) ** 2).sum(dim=1)
        loss.sum().backward()
        l = loss.detach().cpu().numpy()
        d = _chamfer_series([m[0] for m in world.body_meshes], tgt_cloud)
        hist.append(dict(iter=e, loss=l.copy(), latent=lat.detach().numpy().copy(), grad=lat.grad.numpy().copy(), chamfer=d))
        if log:
            log("iter %3d  mean loss %.3e  mean chamfer %.3e  mean |latent - target| %.4f  |grad| %.3e" %
                (e, float(l.mean()), float(d.mean()), float(np.abs(lat.detach().numpy() - np.asarray(target_latents)).mean()), float(lat.grad.abs().mean())))
        if last is not None and np.all(np.abs(last - l) < conv_thresh):
            break
        opt.step()
        last = l
    return dict(latent=lat.detach().numpy().copy(), target=np.asarray(target_latents), history=hist)


def fit_pointcloud_latent(target_latents, start_latents, packed, target_pose=None, start_pose=None, run_time=1.0, max_iter=100, lr=1e-3,
                          conv_thresh=1e-5, latent_reg=1e-4, optimizer="Adam", noise=0.0, every=1, detach_2nd_bounce=True,
                          fit_first_frame=True, fit_trajectory=True, optimize_pose=False, seed=0, log=None, observe="vertices", **scene):
    """The two stages of fit_pointcloud for a neural body: the latent code [B, L] (and, with optimize_pose, the start pose) is
    fitted to what the camera records of bounce_world_latent(target_latents) (pointcloud_observations, either `observe` mode).
      first frame   the loss of observation 0 seen from the start pose, through the network alone (dss_pointcloud_loss_igr),
      trajectory    bounce_world_latent + run_world_fixed_dt + pointcloud_trajectory_loss: the latent gradient arrives through the
                    loss and through the stepper (SDF queries, level-set mesh, inertia).
    Adam, lr 1e-3 and latent_reg 1e-4 as fit_trajectory_latent; loss = point-cloud loss + latent_reg |latent|^2 per scene.
    Returns dict(latent, pose, target, history: {'frame': [...], 'trajectory': [...]}, observations)."""
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    target = T(target_latents)
    B = target.shape[0]
    obj_pos = scene.get("obj_pos", (0.0, 5.0, 0.0))
    ident = torch.tensor([1.0, 0, 0, 0, *obj_pos], dtype=torch.float64).repeat(B, 1)
    target_pose = ident.clone() if target_pose is None else T(target_pose).reshape(B, 7)
    with torch.no_grad():
        wt = bounce_world_latent(target, packed, run_time=run_time, **scene)
        obs = pointcloud_observations(wt, camera_pose(), noise=noise, every=every, run_time=run_time, seed=seed, observe=observe)
    lat = T(start_latents).clone().requires_grad_()
    start_pose = target_pose.clone() if start_pose is None else T(start_pose).reshape(B, 7)
    rot, pos = start_pose[:, :4].clone().requires_grad_(optimize_pose), start_pose[:, 4:].clone().requires_grad_(optimize_pose)
    var = [lat] + ([rot, pos] if optimize_pose else [])
    first = np.nonzero(obs["time"] < 0)[0]
    hist = {}
    for stage in [n for n, on in (("frame", fit_first_frame), ("trajectory", fit_trajectory)) if on]:
        opt = torch.optim.Adam(var, lr=lr) if optimizer == "Adam" else torch.optim.SGD(var, lr=lr)
        last, h = None, []
        for e in range(max_iter):
            opt.zero_grad()
            pose0 = torch.cat([rot, pos], 1)
            if stage == "frame":
                loss = pointcloud_frame_loss(obs, first, pose0[obs["scene"][first]], None, "igr", packed=packed, latent=lat)
            else:
                world = bounce_world_latent(lat, packed, run_time=run_time, **scene)
                traj = run_world_fixed_dt(world, run_time, detach_2nd_bounce=detach_2nd_bounce)
                loss = pointcloud_trajectory_loss(traj, obs, None, "igr", packed=packed, latent=lat)
            loss = loss + latent_reg * (lat.to(loss.device) ** 2).sum(dim=1)
            loss.sum().backward()
            l = loss.detach().cpu().numpy()
            h.append(dict(iter=e, loss=l.copy(), latent=lat.detach().numpy().copy(), grad=lat.grad.numpy().copy(), pose=pose0.detach().numpy().copy()))
            if log:
                log("[%s] iter %3d  mean loss %.3e  mean |latent - target| %.4f  |grad| %.3e" %
                    (stage, e, float(l.mean()), float((lat.detach() - target).abs().mean()), float(lat.grad.abs().mean())))
            if last is not None and np.all(np.abs(last - l) < conv_thresh):
                break
            opt.step()
            if optimize_pose:
                with torch.no_grad():
                    rot /= rot.norm(dim=1, keepdim=True)
            last = l
        hist[stage] = h
    return dict(latent=lat.detach().numpy().copy(), pose=torch.cat([rot, pos], 1).detach().numpy().copy(), target=target.numpy(),
                history=hist, observations=obs)


# ---- inertia fitting: a neural-SDF body spun by a torque (optim_shapespace.py) ------------------------------------------------
def spin_world(latents, torque_dirs, packed, scale=1.0, mass=1.0, res=128, steps=64, device=None, keep_meshes=True):
    """optim_shapespace.py:71-92 for one scene per latent code: a single neural-SDF body (scale 1) whose translation is locked
    by X/Y/Z constraints; no contacts, so only its inertia matters -- integrated over its level-set mesh (MeshSDF:
    differentiable w.r.t. the latent).  The torque (t < 0.3) is applied by the caller through world.params['fext'].
    keep_meshes='device': world.meshes as with False, the vertices stay on the device as world.mesh_verts (what the chamfer
    distance of the report reads)."""
    B = latents.shape[0]
    Is, ms, vs = [], [], []
    for s in range(B):
        v, f = meshsdf.igr_mesh(latents[s], packed, res=res)
        vt = v * scale
        Is.append(mass_properties.mesh_inertia_diff(vt, f, torch.tensor(float(mass), dtype=torch.float64)))
        # (the meshes are only kept for the chamfer distance of the experiment's report; a caller that does not need them saves
        # a device -> host copy of ~1 MB and a synchronisation per scene)
        ms.append((vt.detach().cpu().numpy(), f.cpu().numpy()) if keep_meshes is True else (None, int(f.shape[0])))
        vs.append(vt.detach())
    return _spin_world(torch.stack(Is), ms, scale, mass, steps, device, vs if keep_meshes else None)


def _spin_world(inertias, ms, scale, mass, steps, device, verts=None):
    """One free-spinning body per scene with the given body-frame inertia tensors [B, 3, 3] (graph kept) and meshes; verts: the
    meshes' vertices per scene as tensors of any device (world.mesh_verts; default: those of `ms`)."""
    B = len(ms)
    inertia = inertias[:, None]                                               # [B,1,3,3], graph to the shape parameters
    one = lambda a: np.tile(np.asarray(a, np.float64), (B, 1, 1))
    spec = dict(pose=one([1.0, 0, 0, 0, 0, 0, 0]), vel=one(np.zeros(6)), mass=np.full((B, 1), float(mass)),
                inertia=inertia.detach().cpu().numpy(), restitution=np.zeros((B, 1)), fric=np.zeros((B, 1)), fext=np.zeros((B, 1, 6)),
                shape_type=np.full((B, 1), abi.SHAPE_SPHERE, np.int32), shape_prm=one([scale, 0, 0]),      # (nothing collides: the shape is never queried)
                # (a lone body per scene: the stepper never searches its mesh, so it gets one shared triangle instead of B
                # level-set meshes of 10^5 faces whose search structures would take seconds to build; the real meshes stay on
                # the world object for the chamfer distance)
                mesh_id=np.zeros((B, 1), np.int32), meshes=[(0.1 * np.eye(3), np.array([[0, 1, 2]]))], mesh_vgrad=[np.zeros((3, 3))],
                Je=np.tile(np.concatenate([np.zeros((3, 3)), np.eye(3)], 1), (B, 1, 1)), no_contact=np.zeros((1, 1), np.uint8))
    w = BatchWorld3D(spec, params=dict(inertia=inertia), max_substeps=steps + 16, device=device)
    w.meshes = ms
    w.mesh_verts = verts if verts is not None else [m[0] for m in ms]
    return w


PRIMITIVES = {"box": 3, "sphere": 1, "cylinder": 2}      # parameters per kind (optim_primitives.py:77-92)


def primitive_spin_world(kind, dims, mass=1.0, steps=64, device=None):
    """optim_primitives.py:95-115 for one scene per parameter row: an SDFBox / SDFSphere / SDFCylinder at the origin with the
    reference's defaults there (custom_mesh = custom_inertia = False: marching-cubes mesh of the analytic SDF, inertia from that
    mesh, differentiable w.r.t. the dimensions through the mesher), translation locked."""
    from .physics3d import SDFBox, SDFCylinder, SDFSphere
    make = {"box": lambda d: SDFBox([0, 0, 0], d, mass=mass, custom_mesh=False, custom_inertia=False),
            "sphere": lambda d: SDFSphere([0, 0, 0], d[0], mass=mass, custom_mesh=False, custom_inertia=False),
            "cylinder": lambda d: SDFCylinder([0, 0, 0], rad=d[0], height=d[1], mass=mass, custom_mesh=False, custom_inertia=False)}[kind]
    bodies = [make(dims[s]) for s in range(dims.shape[0])]
    ms = [(b.verts_np, np.asarray(b.faces_np)) for b in bodies]
    return _spin_world(torch.stack([b.ang_inertia.to(torch.float64).cpu() for b in bodies]), ms, 1.0, mass, steps, device)


def run_spin(world, torque_dirs, run_time=2.0, torque_time=0.3):
    """`run_world(world, run_time=...)` with the experiment's force function: torque_dir for t < 0.3, then nothing."""
    B = world.B
    tq = torch.cat([torch.as_tensor(torque_dirs, dtype=torch.float64), torch.zeros(B, 3, dtype=torch.float64)], 1)[:, None]
    while float(world.t.min()) < run_time:
        world.params["fext"] = tq if float(world.t.min()) < torque_time else torch.zeros_like(tq)
        world.step()
    return world.vel[:, 0]


def fit_inertia_latent(target_latents, start_latents, torque_dirs, packed, run_time=2.0, max_iter=20, lr=1e-2, latent_reg=0.0,
                       conv_thresh=1e-7, res=128, log=None):
    """optim_shapespace.py:136-250: gradient descent on the latent code so that the body's final velocity under the torque
    matches the target's.  The gradient runs latent -> level-set mesh (MeshSDF) -> volume integrals -> world-frame inertia ->
    linear solve of every step."""
    steps = int(math.ceil(run_time / Defaults3D.DT)) + 2
    with torch.no_grad():
        wt = spin_world(torch.as_tensor(target_latents, dtype=torch.float64), torque_dirs, packed, res=res, steps=steps, keep_meshes="device")
        v_target = run_spin(wt, torque_dirs, run_time).clone()
        tgt_cloud = chamfer_hip.pack(wt.mesh_verts)      # (once: the target's vertices of every scene, packed on the device)
    lat = torch.tensor(np.asarray(start_latents, np.float64), requires_grad=True)
    hist, last = [], None
    for e in range(max_iter):
        if lat.grad is not None:
            lat.grad = None
        w = spin_world(lat, torque_dirs, packed, res=res, steps=steps, keep_meshes="device")
        v = run_spin(w, torque_dirs, run_time)
        loss = ((v - v_target.to(v)) ** 2).sum(dim=1) + latent_reg * (lat.to(v.device) ** 2).sum(dim=1)
        loss.sum().backward()
        l = loss.detach().cpu().numpy()
        d = _chamfer_series(w.mesh_verts, tgt_cloud)
        hist.append(dict(iter=e, loss=l.copy(), latent=lat.detach().numpy().copy(), grad=lat.grad.numpy().copy(), chamfer=d))
        if log:
            log("iter %3d  mean loss %.3e  mean chamfer %.3e  |grad| %.3e" % (e, float(l.mean()), float(d.mean()), float(lat.grad.abs().mean())))
        if last is not None and np.all(np.abs(last - l) < conv_thresh):
            break
        with torch.no_grad():
            lat -= lr * lat.grad
        last = l
    return dict(latent=lat.detach().numpy().copy(), target=np.asarray(target_latents), history=hist)


def fit_inertia_primitive(kind, target_dims, start_dims, torque_dirs, run_time=2.0, max_iter=200, lr=1e-2, conv_thresh=1e-5,
                          min_dim=0.5, max_dim=2.0, optimizer="Adam", log=None):
    """optim_primitives.py:160-240 for B (target, start) rows at once: Adam (or plain gradient descent) on the dimensions so
    that the final velocity under the torque matches the target's; dimensions clamped to [min_dim, max_dim] after each update;
    stops when no scene's loss moved by more than conv_thresh."""
    steps = int(math.ceil(run_time / Defaults3D.DT)) + 2
    tgt = torch.as_tensor(np.asarray(target_dims, np.float64)).reshape(-1, PRIMITIVES[kind])
    with torch.no_grad():
        wt = primitive_spin_world(kind, tgt, steps=steps)
        v_target = run_spin(wt, torque_dirs, run_time).clone()
        tgt_cloud = chamfer_hip.pack(wt.mesh_verts)
    dims = torch.tensor(np.asarray(start_dims, np.float64).reshape(-1, PRIMITIVES[kind]), requires_grad=True)
    opt = torch.optim.Adam([dims], lr=lr) if optimizer == "Adam" else torch.optim.SGD([dims], lr=lr)
    hist, last = [], None
    for e in range(max_iter):
        opt.zero_grad()
        w = primitive_spin_world(kind, dims, steps=steps)
        v = run_spin(w, torque_dirs, run_time)
        loss = ((v - v_target.to(v)) ** 2).sum(dim=1)
        loss.sum().backward()
        l = loss.detach().cpu().numpy()
        d = _chamfer_series(w.mesh_verts, tgt_cloud)
        hist.append(dict(iter=e, loss=l.copy(), dims=dims.detach().numpy().copy(), grad=dims.grad.numpy().copy(), chamfer=d))
        if log:
            log("iter %3d  mean loss %.3e  mean chamfer %.3e  mean |dims - target| %.4f" %
                (e, float(l.mean()), float(d.mean()), float((dims.detach() - tgt).abs().mean())))
        if last is not None and np.all(np.abs(last - l) < conv_thresh):
            break
        opt.step()
        with torch.no_grad():
            dims.clamp_(min_dim, max_dim)
        last = l
    return dict(dims=dims.detach().numpy().copy(), target=tgt.numpy(), history=hist)


# ---- system identification (experiments/system_identification/optim_sysid.py) --------------------------------------------
def push_world(latents, packed, force, mass, fric, run_steps, floor_dims=(20.0, 1.0, 20.0), restitution=0.0, g=10.0, res=128, device=None,
               mesh_cache=None):
    """optim_sysid.py:104-131 (`make_world`) for one scene per latent code: the floor and a neural-SDF body (scale 1) set down
    on it (2 eps above, by its mesh's lowest vertex), gravity, a constant push (force[:, 0] along x, force[:, 1] along z),
    strict_no_penetration=False, fric_dirs=8.  `force` [B,2], `mass` [B], `fric` [B] (both bodies, as in the experiment) are
    torch tensors and may require grad: the batch's parameters are built from them (inertia = mass x the mesh's unit inertia).
    `latents` [B, 2] or, with a `packed` of the shapenet shape, [B, 4]; a tensor that requires grad makes the scene
    differentiable w.r.t. it as bounce_world_latent's is (SDF queries, level-set mesh, inertia; the start pose is a constant)."""
    lat_t = latents if torch.is_tensor(latents) and latents.requires_grad else None
    latents = np.asarray(latents.detach().cpu() if torch.is_tensor(latents) else latents, np.float64)
    B, nb = latents.shape[0], 2
    spec, cache = scenes._base(B, nb), {}
    fd = np.asarray(floor_dims, np.float64)
    scenes._floor(spec, cache, fd, 0.0, restitution)
    spec["shape_aux"] = np.zeros((B, nb))
    spec["igr_net"] = packed
    spec["shape_type"][:, 1] = abi.SHAPE_IGR
    spec["shape_aux"][:, 1] = 1.0
    Iunit, vts = [], [torch.as_tensor(m[0], dtype=torch.float64) for m in spec["meshes"]]
    for s in range(B):
        key = tuple(latents[s])
        if lat_t is not None:
            v, f = meshsdf.igr_mesh(lat_t[s].to(torch.float64), packed, res=res)
            vts.append(v)
            ent = (v.detach().cpu().numpy(), f.cpu().numpy(), mass_properties.mesh_inertia_diff(v, f, torch.tensor(1.0, dtype=torch.float64)).cpu())
        elif mesh_cache is None or key not in mesh_cache:
            v, f = meshsdf.igr_mesh(torch.tensor(latents[s], dtype=torch.float64), packed, res=res)
            v = v.cpu().numpy(); f = f.cpu().numpy()
            ent = (v, f, np.asarray(mass_properties.mesh_inertia(v, f, 1.0).cpu()))
            if mesh_cache is not None:
                mesh_cache[key] = ent
        else:
            ent = mesh_cache[key]
        v, f, J = ent
        spec["meshes"].append((v, f)); spec["mesh_vgrad"].append(np.zeros_like(v))
        spec["mesh_id"][s, 1] = len(spec["meshes"]) - 1
        spec["pose"][s, 1, 4:] = (0.0, -v[:, 1].min() + 2 * Defaults3D.EPSILON, 0.0)
        Iunit.append(J)
    scenes.set_latents(spec, 1, latents, packed)      # ([B, 2] or, with the shapenet network, [B, 4])
    T = lambda x: torch.as_tensor(x, dtype=torch.float64)
    mass, fric, force = T(mass), T(fric), T(force)
    Iu = torch.stack(Iunit) if lat_t is not None else T(np.stack(Iunit))
    one = torch.ones(B, dtype=torch.float64)
    zero = torch.zeros(B, dtype=torch.float64)
    params = dict(
        mass=torch.stack([one, mass], 1),
        inertia=torch.stack([T(spec["inertia"][:, 0]), mass[:, None, None] * Iu], 1),
        fric=torch.stack([fric, fric], 1),
        fext=torch.stack([torch.zeros(B, 6, dtype=torch.float64), torch.stack([zero, zero, zero, force[:, 0], -g * mass, force[:, 1]], 1)], 1))
    for k in ("mass", "inertia", "fric", "fext"):
        spec[k] = params[k].detach().numpy()
    if lat_t is not None:
        key, width = ("igr_latent", abi.IGR_LATENT_MAX) if "igr_latent" in spec else ("shape_prm", 3)
        rows = torch.cat([lat_t.cpu().to(torch.float64), torch.zeros(B, width - latents.shape[1], dtype=torch.float64)], 1)
        params[key] = torch.stack([T(spec[key][:, 0]), rows], 1)
        params["verts"] = torch.cat([v.to(vts[-1].device) for v in vts])
    w = BatchWorld3D(spec, params=params, strict_no_penetration=False, max_substeps=4 * run_steps + 64, device=device,
                     maxc=256, max_cand=8192, max_pc=128)
    return w


def fit_sysid(goal, latents, packed, target, start, run_time=1.0, max_iter=100, lr=None, conv_thresh=1e-5, res=128, log=None):
    """optim_sysid.py:184-300 for B scenes at once: `goal` in ('mass', 'force', 'friction') is estimated by gradient descent
    on sum_t |pos_t - pos_t*|^2 of the pushed body, the other two quantities are the targets'.  `target` / `start`: dicts with
    force [B,2], mass [B], fric [B] (start: only the goal's entry is read).  Learning rates as in the experiment's named
    configs (:84-100)."""
    lr = {"mass": 1e-2, "friction": 1e-3, "force": 1e-1}[goal] if lr is None else lr
    steps = int(math.ceil(run_time / Defaults3D.DT - 1e-9))
    key = {"mass": "mass", "friction": "fric", "force": "force"}[goal]
    tv = {k: torch.as_tensor(np.asarray(target[k], np.float64)) for k in ("force", "mass", "fric")}
    cache = {}
    with torch.no_grad():
        wt = push_world(latents, packed, tv["force"], tv["mass"], tv["fric"], steps, res=res, mesh_cache=cache)
        pos_t = rollout(wt, steps)[0][:, :, 1, 4:].clone()
    x = torch.tensor(np.asarray(start[key], np.float64), requires_grad=True)
    hist, last = [], None
    for e in range(max_iter):
        if x.grad is not None:
            x.grad = None
        cur = dict(tv); cur[key] = x
        w = push_world(latents, packed, cur["force"], cur["mass"], cur["fric"], steps, res=res, mesh_cache=cache)
        pos = rollout(w, steps)[0][:, :, 1, 4:]
        loss = ((pos - pos_t.to(pos)) ** 2).sum(dim=(0, 2))
        loss.sum().backward()
        l = loss.detach().cpu().numpy()
        d = (x.detach() - tv[key]).reshape(len(l), -1).norm(dim=1).numpy()
        hist.append(dict(iter=e, loss=l.copy(), value=x.detach().numpy().copy(), grad=x.grad.numpy().copy(), dist=d.copy()))
        if log:
            log("[%s] iter %3d  mean loss %.3e  mean |x - x*| %.4f  |grad| %.3e" % (goal, e, float(l.mean()), float(d.mean()), float(x.grad.abs().mean())))
        if last is not None and np.all(np.abs(last - l) < conv_thresh):
            break
        with torch.no_grad():
            x -= lr * x.grad
        last = l
    return dict(goal=goal, value=x.detach().numpy().copy(), target=tv[key].numpy().copy(), start=np.asarray(start[key], np.float64), history=hist)


def export_trajectory(path, pose, vel, **meta):
    """(T, B, nb, 13) = pose (quaternion wxyz, position) | velocity (angular, linear), as the reference's
    world.trajectory entries (world.py:376-378), one array instead of a python list per scene."""
    np.savez_compressed(path, trajectory=torch.cat([pose, vel], dim=3).detach().cpu().numpy(), **meta)


def main(argv=None):
    ap = argparse.ArgumentParser(description="batched experiment drivers (trajectory_fitting/optim_sphere, inertia_fitting/optim_shapespace and optim_primitives, system_identification/optim_sysid)")
    ap.add_argument("what", choices=["sphere", "shapespace", "inertia", "primitives", "sysid", "pointcloud", "recorded", "depth"])
    ap.add_argument("--shape", default="sphere", choices=["sphere", "cube", "igr", "grid"],
                    help="pointcloud, depth, recorded: the fitted body (pointcloud and depth only: igr, a neural body of --net whose latent code is fitted; "
                         "grid, a voxel body of --res samples per axis whose samples are fitted to a sphere seen from three sides)")
    ap.add_argument("--res", type=int, default=33, help="pointcloud, depth --shape grid: samples per axis of the voxel body; depth --shape igr: of the neural body's value grid")
    ap.add_argument("--mesh", default=None, metavar="FILE.obj",
                    help="pointcloud --shape grid: fit the samples to this closed triangle mesh (SDFGrid3D.from_mesh) instead of a sphere")
    ap.add_argument("--file", default=None, help="recorded: the recording (real_world_data.pkl, or an .npz with its keys)")
    ap.add_argument("--synthetic", action="store_true", help="recorded: fit recordings made by synthesize_recording instead of --file")
    ap.add_argument("--optimizer", default="GD", choices=["GD", "Adam"])
    ap.add_argument("--observe", default="vertices", choices=["vertices", "depth"],
                    help="pointcloud: the target's mesh vertices that face the camera, or what the depth camera sees of it")
    ap.add_argument("--kind", default="box", choices=sorted(PRIMITIVES))
    ap.add_argument("--goal", default="mass", choices=["mass", "force", "friction"])
    ap.add_argument("--run-time", type=float, default=1.0)
    ap.add_argument("--scenes", type=int, default=None, help="default 64; recorded --synthetic: 2")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--net", default="bob_spot", choices=["bob_spot", "shapenet"],
                    help="shapespace, sysid, inertia, pointcloud --shape igr: the network shape (bob_spot: latent 2, 8 x 128; shapenet: latent 4, 8 x 256)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    synthetic_default = a.scenes is None
    a.scenes = 64 if a.scenes is None else a.scenes
    r = np.random.default_rng(a.seed)
    if a.what == "sphere":
        # RESULTS.md:14-47: radius error after fitting, target and start radii ~ U(0.4, 2.0) (optim_sphere.py:214-218)
        target, start = 0.4 + 1.6 * r.random(a.scenes), 0.4 + 1.6 * r.random(a.scenes)
        res = {}
        for name, kw in (("gravity, no toc", dict(use_toc_diff=False)), ("gravity, toc", dict(use_toc_diff=True)),
                         ("no gravity, toc", dict(use_toc_diff=True, use_gravity=False))):
            res[name] = fit_sphere_radius(target, start, max_iter=a.iters, log=lambda s, n=name: print("[%s] %s" % (n, s)), **kw)
        print(radius_error_table(res))
        if a.out:
            np.savez_compressed(a.out, **{k.replace(" ", "_").replace(",", ""): v["radius"] for k, v in res.items()}, target=target, start=start)
    elif a.what == "pointcloud" and a.shape == "igr":
        from . import igr
        width, nlat = igr.SHAPES[a.net == "shapenet"]
        packed = igr.pack_weights(*scenes.geometric_init_weights(a.seed, 0.5, width, nlat))
        tgt, st = 0.1 * r.standard_normal((a.scenes, nlat)), 0.1 * r.standard_normal((a.scenes, nlat))
        res = fit_pointcloud_latent(tgt, st, packed, run_time=a.run_time, max_iter=a.iters, log=print, observe=a.observe)
        for stage, h in res["history"].items():
            print("pointcloud igr [%s]: mean loss %.3e -> %.3e, %d scenes" % (stage, float(h[0]["loss"].mean()), float(h[-1]["loss"].mean()), a.scenes))
    elif a.what == "pointcloud" and a.shape == "grid":
        tgt = 0.5 + r.random(a.scenes); st = tgt + 0.1 + 0.4 * r.random(a.scenes)
        mesh = None
        if a.mesh:      # every scene fits the user's mesh, from start spheres of 0.8 .. 1.2 of its extent
            mesh = meshes.load_obj(a.mesh)
            st = np.abs(mesh[0] - mesh[0].mean(0)).max() * (0.8 + 0.4 * r.random(a.scenes))
        res = fit_pointcloud_grid("sphere", tgt, st, res=a.res, max_iter=a.iters, log=print, observe=a.observe, target_mesh=mesh)
        for s in range(a.scenes):
            print("pointcloud grid scene %d: loss %.3e -> %.3e, chamfer %.3e -> %.3e" %
                  (s, res["loss_start"][s], res["loss_final"][s], res["chamfer_start"][s], res["chamfer_final"][s]))
    elif a.what == "pointcloud":
        # optim_pointcloud.py:365-402: target half size ~ U(0.5, 1.5), start = target + U(0, 1); target pose = identity at
        # (0,5,0) perturbed by N(0, 0.1) in rotation and position, start pose = target pose perturbed the same way again
        tgt = 0.5 + r.random(a.scenes); st = tgt + r.random(a.scenes)
        def perturbed(base):
            q = base[:, :4] + 0.1 * r.standard_normal((a.scenes, 4))
            return np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), base[:, 4:] + 0.1 * r.standard_normal((a.scenes, 3))], 1)
        tp = perturbed(np.tile([1.0, 0, 0, 0, 0, 5.0, 0], (a.scenes, 1))); sp = perturbed(tp)
        res = fit_pointcloud(a.shape, tgt, st, tp, sp, run_time=a.run_time, max_iter=a.iters, optimizer=a.optimizer, noise=1e-4, log=print,
                             observe=a.observe)
        print("pointcloud %s: mean |rad - rad*| %.4f -> %.4f, mean |pos - pos*| %.4f -> %.4f, %d scenes" %
              (a.shape, np.abs(st - tgt).mean(), np.abs(res["rad"] - tgt).mean(), np.linalg.norm(sp[:, 4:] - tp[:, 4:], axis=1).mean(),
               np.linalg.norm(res["pose"][:, 4:] - tp[:, 4:], axis=1).mean(), a.scenes))
    elif a.what == "depth":
        # a first-frame fit to depth images through the differentiable depth camera (fit_depth): half sizes as in `pointcloud`
        if a.shape == "igr":      # the latent code of a neural body of --net, as `pointcloud --shape igr` draws it
            from . import igr
            width, nlat = igr.SHAPES[a.net == "shapenet"]
            packed = igr.pack_weights(*scenes.geometric_init_weights(a.seed, 0.5, width, nlat))
            tl, sl = 0.1 * r.standard_normal((a.scenes, nlat)), 0.1 * r.standard_normal((a.scenes, nlat))
            res = fit_depth("igr", res=a.res, max_iter=a.iters, optimizer="Adam", log=print, target_latents=tl, start_latents=sl, packed=packed)
            print("depth igr: mean |latent - target| %.4f -> %.4f" % (np.abs(sl - tl).mean(), np.abs(res["latent"] - tl).mean()))
        else:
            tgt = 0.5 + r.random(a.scenes); st = tgt + 0.1 + 0.4 * r.random(a.scenes)
            res = fit_depth(a.shape, tgt, st, res=a.res, max_iter=a.iters, optimizer="Adam" if a.shape == "grid" else a.optimizer, log=print)
        for s in range(a.scenes):
            print("depth %s scene %d: loss %.3e -> %.3e, chamfer %.3e -> %.3e" %
                  (a.shape, s, res["loss_start"][s], res["loss_final"][s], res["chamfer_start"][s], res["chamfer_final"][s]))
    elif a.what == "recorded":
        if a.shape in ("igr", "grid"):
            ap.error("recorded: --shape sphere or cube")
        if a.synthetic:
            n = 2 if synthetic_default else a.scenes
            recs = synthesize_recording(rad=0.08 + 0.04 * r.random(n), shape=a.shape, noise=1e-4, seed=a.seed)
        elif a.file:
            from . import recorded
            recs = [recorded.load_recording(a.file)]
        else:
            ap.error("recorded: give --file PATH or --synthetic")
        first, traj = fit_recorded(recs, shape=a.shape, max_iter=a.iters, optimizer=a.optimizer, log=print)
        print("%-6s %-10s %-10s %-10s %-12s %-12s %-9s %-9s" % ("scene", "start rad", "frame rad", "traj rad", "frame loss", "traj loss", "friction", "restit."))
        for s in range(len(recs)):
            print("%-6d %-10.5f %-10.5f %-10.5f %-12.3e %-12.3e %-9.4f %-9.4f" % (s, first["start_rad"][s], first["final_rad"][s], traj["final_rad"][s],
                                                                          first["final_loss"][s], traj["final_loss"][s], traj["friction"][s], traj["restitution"][s]))
        if a.synthetic:
            tr = np.array([rc["truth"]["rad"] for rc in recs])
            print("recorded %s: |rad - rad*| start mean %.5f -> first frame %.5f -> trajectory %.5f, %d recordings" %
                  (a.shape, np.abs(first["start_rad"] - tr).mean(), np.abs(first["final_rad"] - tr).mean(), np.abs(traj["final_rad"] - tr).mean(), len(recs)))
    elif a.what == "shapespace":
        from . import igr
        width, nlat = igr.SHAPES[a.net == "shapenet"]
        packed = igr.pack_weights(*scenes.geometric_init_weights(a.seed, 0.5, width, nlat))
        tgt, st = 0.1 * r.standard_normal((a.scenes, nlat)), 0.1 * r.standard_normal((a.scenes, nlat))
        res = fit_trajectory_latent(tgt, st, packed, run_time=a.run_time, max_iter=a.iters, log=print)
        print("shapespace: mean loss %.3e -> %.3e, %d scenes" % (float(res["history"][0]["loss"].mean()), float(res["history"][-1]["loss"].mean()), a.scenes))
    elif a.what == "primitives":
        # optim_primitives.py:160-175: target and start dimensions ~ U(0.5, 2.0), a random unit torque direction per scene
        n = PRIMITIVES[a.kind]
        tgt, st = 0.5 + 1.5 * r.random((a.scenes, n)), 0.5 + 1.5 * r.random((a.scenes, n))
        dirs = r.standard_normal((a.scenes, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        res = fit_inertia_primitive(a.kind, tgt, st, dirs, run_time=a.run_time if a.run_time != 1.0 else 2.0, max_iter=a.iters, log=print)
        d0, d1 = np.abs(st - tgt).mean(), np.abs(res["dims"] - tgt).mean()
        print("%s: mean |dims - target| %.4f -> %.4f, final mean loss %.3e, %d scenes" % (a.kind, d0, d1, float(res["history"][-1]["loss"].mean()), a.scenes))
    elif a.what == "sysid":
        # optim_sysid.py:184-220: a random latent, push, mass and friction per scene; the goal's start value is drawn anew
        from . import igr
        width, nlat = igr.SHAPES[a.net == "shapenet"]
        packed = igr.pack_weights(*scenes.geometric_init_weights(a.seed, 0.5, width, nlat))
        uni = lambda lo, hi, *sh: lo + (hi - lo) * r.random((a.scenes,) + sh)
        lat = 0.1 * r.standard_normal((a.scenes, nlat))
        target = dict(force=uni(2.0, 5.0, 2), mass=uni(0.9, 1.1), fric=uni(0.01, 0.25))
        start = dict(force=uni(2.0, 5.0, 2), mass=uni(0.9, 1.1), fric=uni(0.01, 0.25))
        res = fit_sysid(a.goal, lat, packed, target, start, run_time=a.run_time, max_iter=a.iters, log=print)
        d0, d1 = np.abs(res["start"] - res["target"]).reshape(a.scenes, -1).max(1), np.abs(res["value"] - res["target"]).reshape(a.scenes, -1).max(1)
        print("%s: |x - x*| start mean %.4f -> final mean %.4f (max %.4f), %d scenes" % (a.goal, d0.mean(), d1.mean(), d1.max(), a.scenes))
    else:
        # (the spin scene has no contacts, so it takes either network: the latent code acts through mesh and inertia only)
        from . import igr
        width, nlat = igr.SHAPES[a.net == "shapenet"]
        packed = igr.pack_weights(*scenes.geometric_init_weights(a.seed, 0.5, width, nlat))
        tgt, st = 0.1 * r.standard_normal((a.scenes, nlat)), 0.1 * r.standard_normal((a.scenes, nlat))
        dirs = r.standard_normal((a.scenes, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        fit_inertia_latent(tgt, st, dirs, packed, max_iter=a.iters, log=print)


if __name__ == "__main__":
    main()
