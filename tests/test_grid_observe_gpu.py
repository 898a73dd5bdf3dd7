"""GPU, end to end: level-set bodies observed by the depth camera and fitted to what it saw.

  * an SDFGrid3D torus above the floor is observed (depth_camera.observe(..., grids=)) at 80 x 60; every observed point is a hit
    bracketed to rounding (|field| ~ 1e-14), so SDFGrid3D.pointcloud_loss on the body's own points at the true pose is at most
    count x 1e-18 (|field| <= 1e-9 per point, five orders above what is expected); at the pose shifted by 0.1 along x the loss is
    at least 1e6 times that, and its position gradient has a positive inner product with the shift: moving back lowers it.
  * experiments.pointcloud_observations(observe='depth') on a one-scene world with a grid body returns points for it; the same
    bodies without the grid table are refused by the renderer, as before.
  * a neural SDF3D (the seeded synthetic 256-wide network of tests/test_igr_shapenet_gpu.py, res = 32) renders through
    depth_camera.body_grid: its segment is non-empty, every back-projected hit satisfies the grid's trilinear field to 1e-10, and
    the grid is igr.igr_values on the mesh's lattice, bit for bit."""
import numpy as np
import pytest
import torch

import depth_camera_ref as ref
import grid_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)
CAM = dict(fx=ref.SMALL["fx"], fy=ref.SMALL["fy"], cx=ref.SMALL["cx"], cy=ref.SMALL["cy"], size=(ref.SMALL["W"], ref.SMALL["H"]))
TORUS_POSE = np.concatenate([G._unit([0.83, 0.41, -0.23, 0.30]), [1.5, 3.2, 5.0]])


def test_torus_is_observed_and_its_own_points_fit_its_pose():
    from diffsdfsim_amd import depth_camera
    from diffsdfsim_amd.physics3d import SDFGrid3D
    grid, scale = G.torus_grid((33, 33, 33)), G.TORUS_SCALE
    pose = np.array([ref.FLOOR[0], TORUS_POSE])
    kind = np.array([[ref.BOX, G.GRID]], np.int32)
    prm = np.array([ref.FLOOR[2], [0.0, 0.0, 0.0, scale]])
    pts, off = depth_camera.observe(dev(pose[None]), kind, dev(prm[None]), 1, ref.experiment_camera(), grids=[grid], grid_id=[[-1, 0]], **CAM)
    n = int(off[-1])
    assert n > 50

    def loss_at(p):
        p = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        loss, count = SDFGrid3D(p, scale, grid).pointcloud_loss(pts)
        g, = torch.autograd.grad(loss, p)
        return float(loss), int(count), g.numpy()
    l0, c0, _ = loss_at(TORUS_POSE)
    shift = np.array([0.1, 0.0, 0.0])
    moved = TORUS_POSE.copy(); moved[4:] += shift
    l1, c1, g1 = loss_at(moved)
    print("%d points; loss at the true pose %.3e (count %d), shifted %.3e (count %d), grad . shift %.3e" % (n, l0, c0, l1, c1, g1[4:] @ shift))
    assert c0 == n and l0 <= n * 1e-18
    assert l1 >= 1e6 * max(l0, 1e-300) and l1 > 1e-6
    assert g1[4:] @ shift > 0


def _grid_world(grid, scale, pos):
    from diffsdfsim_amd import scenes
    from diffsdfsim_amd.physics3d import SDFGrid3D
    from diffsdfsim_amd.physics3d.world import BatchWorld3D
    body = SDFGrid3D(pos, scale, grid)
    spec, cache = scenes._base(1, 2), {}
    scenes._floor(spec, cache, (20.0, 1.0, 20.0), 0.25, 0.5)
    spec["mesh_id"][:, 1] = scenes._add_mesh(spec, cache, ("grid",), lambda: (body.verts_np, body.faces_np, np.zeros_like(body.verts_np)))
    spec["shape_type"][:, 1] = G.GRID
    spec["shape_aux"] = np.array([[0.0, scale]])
    spec["pose"][:, 1, 4:] = pos
    spec["inertia"][:, 1] = np.eye(3)
    spec["grids"], spec["grid_id"] = [grid], np.array([[-1, 0]], np.int32)
    return BatchWorld3D(spec, device=DEV)


def test_observations_of_a_world_with_a_grid_body():
    from diffsdfsim_amd import _lib, depth_camera, experiments as X
    grid = G.sphere_grid(24, (0.0, 0.0, 0.0), 0.6)
    world = _grid_world(grid, 1.5, (0.0, 4.0, 0.0))      # (at rest, no gravity: nothing touches it)
    obs = X.pointcloud_observations(world, X.camera_pose(), observe="depth", every=1, run_time=2.5 * world.dt)
    n = np.diff(obs["seg_off"])
    print("points per frame:", n)
    assert len(n) >= 3 and np.all(n > 500) and len(obs["pts"]) == obs["seg_off"][-1]
    r = np.linalg.norm(obs["pts"].cpu().numpy() - [0.0, 4.0, 0.0], axis=1)
    assert np.abs(r - 0.9).max() < 0.02      # (a 24^3 trilinear sphere: its surface within a few percent of a cell of 0.9)
    E = world.engine
    prm = torch.cat([E.arr["shape_prm"], E.arr["shape_aux"][..., None]], 2)
    with pytest.raises(_lib.HipLibraryError, match="boxes, spheres, cylinders and rounded boxes"):      # the path without the table
        depth_camera.render_depth(world.pose.detach(), E.arr["shape_type"], prm, X.camera_pose(), **CAM)


def test_neural_body_renders_through_the_grid_its_mesh_comes_from():
    from diffsdfsim_amd import depth_camera, igr, meshsdf
    from diffsdfsim_amd.physics3d import SDF3D
    from test_igr_shapenet_gpu import LATENT, weights
    net = igr.IgrNet(*weights())
    lat = torch.tensor(LATENT, dtype=torch.float64)
    body = SDF3D([0, 0, 0], 1.0, igr.decode_igr(net), [lat], res=32)
    grid, scale = depth_camera.body_grid(body)
    assert tuple(grid.shape) == (32, 32, 32) and scale == 1.0
    want = igr.igr_values(meshsdf._grid_cached(32, grid.device), lat.to(grid.device), net.packed).reshape(32, 32, 32)
    assert torch.equal(grid, want)
    scale = 2.0      # (seen larger: the unit body covers few pixels at 80 x 60)
    pose = np.array([ref.FLOOR[0], [1.0, 0, 0, 0, 1.0, 3.0, 5.0]])
    kind = np.array([[ref.BOX, G.IGR]], np.int32)
    prm = np.array([ref.FLOOR[2], [0.0, 0.0, 0.0, scale]])
    cam = ref.experiment_camera()
    depth, seg = depth_camera.render_depth(dev(pose[None]), kind, dev(prm[None]), cam, grids=[grid], grid_id=[[-1, 0]], **CAM)
    depth, seg = depth[0].cpu().numpy(), seg[0].cpu().numpy()
    m = seg == 1
    f = ref.SMALL
    world = ref.backproject(depth, cam, f["fx"], f["fy"], f["cx"], f["cy"])
    phi = np.abs(G.field(grid.cpu().numpy(), scale, world[m] - pose[1, 4:]))
    print("%d pixels of the neural body, |field| <= %.2e" % (int(m.sum()), phi.max() if m.any() else 0.0))
    assert m.sum() > 20 and phi.max() <= 1e-10 and (seg != -2).all()
