"""GPU: voxel-grid bodies in the depth camera (depth_camera.render_depth(..., grids=) over dss_depth_render_grids and
dss_grid_block_min) against the numpy oracle of tests/grid_ref.py.  Scene, checks and tolerances are those of
tests/test_emu_depth_grid.py (derived there): 80 x 60, floor, wall, the 33 x 25 x 21 torus and a fourth body from a pool of two
grids; outside the oracle's delicate pixels (at most 1 % of a view) seg equals the oracle's, a grid hit's depth to 1e-10 and the
field at its back-projected hit to 1e-10, analytic bodies to the analytic camera's 1e-8 / 1e-9, no seg = -2."""
import numpy as np
import pytest
import torch

import depth_camera_ref as ref
import grid_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def render(pose, kind, prm, grids, gid, cam, fx, fy, cx, cy, W, H):
    from diffsdfsim_amd import depth_camera
    return depth_camera.render_depth(dev(pose), dev(kind, torch.int32), dev(prm), cam, fx, fy, cx, cy, size=(W, H), grids=grids, grid_id=gid)


@pytest.fixture(scope="module")
def views():
    from diffsdfsim_amd.grids import GridTable
    pose, kind, prm, grids, gid = G.grid_views()
    cam = ref.experiment_camera()
    table = GridTable(grids, DEV)
    depth, seg = render(pose, kind, prm, table, gid, cam, **ref.SMALL)
    return pose, kind, prm, grids, gid, cam, table, depth, seg


@pytest.mark.parametrize("v", range(3))
def test_rendered_view_matches_the_oracle(views, v):
    pose, kind, prm, grids, gid, cam, table, depth, seg = views
    want = G.render(pose[v], kind[v], prm[v], grids, gid[v], cam, **ref.SMALL)
    assert (want["seg"] == 2).sum() > 30 and (want["seg"] == 3).sum() > 10, "a body is hardly in view"
    G.check_view(depth[v].cpu().numpy(), seg[v].cpu().numpy(), want, pose[v], kind[v], prm[v], grids, gid[v], cam, name="view %d" % v, **ref.SMALL)


def test_the_wall_hides_part_of_the_torus_and_calls_repeat(views):
    pose, kind, prm, grids, gid, cam, table, depth, seg = views
    alone = render(pose[1:2, 2:3], kind[1:2, 2:3], prm[1:2, 2:3], table, gid[1:2, 2:3], cam, **ref.SMALL)[1]
    assert 0 < int((seg[1] == 2).sum()) < int((alone[0] == 0).sum())
    d2, s2 = render(pose, kind, prm, table, gid, cam, **ref.SMALL)
    assert torch.equal(d2, depth) and torch.equal(s2, seg) and bool((seg != -2).all())
    d3, s3 = render(pose, kind, prm, grids, gid, cam, **ref.SMALL)      # (a list of arrays makes its own table)
    assert torch.equal(d3, depth) and torch.equal(s3, seg)


def test_views_without_a_grid_body_are_the_analytic_renderers_bits(views):
    from diffsdfsim_amd import depth_camera
    table = views[6]
    pose, kind, prm = ref.bounce_views()
    cam = ref.experiment_camera()
    f = ref.SMALL
    d0, s0 = depth_camera.render_depth(dev(pose), dev(kind, torch.int32), dev(prm), cam, f["fx"], f["fy"], f["cx"], f["cy"], size=(f["W"], f["H"]))
    d1, s1 = render(pose, kind, prm, table, np.full(kind.shape, -1), cam, **f)
    assert torch.equal(d0, d1) and torch.equal(s0, s1) and bool((s0 >= 0).any())


@pytest.mark.parametrize("kind,gid", [(7, -1), (6, -1), (4, -1), (5, -1)])
def test_refused_inputs_raise_and_leave_the_outputs_alone(views, kind, gid):
    from diffsdfsim_amd import _lib
    pose, types, prm, grids, ids, cam, T = views[:7]
    types, ids = types.copy(), ids.copy()
    types[1, 3], ids[1, 3] = kind, gid
    with pytest.raises(_lib.HipLibraryError, match="grid and neural bodies"):
        render(pose, types, prm, T, ids, cam, **ref.SMALL)
    depth = torch.full((3, 60, 80), -7.0, dtype=torch.float64, device=DEV)
    seg = torch.full((3, 60, 80), -7, dtype=torch.int32, device=DEV)
    p, t, q, c, i = dev(pose), dev(types, torch.int32), dev(prm), dev(cam), dev(ids, torch.int32)
    rc = _lib.lib().dss_depth_render_grids(3, 4, _lib.ptr(p), _lib.ptr(t), _lib.ptr(q), _lib.ptr(c), 64.375, 64.375, 39.5, 29.5, 80, 60, 0.1, 100.0,
                                           _lib.ptr(i), T.ngrid, _lib.ptr(T.off), _lib.ptr(T.dims), _lib.ptr(T.data), _lib.ptr(T.blk_off),
                                           _lib.ptr(T.block_min()), _lib.ptr(depth), _lib.ptr(seg), _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == -3 and bool((depth == -7.0).all()) and bool((seg == -7).all())


def test_block_minima_equal_numpy(views):
    grids, table = views[3], views[6]
    want = np.concatenate([G.block_min(g) for g in grids])
    assert table.nblk == len(want) == 8 * 6 * 5 + 27 and np.array_equal(table.block_min().cpu().numpy(), want)
