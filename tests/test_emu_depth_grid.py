"""CPU: voxel-grid bodies in the depth camera (dss_depth_render_grids, dss_grid_block_min of csrc/depth_camera.hip) through the
emulator, against the numpy oracle of tests/grid_ref.py.  Floor, wall, a torus sampled on 33 x 25 x 21 (non-cubic, non-convex:
rays through the hole approach, leave and approach again) and a fourth body from a pool of two grids, at 80 x 60.

Tolerances (outside the oracle's delicate pixels, at most 1 % of a view): hit / miss / body equal the oracle's.  A grid hit is
bracketed down to rounding: the trilinear value and the ray point at t <= 30 round at about 1e-14 in world units, divided by a
slope >= 0.05 that is 3e-13; |depth - oracle| <= 1e-10 and |field| <= 1e-10 at the back-projected hit leave room for another
evaluation order.  Analytic bodies of the same views keep the analytic camera's bounds (1e-8 in depth, 1e-9 on the surface).
No grid trace has an iteration cap: no seg = -2."""
import numpy as np
import pytest

import depth_camera_ref as ref
import grid_ref as G
from emu import emu

_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)


def block_min(grids):
    L = emu.lib()
    off, dims, data, blk_off, nblk = G.pooled(grids)
    out = np.full(nblk + 1, -3.0)      # (one more: nothing may be written past the last block)
    assert L.dss_grid_block_min(len(grids), off.ctypes.data, dims.ctypes.data, data.ctypes.data, blk_off.ctypes.data, nblk, out.ctypes.data, None) == 0
    assert out[nblk] == -3.0
    return out[:nblk]


def render(pose, kind, prm, grids, gid, cam, fx, fy, cx, cy, W, H, znear=0.1, zfar=100.0, fill=None):
    L = emu.lib()
    pose, kind, prm, cam, gid = _c(pose), _c(kind, np.int32), _c(prm), _c(cam), _c(gid, np.int32)
    off, dims, data, blk_off, nblk = G.pooled(grids)
    bmin = _c(block_min(grids))
    nview, nbody = kind.shape
    depth = np.zeros((nview, H, W)) if fill is None else np.full((nview, H, W), float(fill))
    seg = np.full((nview, H, W), -1 if fill is None else int(fill), np.int32)
    rc = L.dss_depth_render_grids(nview, nbody, pose.ctypes.data, kind.ctypes.data, prm.ctypes.data, cam.ctypes.data, fx, fy, cx, cy, W, H,
                                  znear, zfar, gid.ctypes.data, len(grids), off.ctypes.data, dims.ctypes.data, data.ctypes.data,
                                  blk_off.ctypes.data, bmin.ctypes.data, depth.ctypes.data, seg.ctypes.data, None)
    return rc, depth, seg


@pytest.fixture(scope="module")
def views():
    pose, kind, prm, grids, gid = G.grid_views()
    cam = ref.experiment_camera()
    rc, depth, seg = render(pose, kind, prm, grids, gid, cam, **ref.SMALL)
    assert rc == 0
    want = [G.render(pose[v], kind[v], prm[v], grids, gid[v], cam, **ref.SMALL) for v in range(len(pose))]
    return pose, kind, prm, grids, gid, cam, depth, seg, want


@pytest.mark.parametrize("v", range(3))
def test_rendered_view_matches_the_oracle(views, v):
    pose, kind, prm, grids, gid, cam, depth, seg, want = views
    assert (want[v]["seg"] == 2).sum() > 30 and (want[v]["seg"] == 3).sum() > 10, "a body is hardly in view"
    G.check_view(depth[v], seg[v], want[v], pose[v], kind[v], prm[v], grids, gid[v], cam, name="view %d" % v, **ref.SMALL)


def test_the_wall_hides_part_of_the_torus(views):
    pose, kind, prm, grids, gid, cam, depth, seg, want = views
    alone = render(pose[1:2, 2:3], kind[1:2, 2:3], prm[1:2, 2:3], grids, gid[1:2, 2:3], cam, **ref.SMALL)[2]
    seen, whole = int((seg[1] == 2).sum()), int((alone[0] == 0).sum())
    print("torus pixels: %d seen, %d without the wall" % (seen, whole))
    assert 0 < seen < whole


def test_firm_hits_of_the_torus_start_outside_it(views):
    # the hit rule's first case (entry value <= 0) does not decide these views: every firm hit is a sign change inside the grid
    pose, kind, prm, grids, gid, cam, depth, seg, want = views
    firm = (want[0]["seg"] == 2) & ~want[0]["delicate"]
    assert firm.sum() > 30 and np.all(want[0]["entry"][2][firm] > 0)


def test_two_calls_return_the_same_bits(views):
    pose, kind, prm, grids, gid, cam, depth, seg, want = views
    rc, d2, s2 = render(pose, kind, prm, grids, gid, cam, **ref.SMALL)
    assert rc == 0 and np.array_equal(d2, depth) and np.array_equal(s2, seg)


def test_views_without_a_grid_body_are_the_analytic_renderers_bits():
    pose, kind, prm = ref.bounce_views()
    cam = ref.experiment_camera()
    grids = G.grid_views()[3]
    L = emu.lib()
    p, k, q, c = _c(pose), _c(kind, np.int32), _c(prm), _c(cam)
    d0 = np.zeros((5, 60, 80)); s0 = np.full((5, 60, 80), -1, np.int32)
    assert L.dss_depth_render(5, 3, p.ctypes.data, k.ctypes.data, q.ctypes.data, c.ctypes.data, 64.375, 64.375, 39.5, 29.5, 80, 60, 0.1, 100.0,
                              d0.ctypes.data, s0.ctypes.data, None) == 0
    rc, d1, s1 = render(pose, kind, prm, grids, np.full(kind.shape, -1), cam, **ref.SMALL)
    assert rc == 0 and np.array_equal(d0, d1) and np.array_equal(s0, s1) and (s0 >= 0).any()


@pytest.mark.parametrize("kind,gid", [(7, -1), (6, -1), (4, -1), (5, -1), (4, 0)])
def test_refused_inputs_give_a_status_and_leave_the_outputs_alone(kind, gid):
    pose, types, prm, grids, ids = G.grid_views()
    types, ids = types.copy(), ids.copy()
    types[1, 3], ids[1, 3] = kind, gid
    rc, depth, seg = render(pose, types, prm, grids, ids, ref.experiment_camera(), fill=-7, **ref.SMALL)
    assert rc == -3 and np.all(depth == -7.0) and np.all(seg == -7)      # DSS_E_UNSUPPORTED


def test_block_minima_equal_numpy():
    grids = G.grid_views()[3]
    got = block_min(grids)
    want = np.concatenate([G.block_min(g) for g in grids])
    assert len(want) == 8 * 6 * 5 + 3 * 3 * 3 and np.array_equal(got, want)
    assert (want > 0).any() and (want <= 0).any()
