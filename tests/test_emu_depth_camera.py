"""CPU: csrc/depth_camera.hip through the emulator (the kernels, their launch shapes, the LDS body table, ballots and prefix
popcounts as on the device) against the float64 oracle of tests/depth_camera_ref.py and the reference's own selection
(tests/golden/depth_camera_points.npz, tools/gen_depth_camera_golden.py).

Tolerances, all derived: the four fields are convex along a ray and the trace never passes the surface, so a hit at cosine c
lies within tau / c = 2e-9 (tau = 1e-10, c >= 0.05) before the true one, plus rounding of order 1e-12 at depth 30: depth to 1e-8;
the back-projected hit has |phi| <= tau + rounding: 1e-9; hit / miss / body equal the oracle's except at the pixels the oracle
marks delicate, which may be at most 1 % of a view, and no pixel may use up the iteration cap.  Back-projection is about ten
operations at magnitudes <= 50: points to 1e-12, order and counts exact.  The reference forms nx, ny in float32 (6e-8 relative),
which at depth <= 30 moves a point by < 5e-6: points of the golden to 5e-6, mask, order and count exact."""
import os

import numpy as np
import pytest
import scipy.ndimage

import depth_camera_ref as ref
from emu import emu

G = os.path.join(os.path.dirname(__file__), "golden", "depth_camera_points.npz")
_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)


def render(pose, kind, prm, cam, fx, fy, cx, cy, W, H, znear=0.1, zfar=100.0, fill=None):
    L = emu.lib()
    pose, kind, prm, cam = _c(pose), _c(kind, np.int32), _c(prm), _c(cam)
    nview, nbody = kind.shape
    depth = np.zeros((nview, H, W)) if fill is None else np.full((nview, H, W), float(fill))
    seg = np.full((nview, H, W), -1 if fill is None else int(fill), np.int32)
    rc = L.dss_depth_render(nview, nbody, pose.ctypes.data, kind.ctypes.data, prm.ctypes.data, cam.ctypes.data, fx, fy, cx, cy, W, H,
                            znear, zfar, depth.ctypes.data, seg.ctypes.data, None)
    return rc, depth, seg


def points(depth, seg, body, cam, fx, fy, cx, cy):
    L = emu.lib()
    depth, seg, cam = _c(depth), _c(seg, np.int32), _c(cam)
    nview, H, W = depth.shape
    rows = np.full(nview * H, -5, np.int32)
    assert L.dss_depth_points_count(nview, H, W, body, depth.ctypes.data, seg.ctypes.data, rows.ctypes.data, None) == 0
    off = _c(np.cumsum(rows) - rows, np.int32)
    n = int(rows.sum())
    pts = np.full((n + 1, 3), 7.5)      # (one row more: nothing may be written past the last point)
    assert L.dss_depth_points_emit(nview, H, W, body, depth.ctypes.data, seg.ctypes.data, off.ctypes.data, cam.ctypes.data, fx, fy, cx, cy,
                                   pts.ctypes.data, None) == 0
    assert np.all(pts[n] == 7.5)
    return pts[:n], np.concatenate([[0], np.cumsum(rows.reshape(nview, H).sum(1))])


@pytest.fixture(scope="module")
def views():
    pose, kind, prm = ref.bounce_views()
    cam = ref.experiment_camera()
    rc, depth, seg = render(pose, kind, prm, cam, **ref.SMALL)
    assert rc == 0
    return pose, kind, prm, cam, depth, seg


@pytest.mark.parametrize("v", range(4))
def test_rendered_view_matches_the_oracle(views, v):
    pose, kind, prm, cam, depth, seg = views
    want = ref.render(pose[v], kind[v], prm[v], cam, **ref.SMALL)
    assert (want["seg"] == 2).sum() > 10, "the object is hardly in view"
    ref.check_view(depth[v], seg[v], want, pose[v], kind[v], prm[v], cam, name="view %d" % v, **ref.SMALL)


def test_object_behind_the_wall_is_not_seen(views):
    pose, kind, prm, cam, depth, seg = views
    assert not (seg[4] == 2).any() and (seg[4] == 1).any() and (seg[4] != -2).all()
    alone = render(pose[4:, 2:], kind[4:, 2:], prm[4:, 2:], cam, **ref.SMALL)[2]      # (without floor and wall it is in view)
    assert (alone[0] == 0).sum() > 3


def test_two_calls_return_the_same_bits(views):
    pose, kind, prm, cam, depth, seg = views
    rc, d2, s2 = render(pose[:2], kind[:2], prm[:2], cam, **ref.SMALL)
    assert rc == 0 and np.array_equal(d2, depth[:2]) and np.array_equal(s2, seg[:2])


def test_closed_forms_of_the_oracle_agree_with_its_generic_path():
    pose, kind, prm = ref.bounce_views()
    o, d, L = ref.rays(ref.experiment_camera(), **ref.SMALL)
    for v, j in ((0, 2), (3, 2), (0, 1)):      # the sphere, the tilted box, the wall
        t, cos, _ = ref.body_hits(int(kind[v, j]), prm[v, j], pose[v, j], o, d, L)
        R = ref.quat_to_mat(pose[v, j, :4])
        tmin, fmin = ref._ray_min(int(kind[v, j]), prm[v, j], R.T @ (o - pose[v, j, 4:]), d @ R, 100.0)
        sure = np.abs(fmin) > 1e-6
        assert np.array_equal(np.isfinite(t)[sure], (fmin < 0)[sure])
        hit = np.isfinite(t)
        pb = (o + t[hit][:, None] * d[hit] - pose[v, j, 4:]) @ R
        assert np.abs(ref.sdf(int(kind[v, j]), prm[v, j], pb)).max() < 1e-12


@pytest.mark.parametrize("kind", [4, 5, 6, 7])
def test_unsupported_types_give_a_status_and_leave_the_outputs_alone(kind):
    pose, types, prm = ref.bounce_views()
    types = types[:2].copy(); types[1, 2] = kind
    rc, depth, seg = render(pose[:2], types, prm[:2], ref.experiment_camera(), fill=-7, **ref.SMALL)
    assert rc == -3 and np.all(depth == -7.0) and np.all(seg == -7)      # DSS_E_UNSUPPORTED


def test_points_of_the_reference_golden():
    g = np.load(G)
    fx, fy, cx, cy = g["intrinsics"]
    for k in range(3):      # each input has its own camera
        pts, off = points(g["depth"][k:k + 1], g["seg"][k:k + 1], int(g["body"]), g["cam"][k], fx, fy, cx, cy)
        want = g["pts"][g["seg_off"][k]:g["seg_off"][k + 1]]
        assert len(pts) == len(want) and off[-1] == len(want)
        assert len(want) == 0 or np.abs(pts - want).max() < 5e-6
        mine, _ = ref.observed_points(g["depth"][k:k + 1], g["seg"][k:k + 1], int(g["body"]), g["cam"][k], fx, fy, cx, cy)
        assert len(mine) == len(pts) and (len(pts) == 0 or np.abs(pts - mine).max() < 1e-12)


def _synthetic(r, nview, H, W, kind):
    depth = r.uniform(5.0, 30.0, (nview, H, W))
    if kind == "full":
        seg = np.full((nview, H, W), 2)
    elif kind == "empty":
        seg = r.integers(-1, 2, (nview, H, W))
    else:      # blobs that touch the border, thin lines, holes of depth 0, other bodies' pixels
        seg = np.where(scipy.ndimage.binary_dilation(r.random((nview, H, W)) < 0.25), 2, r.integers(-2, 2, (nview, H, W)))
        seg[:, :, :3] = 2; seg[:, 0] = 2
        depth[r.random((nview, H, W)) < 0.1] = 0.0
    return depth, seg.astype(np.int32)


@pytest.mark.parametrize("W,H,kind", [(67, 5, "border"), (80, 5, "border"), (67, 5, "full"), (80, 60, "full"), (67, 5, "empty"),
                                      (130, 7, "border"), (3, 3, "full"), (2, 9, "full")])
def test_points_of_synthetic_masks(W, H, kind):
    r = np.random.default_rng(W * 100 + H)
    depth, seg = _synthetic(r, 3, H, W, kind)
    seg[1] = 0      # an empty view in the middle
    cam = ref.experiment_camera()
    pts, off = points(depth, seg, 2, cam, 64.375, 64.375, (W - 1) / 2, (H - 1) / 2)
    want, woff = ref.observed_points(depth, seg, 2, cam, 64.375, 64.375, (W - 1) / 2, (H - 1) / 2)
    assert np.array_equal(off, woff) and off[1] == off[2]
    assert kind == "empty" or W < 4 or off[-1] > 0
    assert len(pts) == len(want) and (len(want) == 0 or np.abs(pts - want).max() < 1e-12)
