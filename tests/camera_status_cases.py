"""The status that each camera entry returns for a scene it refuses, case by case, and the order in which the refusals win; shared by
tests/test_emu_camera_statuses.py (through the emulator) and tests/test_camera_statuses_gpu.py (on the device).

R, RG, S and A are dss_depth_render, dss_depth_render_grids, dss_shade_render and dss_depth_adjoint.  The scene is the smallest that
reaches every branch: the first two views of depth_camera_ref.bounce_views (floor, wall, one object) at 16 x 16 pixels beside a pooled
table of one 5 x 5 x 5 sphere grid that no body uses (every grid id is -1).  A case changes one body of view 1 (the order cases two),
the table or a size; every output and the adjoint's workspace hold FILL before the call and, after a refusal, still do: a refused call
returns before anything is enqueued.  The two point-cloud entries that take a table follow, on one segment of five points.

A test module supplies `run(name, args, outs)`: call entry `name` with `args` (numpy arrays stand for device arrays, a Host for memory
that stays on the host, the stream is the backend's own) and leave the device's values of the arrays `outs` in them; and `lib()`,
the bound library, for the workspace sizes."""
import numpy as np

import depth_camera_ref as ref
import grid_ref as G

FILL = -7
OK, BADARG, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3
W = H = 16
K = (12.875, 12.875, 7.5, 7.5)      # depth_camera_ref.SMALL at a fifth of its size
ENTRIES = {"R": "dss_depth_render", "RG": "dss_depth_render_grids", "S": "dss_shade_render", "A": "dss_depth_adjoint"}


class Host:
    """An argument the entry reads on the host (dss_shade_render's background)."""

    def __init__(self, a):
        self.a = a


def _filled(shape, dtype=np.float64):
    return np.full(shape, FILL, np.int64).astype(dtype)      # (uint8: 249)


# name, what changes (see arguments()), the status of R, RG, S, A (None: the case does not exist for that entry)
CAMERA_CASES = [
    ("brick", dict(kind={2: 4}), (-3, -3, -3, -3)),
    ("bowl", dict(kind={2: 5}), (-3, -3, -3, -3)),
    ("neural body, no table", dict(kind={2: 6}, table=False), (-3, None, -3, -3)),
    ("grid body, no table", dict(kind={2: 7}, table=False), (-3, None, -3, -3)),
    ("neural body, id -1", dict(kind={2: 6}), (None, -3, -3, -3)),
    ("grid body, id -1", dict(kind={2: 7}), (None, -3, -3, -3)),
    ("grid body, id == ngrid", dict(kind={2: 7}, ids={2: 1}), (None, -1, -1, -1)),
    ("grid body, id 0, ngrid 0, grid_id not NULL", dict(kind={2: 7}, ids={2: 0}, ngrid=0), (None, -1, -3, -3)),
    ("a dim of 1, no body uses the grid", dict(dim1=True), (None, -1, -1, -1)),
    ("brick below a bad id", dict(kind={0: 4, 2: 7}, ids={2: 1}), (None, -3, -3, -3)),
    ("bad id below a brick", dict(kind={0: 7, 2: 4}, ids={0: 1}), (None, -1, -1, -1)),
    ("a dim of 1 and a brick", dict(kind={2: 4}, dim1=True), (None, -1, -1, -1)),
    ("nine bodies", dict(nbody=9), (-3, -3, -3, -3)),
    ("workspace 8 bytes short", dict(ws_short=8), (None, None, None, -2)),
    ("workspace short and a brick", dict(kind={2: 4}, ws_short=8), (None, None, None, -2)),
    ("box with id == ngrid", dict(ids={0: 1}), (None, 0, 0, 0)),
]
CAMERA_IDS = [(e, name) for name, _, codes in CAMERA_CASES for e, c in zip("R RG S A".split(), codes) if c is not None]
_CACHE = {}


def _scene(nbody):
    pose, kind, prm = (a[:2] for a in ref.bounce_views(3))
    if nbody != 3:      # (the floor, nbody times: such a scene is refused by its size)
        pose, kind, prm = (np.repeat(a[:, :1], nbody, 1) for a in (pose, kind, prm))
    return pose.copy(), kind.copy(), prm.copy()


def _images(run):
    """depth and seg of the unchanged scene, from the backend's dss_depth_render: what S and A take as input."""
    if "images" not in _CACHE:
        a, outs = arguments("R", run)
        assert run(ENTRIES["R"], a, outs) == OK
        _CACHE["images"] = tuple(o.copy() for o in outs)
    return _CACHE["images"]


def arguments(entry, run, lib=None, kind=None, ids=None, table=True, ngrid=None, dim1=False, nbody=3, ws_short=0):
    """-> (the entry's argument list without the stream, its output arrays).  kind / ids: {body of view 1: value}; table=False: no
    grid arguments at all (ngrid 0, every pointer NULL); ngrid: passed in place of 1, with the table's pointers NULL when it is 0;
    dim1: the grid's middle dim reads 1; ws_short: bytes that workspace_bytes understates."""
    pose, types, prm = _scene(nbody)
    gid = np.full((2, nbody), -1, np.int32)
    for b, t in (kind or {}).items():
        types[1, b] = t
    for b, i in (ids or {}).items():
        gid[1, b] = i
    off, dims, data, blk_off, nblk = G.pooled([G.sphere_grid(n=5)])
    bmin = G.block_min(G.sphere_grid(n=5))
    if dim1:
        dims = dims.copy(); dims[0, 1] = 1
    ng = 1 if ngrid is None else ngrid
    if not table:
        gargs = [None, 0, None, None, None, None, None]
    elif ng == 0:
        gargs = [gid, 0, None, None, None, None, None]
    else:
        gargs = [gid, ng, off, dims, data, blk_off, bmin]
    cam = np.ascontiguousarray(ref.experiment_camera())
    head = [2, nbody, pose, types, prm, cam, *K, W, H]
    if entry in ("R", "RG"):
        outs = [_filled((2, H, W)), _filled((2, H, W), np.int32)]
        return head + [0.1, 100.0] + (gargs if entry == "RG" else []) + outs, outs
    depth, seg = _images(run)
    if entry == "S":
        outs = [_filled((2, H, W, 3)), _filled((2, H, W)), _filled((2, H, W, 3), np.uint8), _filled((2, H, W), np.uint8)]
        light = np.array([[0.3, 0.8, 0.5, 0.9]])
        return head + [100.0] + gargs + [depth, seg, np.full((2, nbody, 3), 0.5), 1, light, 0.1, Host(np.ones(3)), 1, 1e-3] + outs, outs
    nbytes = lib().dss_depth_adjoint_workspace_bytes(2, 3, W, H)      # (of the three-body scene: nine bodies have no size)
    assert nbytes == 2 * 3 * 11 * 8
    outs = [_filled((2, nbody, 7)), _filled((2, nbody, 3)), _filled(data.shape), _filled((2, nbody), np.int32), _filled(nbytes // 8)]
    g_pose, g_prm, g_grid, dropped, ws = outs
    return head + [depth, seg, np.ones((2, H, W)), 1e-3] + gargs[:5] + [g_pose, g_prm, g_grid, dropped, ws, nbytes - ws_short], outs


def check_camera(run, lib, entry, name):
    change, codes = next((c, k) for n, c, k in CAMERA_CASES if n == name)
    want = codes["R RG S A".split().index(entry)]
    args, outs = arguments(entry, run, lib, **change)
    rc = run(ENTRIES[entry], args, outs)
    print("%s, %s: status %d, expected %d" % (ENTRIES[entry], name, rc, want))
    assert rc == want
    if want != OK:
        assert all((o == _filled((), o.dtype)).all() for o in outs), "a refused call wrote an output"
        return
    # an analytic body's id is not judged: the bits of the same call with id -1
    args2, outs2 = arguments(entry, run, lib, **dict(change, ids=None))
    assert run(ENTRIES[entry], args2, outs2) == OK
    written = outs[:2] + outs[3:4] if entry == "A" else outs      # (A: g_grid is added into and the workspace is scratch)
    assert all(np.array_equal(a, b) for a, b in zip(written, outs2[:2] + outs2[3:4] if entry == "A" else outs2))
    assert all((o != _filled((), o.dtype)).any() for o in written), "an accepted call left an output at its fill"
    if entry == "A":
        assert (outs[2] == FILL).all(), "no body uses the grid"


# ---- the point-cloud entries that take a table: one segment of five points ---------------------------------------------------------------
POINTCLOUD_CASES = [
    ("neural segment", dict(kind=6, gid=0), -3),
    ("grid segment, id -1", dict(kind=7, gid=-1), -3),
    ("grid segment, id == ngrid", dict(kind=7, gid=1), -1),
    ("a dim of 1", dict(kind=0, gid=-1, dim1=True), -1),
    ("bowl", dict(kind=5, gid=-1), 0),
]
POINTCLOUD_IDS = [(e, name) for name, _, _ in POINTCLOUD_CASES for e in ("dss_pointcloud_loss_grids", "dss_pointcloud_loss_grids_adjoint")]


def check_pointcloud(run, lib, entry, name):
    change, want = next((c, k) for n, c, k in POINTCLOUD_CASES if n == name)
    pts = np.random.default_rng(5).uniform(-0.4, 0.4, (5, 3))
    seg_off = np.array([0, 5], np.int32)
    pose, prm = np.array([[1.0, 0, 0, 0, 0, 0, 0]]), np.array([[1.0, 0.3, 0.0, 1.0]])
    types, gid = np.array([change["kind"]], np.int32), np.array([change["gid"]], np.int32)
    off, dims, data, _, _ = G.pooled([G.sphere_grid(n=5)])
    if change.get("dim1"):
        dims = dims.copy(); dims[0, 1] = 1
    head = [1, 5, seg_off, pts, pose, types, prm, gid, 1, off, dims, data]
    if entry == "dss_pointcloud_loss_grids":
        nbytes = lib().dss_pointcloud_loss_workspace_bytes(1, 5)
        outs = [_filled(12), _filled(nbytes // 8)]
        rc = run(entry, head + outs + [nbytes], outs)
    else:
        outs = [_filled(data.shape)]
        rc = run(entry, head + [np.ones(1)] + outs, outs)
    print("%s, %s: status %d, expected %d" % (entry, name, rc, want))
    assert rc == want
    if want != OK:
        assert all((o == FILL).all() for o in outs), "a refused call wrote an output"
    elif entry == "dss_pointcloud_loss_grids":
        assert (outs[0] != FILL).all()
    else:
        assert (outs[0] == FILL).all()      # (an analytic segment adds nothing)
