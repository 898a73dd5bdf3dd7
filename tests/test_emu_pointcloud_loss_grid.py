"""CPU: dss_pointcloud_loss_grids (csrc/pointcloud_loss.hip) through the emulator against
tests/golden/pointcloud_loss_grid.npz: the reference's match_pointcloud arithmetic with the reference's own SDFGrid3D and its
autograd gradient w.r.t. the pose (tools/gen_pointcloud_grid_golden.py).  Segments: empty, one point, every point outside the
cube, 257 points on the 33 x 25 x 21 torus, 4096 + 37 points on the 12^3 sphere (three chunks, a non-zero grid offset), the torus
with a quaternion of length 1.3, and a box and a rounded box between the grid segments.

Tolerance: 1e-12 x abs_sum per output, the rule of tests/test_pointcloud_loss_gpu.py (its derivation covers n = 4133); mask
counts exact (every point keeps 1e-6 from the faces of its cube, checked by the generator); the prm outputs of grid segments
exactly 0; analytic segments bit-equal to dss_pointcloud_loss."""
import os

import numpy as np
import pytest

from emu import emu

G = os.path.join(os.path.dirname(__file__), "golden", "pointcloud_loss_grid.npz")
_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)


def table(g):
    grids = [g["grid_0"], g["grid_1"]]
    return (_c(np.cumsum([0] + [x.size for x in grids[:-1]]), np.int32), _c([x.shape for x in grids], np.int32),
            _c(np.concatenate([x.reshape(-1) for x in grids])))


def launch(g, types=None, gid=None, fill=0.0, sel=None):
    """sel: the segments to pass (default all), each with its own points."""
    L = emu.lib()
    sel = np.arange(len(g["shape_type"])) if sel is None else np.asarray(sel)
    n = np.diff(g["seg_off"])[sel]
    off = _c(np.concatenate([[0], np.cumsum(n)]), np.int32)
    pts = _c(np.concatenate([g["pts"][g["seg_off"][s]:g["seg_off"][s + 1]] for s in sel] + [np.zeros((1, 3))]))
    pose, prm = _c(g["pose"][sel]), _c(g["prm"][sel])
    types = _c((g["shape_type"] if types is None else types)[sel], np.int32)
    gid = _c((g["grid_id"] if gid is None else gid)[sel], np.int32)
    goff, gdims, gdata = table(g)
    nseg, max_len = len(sel), int(n.max())
    out = np.full((nseg, 12), fill)
    nbytes = L.dss_pointcloud_loss_workspace_bytes(nseg, max_len)
    ws = np.zeros(max(nbytes // 8, 1))
    rc = L.dss_pointcloud_loss_grids(nseg, max_len, off.ctypes.data, pts.ctypes.data, pose.ctypes.data, types.ctypes.data, prm.ctypes.data,
                                     gid.ctypes.data, 2, goff.ctypes.data, gdims.ctypes.data, gdata.ctypes.data, out.ctypes.data,
                                     ws.ctypes.data, nbytes, None)
    return rc, out


def check_against_golden(out, g):
    names = list(g["names"])
    grid = g["shape_type"] == 7
    for s, name in enumerate(names):
        print(name, "count", out[s, 1], "worst |out - golden| / abs_sum %.2e" % (np.abs(out[s] - g["out"][s]) / np.maximum(g["abs_sum"][s], 1e-300)).max())
    assert np.diff(g["seg_off"])[[names.index(n) for n in ("empty", "one_point", "torus_257", "sphere_4133")]].tolist() == [0, 1, 257, 4133]
    assert abs(np.linalg.norm(g["pose"][names.index("torus_nonunit_quat"), :4]) - 1.3) < 1e-12
    assert g["grid_id"][names.index("sphere_4133")] == 1 and sorted(set(g["shape_type"][~grid])) == [0, 3]
    assert np.array_equal(out[:, 1], g["out"][:, 1]), "mask counts differ"
    assert out[names.index("all_outside"), 1] == 0 and out[names.index("sphere_4133"), 1] > 2048
    bad = np.abs(out - g["out"]) > 1e-12 * g["abs_sum"]
    assert not bad.any(), [(names[s], k, out[s, k], g["out"][s, k], g["abs_sum"][s, k]) for s, k in np.argwhere(bad)]
    assert np.all(out[grid, 9:] == 0.0), "a grid segment has no shape parameter"


def test_kernel_matches_the_reference_golden_on_every_segment():
    g = np.load(G)
    rc, out = launch(g)
    assert rc == 0
    check_against_golden(out, g)
    rc2, again = launch(g)
    assert rc2 == 0 and np.array_equal(out, again)


def test_analytic_segments_are_the_analytic_kernels_bits():
    g = np.load(G)
    L = emu.lib()
    sel = np.nonzero(g["shape_type"] != 7)[0]
    rc, out = launch(g)
    n = np.diff(g["seg_off"])[sel]
    off = _c(np.concatenate([[0], np.cumsum(n)]), np.int32)
    pts = _c(np.concatenate([g["pts"][g["seg_off"][s]:g["seg_off"][s + 1]] for s in sel]))
    pose, prm, types = _c(g["pose"][sel]), _c(g["prm"][sel]), _c(g["shape_type"][sel], np.int32)
    want = np.zeros((len(sel), 12))
    nbytes = L.dss_pointcloud_loss_workspace_bytes(len(sel), int(n.max()))
    ws = np.zeros(max(nbytes // 8, 1))
    assert L.dss_pointcloud_loss(len(sel), int(n.max()), off.ctypes.data, pts.ctypes.data, pose.ctypes.data, types.ctypes.data, prm.ctypes.data,
                                 want.ctypes.data, ws.ctypes.data, nbytes, None) == 0
    assert rc == 0 and len(sel) == 2 and np.array_equal(out[sel], want) and np.all(want[:, 1] > 0)


@pytest.mark.parametrize("kind,gid", [(6, 0), (6, -1), (7, -1)])
def test_refused_segments_give_a_status_and_leave_out_alone(kind, gid):
    g = np.load(G)
    types, ids = g["shape_type"].copy(), g["grid_id"].copy()
    types[4], ids[4] = kind, gid
    rc, out = launch(g, types, ids, fill=-7.0)
    assert rc != 0 and np.all(out == -7.0)
