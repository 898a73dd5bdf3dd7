"""CPU: csrc/pointcloud_loss.hip through the emulator (both kernels, the launch shape and the reductions as on the device)
against tests/golden/pointcloud_loss.npz, the reference's match_pointcloud arithmetic and its autograd gradient
(tools/gen_pointcloud_golden.py).  Tolerance and inputs as in tests/test_pointcloud_loss_gpu.py: 1e-12 x abs_sum per output,
mask counts exact.  abs_sum is the sum of the absolute per-point terms, except for the quaternion outputs (2..5) of sphere
segments, whose per-point term is exactly zero: there it is the sum of the absolute summands of the chain-rule contraction
(tools/gen_pointcloud_golden.py: reference_terms)."""
import os

import numpy as np
import pytest

from emu import emu

G = os.path.join(os.path.dirname(__file__), "golden", "pointcloud_loss.npz")


def launch(g, types=None, fill=0.0):
    L = emu.lib()
    c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)
    off, pts, pose, prm = c(g["seg_off"], np.int32), c(g["pts"]), c(g["pose"]), c(g["prm"])
    types = c(g["shape_type"] if types is None else types, np.int32)
    nseg, max_len = len(types), int(np.diff(off).max())
    out = np.full((nseg, 12), fill)
    nbytes = L.dss_pointcloud_loss_workspace_bytes(nseg, max_len)
    ws = np.zeros(max(nbytes // 8, 1))
    rc = L.dss_pointcloud_loss(nseg, max_len, off.ctypes.data, pts.ctypes.data, pose.ctypes.data, types.ctypes.data, prm.ctypes.data,
                               out.ctypes.data, ws.ctypes.data, nbytes, None)
    return rc, out


def test_kernel_matches_the_reference_golden_on_every_segment():
    g = np.load(G)
    rc, out = launch(g)
    assert rc == 0
    assert np.array_equal(out[:, 1], g["out"][:, 1]), "mask counts differ"
    bad = np.abs(out - g["out"]) > 1e-12 * g["abs_sum"]
    assert not bad.any(), [(g["names"][s], k, out[s, k], g["out"][s, k], g["abs_sum"][s, k]) for s, k in np.argwhere(bad)]
    rc2, again = launch(g)
    assert rc2 == 0 and np.array_equal(out, again)


@pytest.mark.parametrize("kind", [6, 7])
def test_neural_and_grid_segments_give_a_status_and_leave_out_alone(kind):
    g = np.load(G)
    types = g["shape_type"].copy(); types[3] = kind
    rc, out = launch(g, types, fill=-7.0)
    assert rc != 0 and np.all(out == -7.0)
