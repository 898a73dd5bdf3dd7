"""CPU: csrc/cloud_select.hip through the emulator (the kernels, their launch shapes, ballots, prefix popcounts, butterflies and
the LDS tree as on the device) against the numpy reference of tests/cloud_select_ref.py: the select cases of
tests/test_cloud_select_gpu.py, and its statistics at segment lengths that still cross a wavefront and a chunk.  Bounds as
derived there: select exact, count / min / max exact, sums within n 2^-52 sum|x| of math.fsum.
tests/emu/check_cloud_select.cpp is the same walk as a program of its own, built with the address and undefined-behaviour
sanitizers where g++ has their runtimes: nothing may be read or written outside the arrays."""
import os
import subprocess

import numpy as np
import pytest

import cloud_select_ref as ref
from emu import emu

HERE = os.path.dirname(os.path.abspath(__file__))
_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)


def select(pcs, segs, label):
    L = emu.lib()
    pcs, segs = _c(pcs), _c(segs, np.int32)
    nframe, H, W = segs.shape
    rows = np.full(nframe * H, -5, np.int32)
    assert L.dss_cloud_select_count(nframe, H, W, label, pcs.ctypes.data, segs.ctypes.data, rows.ctypes.data, None) == 0
    off = _c(np.cumsum(rows) - rows, np.int32)
    n = int(rows.sum())
    pts = np.full((n + 1, 3), 7.5)      # (one row more: nothing may be written past the last point)
    assert L.dss_cloud_select_emit(nframe, H, W, label, pcs.ctypes.data, segs.ctypes.data, off.ctypes.data, pts.ctypes.data, None) == 0
    assert np.all(pts[n] == 7.5)
    return pts[:n], np.concatenate([[0], np.cumsum(rows.reshape(nframe, H).sum(1))])


def stats(pts, seg_off, fill=0.0):
    L = emu.lib()
    pts, off = _c(pts), _c(seg_off, np.int32)
    nseg, max_len = len(off) - 1, int(np.diff(off).max())
    nbytes = L.dss_cloud_stats_workspace_bytes(nseg, max_len)
    ws = np.zeros(max(nbytes // 8, 1))
    out = np.full((nseg, 10), fill)
    rc = L.dss_cloud_stats(nseg, max_len, off.ctypes.data, pts.ctypes.data if pts.size else None, out.ctypes.data, ws.ctypes.data, nbytes, None)
    return rc, out


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("W,H", ref.SHAPES)
def test_selected_points_equal_boolean_indexing(W, H, kind):
    pcs, segs, label = ref.recording(W, H, kind)
    want, woff = ref.select(pcs, segs, label)
    pts, off = select(pcs, segs, label)
    assert np.array_equal(off, woff) and off[1] == off[2]
    assert pts.shape == want.shape and np.array_equal(pts, want)
    assert (off[-1] == 0) == (kind == "absent")
    assert kind != "full" or off[3] - off[2] == W * H
    again, _ = select(pcs, segs, label)
    assert np.array_equal(pts, again)


def test_segment_statistics_and_their_repeat():
    pts, off = ref.segments(ref.SMALL_SEG_LENS)
    rc, out = stats(pts, off, fill=-7.0)
    assert rc == 0
    ref.check_stats(out, pts, off)
    assert np.array_equal(out[0], [0, 0, 0, 0] + [np.inf] * 3 + [-np.inf] * 3)
    assert np.array_equal(out, stats(pts, off)[1])


def test_only_empty_segments_and_bad_arguments():
    rc, out = stats(np.zeros((0, 3)), [0, 0, 0], fill=-7.0)
    assert rc == 0 and np.array_equal(out, [[0, 0, 0, 0] + [np.inf] * 3 + [-np.inf] * 3] * 2)
    L = emu.lib()
    pts, off = ref.segments([5])
    off32, out = _c(off, np.int32), np.full((1, 10), -7.0)
    assert L.dss_cloud_stats(1, 5, off32.ctypes.data, pts.ctypes.data, out.ctypes.data, None, 0, None) == -2
    assert L.dss_cloud_stats(1, 5, None, pts.ctypes.data, out.ctypes.data, None, 0, None) == -1
    assert L.dss_cloud_stats(1, 5, off32.ctypes.data, None, out.ctypes.data, None, 0, None) == -1
    assert L.dss_cloud_stats(2 ** 28, 0, off32.ctypes.data, None, out.ctypes.data, None, 0, None) == -3      # 10 nseg past an int
    assert L.dss_cloud_stats(2 ** 20, 2049, off32.ctypes.data, pts.ctypes.data, out.ctypes.data, None, 0, None) == -2
    rows = np.full(2, -7, np.int32)
    assert L.dss_cloud_select_count(1, 2, 2, 4, None, off32.ctypes.data, rows.ctypes.data, None) == -1
    assert L.dss_cloud_select_count(0, 2, 2, 4, pts.ctypes.data, off32.ctypes.data, rows.ctypes.data, None) == -1
    assert L.dss_cloud_select_count(2 ** 11, 2 ** 10, 2 ** 10, 4, pts.ctypes.data, off32.ctypes.data, rows.ctypes.data, None) == -3
    assert L.dss_cloud_select_emit(1, 2, 2, 4, pts.ctypes.data, off32.ctypes.data, None, None, None) == -1
    assert np.all(out == -7.0) and np.all(rows == -7)


def test_stand_alone_program_under_the_sanitizers():
    out = os.path.join(HERE, "emu", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "check_cloud_select")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(HERE, "..", "diffsdfsim_amd", "csrc"),
           "-o", exe, os.path.join(HERE, "emu", "check_cloud_select.cpp")]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        # only a link without the sanitizers' runtimes may fall back to a plain build; any other failure is the program's
        assert "cannot find" in san.stderr and ("asan" in san.stderr or "ubsan" in san.stderr), san.stderr[-2000:]
        subprocess.check_call(cmd)
    print("check_cloud_select built %s the sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    w = r.stdout.split()
    assert int(w[0]) == 3 * len(ref.SHAPES) and int(w[2]) == 6, r.stdout      # select cases, segments of the statistics
