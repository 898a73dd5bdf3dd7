"""numpy reference of csrc/cloud_select.hip and the cases its tests share (tests/test_cloud_select_gpu.py on the device,
tests/test_emu_cloud_select.py through the emulator).

select: `pcs[t][(segs[t] == label) & all three coordinates finite]`, row-major per frame -- exact, the kernel copies doubles.
stats:  count, min, max exact; a sum of n doubles in ANY order differs from the exact sum by at most (n - 1) u sum|x| to first
        order, u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the bound held here is
        n 2^-52 sum|x| against math.fsum (the correctly rounded sum, itself within u |sum| of the exact one)."""
import math

import numpy as np

LABEL = 4
SHAPES = [(1, 3), (63, 2), (64, 2), (65, 3), (130, 7), (3, 1)]      # (W, H): below, at and above a wavefront of columns
KINDS = ["mixed", "absent", "full"]
SEG_LENS = [0, 1, 63, 64, 65, 2048, 2049, 5000]      # straddle a wavefront, a chunk of 2 048 and two chunks
SMALL_SEG_LENS = [0, 1, 63, 64, 65, 2049]            # what the emulator runs: the same edges, one chunk boundary


def recording(W, H, kind, nframe=3):
    """(pcs [nframe,H,W,3], segs [nframe,H,W] int32, label).  mixed: the label among others (0..5, -1), NaN / +inf / -inf in one
    coordinate of some labelled and some other pixels; the middle frame holds no pixel of the label.  absent: the label occurs
    nowhere.  full: the label fills every frame but the middle one, a few points non-finite."""
    r = np.random.default_rng(1000 * W + 10 * H + KINDS.index(kind))
    pcs = r.uniform(-3.0, 3.0, (nframe, H, W, 3))
    if kind == "full":
        segs = np.full((nframe, H, W), LABEL)
    else:
        segs = r.integers(-1, 6, (nframe, H, W))
        segs[r.random((nframe, H, W)) < 0.4] = LABEL
    if kind == "absent":
        segs[segs == LABEL] = 2
    segs[nframe // 2][segs[nframe // 2] == LABEL] = 0
    bad = r.random((nframe, H, W)) < 0.15
    if kind == "full":
        bad[-1] = False      # every pixel of the last frame is selected
    which = r.integers(0, 3, (nframe, H, W))
    value = np.array([np.nan, np.inf, -np.inf])[r.integers(0, 3, (nframe, H, W))]
    f, y, x = np.nonzero(bad)
    pcs[f, y, x, which[bad]] = value[bad]
    if kind != "absent" and W * H >= 3:      # a dropped point between two kept ones, wherever the draw put the others
        flat_s, flat_p = segs[0].reshape(-1), pcs[0].reshape(-1, 3)
        flat_s[:3] = LABEL
        flat_p[:3] = [[0.5, -1.5, 2.5], [1.0, np.nan, 1.0], [-0.25, 0.75, -2.0]]
    return pcs, segs.astype(np.int32), LABEL


def select(pcs, segs, label):
    """-> (pts [N,3], seg_off [nframe+1] int64)"""
    keep = (segs == label) & np.isfinite(pcs).all(axis=3)
    pts = [pcs[t][keep[t]] for t in range(len(pcs))]
    return np.concatenate(pts).reshape(-1, 3), np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)


def segments(lens, seed=7):
    """(pts [N,3], seg_off) with the given segment lengths; coordinates of mixed sign and magnitude so that sums cancel."""
    r = np.random.default_rng(seed)
    n = int(np.sum(lens))
    pts = r.standard_normal((n, 3)) * 10.0 ** r.integers(-3, 4, (n, 1)) + np.array([0.0, 5.0, -1e3])
    return pts, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def stats(pts, seg_off):
    """-> (out [nseg,10]: count, fsum xyz, min xyz, max xyz; abs_sum [nseg,3])"""
    nseg = len(seg_off) - 1
    out, abs_sum = np.zeros((nseg, 10)), np.zeros((nseg, 3))
    for s in range(nseg):
        p = pts[seg_off[s]:seg_off[s + 1]]
        out[s, 0] = len(p)
        for k in range(3):
            out[s, 1 + k] = math.fsum(p[:, k])
            abs_sum[s, k] = math.fsum(np.abs(p[:, k]))
        out[s, 4:7] = p.min(axis=0) if len(p) else np.inf
        out[s, 7:10] = p.max(axis=0) if len(p) else -np.inf
    return out, abs_sum


def check_stats(got, pts, seg_off):
    want, abs_sum = stats(pts, seg_off)
    n = np.diff(seg_off)[:, None]
    assert np.array_equal(got[:, 0], want[:, 0]), "counts differ"
    assert np.array_equal(got[:, 4:], want[:, 4:]), "min / max differ"
    err, bound = np.abs(got[:, 1:4] - want[:, 1:4]), n * 2.0 ** -52 * abs_sum
    assert (err <= bound).all(), (err, bound)
    return float((err / np.maximum(bound, 1e-300)).max())
