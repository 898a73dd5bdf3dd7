"""GPU: the selection of a labelled body's points from recorded organised clouds and the per-segment statistics
(diffsdfsim_amd/recorded.py over csrc/cloud_select.hip) against the numpy reference of tests/cloud_select_ref.py.

Select copies doubles, so points and offsets are EQUAL to `pcs[t][(segs[t] == label) & finite]`.  Stats: count, min and max are
exact; a sum is within n 2^-52 sum|x| of math.fsum, the bound for any summation order of n terms (derived in
cloud_select_ref.py).  Shapes: widths below, at and above the 64 columns a wavefront takes at a time, more rows than one
workgroup holds wavefronts (7 > 4), a single pixel column and a single row; segment lengths around a wavefront (63, 64, 65), the
chunk of 2 048 points (2 048, 2 049) and two chunks (5 000), with empty and one-point segments, all in one call."""
import numpy as np
import pytest
import torch

import cloud_select_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("W,H", ref.SHAPES)
def test_selected_points_equal_boolean_indexing(W, H, kind):
    from diffsdfsim_amd import recorded
    pcs, segs, label = ref.recording(W, H, kind)
    want, woff = ref.select(pcs, segs, label)
    pts, off = recorded.select_points(dev(pcs), dev(segs, torch.int32), label)
    assert off.dtype == np.int64 and np.array_equal(off, woff) and off[1] == off[2], "the middle frame holds no pixel of the label"
    assert tuple(pts.shape) == want.shape and np.array_equal(pts.cpu().numpy(), want)
    if kind == "absent":
        assert off[-1] == 0
    else:
        assert 0 < off[-1] and (W * H < 3 or np.array_equal(want[:2], [[0.5, -1.5, 2.5], [-0.25, 0.75, -2.0]]))      # the NaN between them is gone
    if kind == "full":
        assert off[3] - off[2] == W * H
    again, off2 = recorded.select_points(dev(pcs), dev(segs, torch.int32), label)
    assert torch.equal(pts, again) and np.array_equal(off, off2)


def test_other_labels_select_their_own_pixels():
    from diffsdfsim_amd import recorded
    pcs, segs, _ = ref.recording(130, 7, "mixed")
    for label in (0, 5, -1, 17):
        want, woff = ref.select(pcs, segs, label)
        pts, off = recorded.select_points(dev(pcs), dev(segs, torch.int32), label)
        assert np.array_equal(off, woff) and np.array_equal(pts.cpu().numpy(), want)


def test_segment_statistics():
    from diffsdfsim_amd import recorded
    pts, off = ref.segments(ref.SEG_LENS)
    out = recorded._stats(dev(pts), off)
    worst = ref.check_stats(out.cpu().numpy(), pts, off)
    print("sums: worst error / bound %.3f" % worst)
    assert torch.equal(out, recorded._stats(dev(pts), off)), "two calls differ"
    st = recorded.segment_stats(dev(pts), off)
    got = {k: v.cpu().numpy() for k, v in st.items()}
    assert np.array_equal(got["count"], ref.SEG_LENS) and np.array_equal(got["min"], out[:, 4:7].cpu().numpy())
    assert np.isnan(got["mean"][0]).all() and np.array_equal(got["min"][0], [np.inf] * 3) and np.array_equal(got["max"][0], [-np.inf] * 3)
    assert np.array_equal(got["mean"][1], pts[0]) and np.array_equal(got["mean"][1:], got["sum"][1:] / got["count"][1:, None])


def test_statistics_of_selected_frames():
    from diffsdfsim_amd import recorded
    pcs, segs, label = ref.recording(130, 7, "mixed")
    pts, off = recorded.select_points(dev(pcs), dev(segs, torch.int32), label)
    ref.check_stats(recorded._stats(pts, off).cpu().numpy(), pts.cpu().numpy(), off)


def test_host_tensors_and_wrong_dtypes_raise():
    from diffsdfsim_amd import _lib, recorded
    pcs, segs, label = ref.recording(3, 1, "mixed")
    host = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt)
    with pytest.raises(_lib.HipLibraryError):
        recorded.select_points(host(pcs, torch.float64), host(segs, torch.int32))
    with pytest.raises(ValueError):
        recorded.select_points(dev(pcs, torch.float32), dev(segs, torch.int32))
    with pytest.raises(ValueError):
        recorded.select_points(dev(pcs), dev(segs, torch.int64))
    with pytest.raises(ValueError):
        recorded.select_points(dev(pcs)[:, :, :, :2], dev(segs, torch.int32))
    with pytest.raises(_lib.HipLibraryError):
        recorded.segment_stats(torch.zeros(4, 3, dtype=torch.float64), [0, 4])
    with pytest.raises(ValueError):
        recorded.segment_stats(torch.zeros(4, 3, dtype=torch.float32, device=DEV), [0, 4])
    with pytest.raises(ValueError):
        recorded.segment_stats(torch.zeros(4, 3, dtype=torch.float64, device=DEV), [0, 5])


def test_bad_arguments_give_a_status_before_any_launch():
    from diffsdfsim_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(torch.device(DEV))
    pcs, segs = torch.zeros(1, 2, 2, 3, dtype=torch.float64, device=DEV), torch.zeros(1, 2, 2, dtype=torch.int32, device=DEV)
    rows = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    assert L.dss_cloud_select_count(1, 2, 2, 0, None, p(segs), p(rows), st) == -1
    assert L.dss_cloud_select_count(1, 2, -2, 0, p(pcs), p(segs), p(rows), st) == -1
    assert L.dss_cloud_select_count(2 ** 11, 2 ** 10, 2 ** 10, 0, p(pcs), p(segs), p(rows), st) == -3      # 2^31 pixels
    assert L.dss_cloud_select_emit(1, 2, 2, 0, p(pcs), p(segs), None, None, st) == -1
    out = torch.full((1, 10), -7.0, dtype=torch.float64, device=DEV)
    assert L.dss_cloud_stats(1, 4, None, p(pcs), p(out), None, 0, st) == -1
    assert L.dss_cloud_stats(-1, 4, p(rows), p(pcs), p(out), None, 0, st) == -1
    assert L.dss_cloud_stats(1, 4, p(rows), p(pcs), p(out), None, 0, st) == -2      # no workspace
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((out == -7.0).all())
