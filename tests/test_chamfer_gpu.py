"""GPU: diffsdfsim_amd/chamfer.py over csrc/chamfer.hip against the numpy reference of tests/chamfer_ref.py (whose docstring
derives every bound used here) and against the parent's experiments.chamfer (torch.cdist, the expanded form) within
2^-44 max(|a|^2 + |b|^2).  The shapes are those of tests/test_emu_chamfer.py: nine unequal segments across the wavefront,
query-block and tile boundaries on the direct and on the split path (more than SPLIT_TILES tiles in the longest reference segment:
partials through the workspace, merge kernel), the integer lattice on both."""
import numpy as np
import pytest
import torch

import chamfer_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def _cases(path, shift=None):
    from diffsdfsim_amd import chamfer
    lens = ref.segment_cases(chamfer.QUERIES, chamfer.TILE)[path]
    assert (chamfer.splits(len(lens), max(a for a, _ in lens), max(b for _, b in lens)) > 1) == (path == "split")
    return ref.random_clouds([a for a, _ in lens], [b for _, b in lens], seed=11, shift=shift)


@pytest.mark.parametrize("shift", [None, ref.SHIFT], ids=["origin", "shifted"])
@pytest.mark.parametrize("path", ["direct", "split"])
def test_nearest_against_argmin_of_the_direct_form(path, shift):
    """Shifted by (1e3, -2e3, 5e2) the same relative bound holds: what an expanded form cannot do."""
    from diffsdfsim_amd import chamfer
    q, qo, r, ro = _cases(path, shift)
    d2, idx = chamfer.nearest(dev(q), qo, dev(r), ro)
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32 and d2.is_cuda
    ref.check_nn(d2.cpu().numpy(), idx.cpu().numpy(), q, qo, r, ro)
    again = chamfer.nearest(dev(q), torch.as_tensor(qo), dev(r), ro)
    assert torch.equal(d2, again[0]) and torch.equal(idx, again[1])


@pytest.mark.parametrize("nr_tiles,extra", [(2, 0), (3, 1), (5, 1)], ids=["direct", "split2", "split3"])
def test_integer_lattice_is_exact_and_ties_keep_the_lowest_index(nr_tiles, extra):
    from diffsdfsim_amd import chamfer
    q, r = ref.lattice_clouds(chamfer.QUERIES + 65, nr_tiles * chamfer.TILE + extra, seed=3)
    qo, ro = np.array([0, len(q)]), np.array([0, len(r)])
    d2, idx = chamfer.nearest(dev(q), qo, dev(r), ro)
    ref.check_nn(d2.cpu().numpy(), idx.cpu().numpy(), q, qo, r, ro, exact=True)


def test_one_long_scene_takes_many_splits():
    from diffsdfsim_amd import chamfer
    q, qo, r, ro = ref.random_clouds([700], [9 * chamfer.TILE + 7], seed=4)
    assert chamfer.splits(1, 700, 9 * chamfer.TILE + 7) == 5
    d2, idx = chamfer.nearest(dev(q), qo, dev(r), ro)
    ref.check_nn(d2.cpu().numpy(), idx.cpu().numpy(), q, qo, r, ro)


@pytest.mark.parametrize("shift", [None, ref.SHIFT], ids=["origin", "shifted"])
@pytest.mark.parametrize("path", ["direct", "split"])
def test_value_and_gradient_per_scene(path, shift):
    from diffsdfsim_amd import chamfer
    a, ao, b, bo = _cases(path, shift)
    ta, tb = dev(a).requires_grad_(), dev(b).requires_grad_()
    out = chamfer.chamfer_packed(ta, ao, tb, bo)
    again = chamfer.chamfer_packed(ta, ao, tb, bo)
    assert tuple(out.shape) == (len(ao) - 1,) and torch.equal(out.detach().view(torch.int64), again.detach().view(torch.int64))      # (bits: two are NaN)
    out.sum().backward()
    got, ga, gb = out.detach().cpu().numpy(), ta.grad.cpu().numpy(), tb.grad.cpu().numpy()
    worst = 0.0
    for s in range(len(ao) - 1):
        A, B = a[ao[s]:ao[s + 1]], b[bo[s]:bo[s + 1]]
        if len(A) == 0 or len(B) == 0:
            assert np.isnan(got[s]) and not ga[ao[s]:ao[s + 1]].any() and not gb[bo[s]:bo[s + 1]].any()
            continue
        want = ref.value(A, B)
        assert abs(got[s] - want) <= ref.value_bound(want, max(len(A), len(B))), (s, got[s], want)
        wa, wb, ba, bb = ref.grad(A, B)
        ea, eb = np.abs(ga[ao[s]:ao[s + 1]] - wa), np.abs(gb[bo[s]:bo[s + 1]] - wb)
        worst = max(worst, (ea / np.maximum(ba, 1e-300)).max(), (eb / np.maximum(bb, 1e-300)).max())
        assert np.all(ea <= ba) and np.all(eb <= bb), (s, (ea / np.maximum(ba, 1e-300)).max(), (eb / np.maximum(bb, 1e-300)).max())
    print("chamfer gradient: worst error / bound %.3g" % worst)


def test_gradient_against_autograd_through_the_parents_chamfer():
    from diffsdfsim_amd import chamfer, experiments as X
    a, ao, b, bo = ref.random_clouds([1500], [1100], seed=8)
    ta, tb = dev(a).requires_grad_(), dev(b).requires_grad_()
    chamfer.chamfer_packed(ta, ao, tb, bo).sum().backward()
    pa, pb = dev(a).requires_grad_(), dev(b).requires_grad_()
    parent = X.chamfer(pa, pb)
    parent.backward()
    bound = ref.parent_bound(a, b)
    assert abs(float(parent.detach()) - ref.value(a, b)) <= bound
    # (a second reference for the gradient, at the bound of the parent's expanded form)
    assert float((ta.grad - pa.grad).abs().max()) <= bound and float((tb.grad - pb.grad).abs().max()) <= bound


def test_identical_clouds_give_zero_and_zero_gradient():
    from diffsdfsim_amd import chamfer
    a, ao, _, _ = ref.random_clouds([777], [1], seed=9)
    ta, tb = dev(a).requires_grad_(), dev(a).requires_grad_()
    out = chamfer.chamfer_packed(ta, ao, tb, ao)
    out.sum().backward()
    assert float(out.detach()) == 0.0 and not ta.grad.any() and not tb.grad.any()


def test_batch_of_mixed_host_and_device_clouds_against_the_parent():
    from diffsdfsim_amd import chamfer, experiments as X
    na, nb = [200, 3000, 1111, 640, 2049], [3000, 200, 900, 2500, 513]
    a, ao, b, bo = ref.random_clouds(na, nb, seed=10)
    A, B = [a[ao[s]:ao[s + 1]] for s in range(5)], [b[bo[s]:bo[s + 1]] for s in range(5)]
    mixed_a = [A[0], torch.as_tensor(A[1]), dev(A[2]), A[3], dev(A[4])]
    mixed_b = [dev(B[0]), B[1], torch.as_tensor(B[2]), dev(B[3]), B[4]]
    out = chamfer.chamfer_batch(mixed_a, mixed_b)
    assert out.is_cuda and tuple(out.shape) == (5,)
    for s in range(5):
        parent = float(X.chamfer(torch.as_tensor(A[s]), torch.as_tensor(B[s])))
        want = ref.value(A[s], B[s])
        assert abs(float(out[s]) - parent) <= ref.parent_bound(A[s], B[s]), (s, float(out[s]), parent)
        assert abs(float(out[s]) - want) <= ref.value_bound(want, max(na[s], nb[s]))


def test_bad_inputs_raise_as_recorded_does():
    from diffsdfsim_amd import _lib, chamfer
    q, r = dev(np.zeros((4, 3))), dev(np.ones((5, 3)))
    with pytest.raises(_lib.HipLibraryError):
        chamfer.nearest(q.cpu(), [0, 4], r, [0, 5])
    with pytest.raises(_lib.HipLibraryError):
        chamfer.chamfer_packed(q, [0, 4], r.cpu(), [0, 5])
    with pytest.raises(TypeError):
        chamfer.nearest(np.zeros((4, 3)), [0, 4], r, [0, 5])
    for bad in (q.float(), q.reshape(3, 4), q.reshape(-1)):
        with pytest.raises(ValueError):
            chamfer.nearest(bad, [0, 4], r, [0, 5])
    for off in ([0, 3, 2, 4], [0, 5], [-1, 4], [0]):
        with pytest.raises(ValueError):
            chamfer.nearest(q, off, r, [0, 5] if len(off) != 4 else [0, 1, 2, 5])
    with pytest.raises(ValueError):
        chamfer.nearest(q, [0, 2, 4], r, [0, 5])      # two query segments, one reference segment


def test_inertia_fit_reports_the_parents_chamfer_per_scene():
    """hist[..]['chamfer'] of fit_inertia_primitive keeps its shape and meaning: the parent's per-scene chamfer of the same meshes."""
    from diffsdfsim_amd import experiments as X
    tgt, st = np.array([[1.0], [1.2]]), np.array([[1.25], [0.96]])
    dirs = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8]])
    res = X.fit_inertia_primitive("sphere", tgt, st, dirs, run_time=0.2, max_iter=2, lr=2e-2)
    h = res["history"]
    assert len(h) == 2 and all(x["chamfer"].shape == (2,) for x in h)
    wt = X.primitive_spin_world("sphere", torch.as_tensor(tgt))
    for x in h:
        w = X.primitive_spin_world("sphere", torch.as_tensor(x["dims"]))
        for s in range(2):
            a, b = np.asarray(w.meshes[s][0], np.float64), np.asarray(wt.meshes[s][0], np.float64)
            parent = float(X.chamfer(torch.as_tensor(a), torch.as_tensor(b)))
            assert abs(x["chamfer"][s] - parent) <= ref.parent_bound(a, b), (s, x["chamfer"][s], parent)
            assert x["chamfer"][s] > 0


def test_sphere_radius_fit_logs_a_falling_chamfer_series():
    from diffsdfsim_amd import experiments as X
    r = np.random.default_rng(5)
    B = 8
    target = 0.5 + 0.8 * r.random(B)
    start = target + np.where(r.random(B) < 0.5, -0.15, 0.15)
    res = X.fit_sphere_radius(target, start, run_time=1.0, max_iter=12, lr=0.1)
    h = res["history"]
    assert all(x["chamfer"].shape == (B,) for x in h)
    assert h[-1]["chamfer"].mean() < h[0]["chamfer"].mean(), (h[0]["chamfer"], h[-1]["chamfer"])
