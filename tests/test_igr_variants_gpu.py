"""GPU: every launch variant of csrc/igr_mlp.hip and every list form of dss_igr_query_list against the numpy restatement
(tests/implicit_net.py) evaluated in np.longdouble, on seeded geometric-init weights of both network shapes.

Variants<NET, MODE>::launch_mode picks the workgroup shape <waves, row groups> from the list length:
    (128, 2):  < 2048 -> <4,1>,  2048 .. 16383 -> <2,2>,  >= 16384 -> <4,2>        (256, 4):  < 2048 -> <8,1>,  >= 2048 -> <8,2>
LENGTHS holds the smallest lengths that select each of them and leave a ragged last tile (a tangent tile is 4 NG points, a
value tile 16 NG; 2049, 2053 and 16389 are ragged for both).

Tolerance (the rule of test_igr_shapenet_gpu.py::test_query_parity_with_long_double_reference, nothing new): per quantity,
8 x the largest deviation of the SAME restatement in float64 from the long-double result on the same points.  Long double at
256 wide is slow, so it is evaluated on 120 points of each list: the first 40, 40 around the middle and the last 40 (the
tail).  40 consecutive points span both row groups of a two-row-group tile in every mode (asserted).  Every other point is
held by bit equality: with the same points evaluated in chunks of 1024, which take the one-row-group variant -- the claim
"All variants give bit-identical results" of Variants<NetBobSpot>.

List forms (what narrowphase_igr.hip and step_bwd_all.hip call through launch_igr_list; the Python surface passes neither): a
latent code per point out of a table [5][7] whose unused columns and one unnamed row are NaN, and a list length in device
memory, for which the grid is min(512, tiles) workgroups striding over the tiles (5000 tangent points: 625 tiles of <2,2> or
<8,2>; 20000: 2500 tiles of <4,2>, up to five trips per workgroup).  Poison is by value only: every index stays in range.

igr_query2_kernel (the value list and the gradient list of a query round in one launch) has no C ABI entry and is not reached
from here; it shares igr_body with what is."""
import functools

import numpy as np
import pytest
import torch

import igr_helpers as H
import implicit_net as IN

pytestmark = pytest.mark.gpu

NETS = {"bob_spot": dict(seed=3, radius_init=1.0, **IN.BOB_SPOT), "shapenet": dict(seed=126, radius_init=0.6, **IN.SHAPENET)}
LENGTHS = {"bob_spot": (2047, 2048, 2049, 16383, 16384, 16389), "shapenet": (2047, 2048, 2053)}
MODES = {"xyz": 0, "latent": 1, "value": 2}      # DSS_IGR_*
CHUNK = 1024                                     # below 2048: the one-row-group variant of either network
LIST_CAPS = (("bob_spot", 5000), ("bob_spot", 20000), ("shapenet", 5000))
NCODES, STRIDE, DEAD = 5, 7, 2                   # the code table: 5 rows of 7, row 2 named by no live point
LIVE = (0, 1, 3, 4)
QUANTITY = ("value", "d/dlatent", "d/dxyz")


def variant(name, n):
    if name == "shapenet":
        return "<8,2>" if n >= 2048 else "<8,1>"
    return "<4,2>" if n >= 16384 else "<2,2>" if n >= 2048 else "<4,1>"


@functools.lru_cache(None)
def backend():
    from diffsdfsim_amd.engine import TorchBackend
    return TorchBackend("cuda")


@functools.lru_cache(None)
def weights(name):
    return IN.geometric_init(**NETS[name])


@functools.lru_cache(None)
def packed(name):
    return H.packed_on(backend(), *weights(name))


def subset(n):
    """The first 40, 40 around the middle, the last 40; each block spans both row groups of a two-row-group tile, for the
    tangent modes (4 points per group) and for the value mode (16 per group)."""
    sub = np.concatenate([np.arange(40), np.arange(n // 2 - 20, n // 2 + 20), np.arange(n - 40, n)])
    for blk in sub.reshape(3, 40):
        assert set((blk // 4) % 2) == {0, 1} and set((blk // 16) % 2) == {0, 1}
    return sub


def long_double_subset(name, pts, codes, lat_idx, sub):
    """(value, d / d latent, d / d xyz) in long double on the subset, and what float64 loses against it there, per quantity."""
    Ws, bs = weights(name)
    idx = None if lat_idx is None else lat_idx[sub]
    ref = H.reference(Ws, bs, pts[sub], codes, idx, dtype=np.longdouble)
    f64 = H.reference(Ws, bs, pts[sub], codes, idx, dtype=np.float64)
    bound = np.array([float(np.abs(a - b).max()) for a, b in zip(f64, ref)])
    assert np.all(bound > 0) and np.all(bound < 1e-13)
    return ref, bound


@functools.lru_cache(None)
def variant_case(name, n):
    latent = NETS[name]["d_in"] - 3
    r = np.random.default_rng(1000 + n)
    pts = r.uniform(-1, 1, (n, 3)); codes = r.normal(0, 0.1, (1, latent))
    sub = subset(n)
    return (pts, codes, sub) + long_double_subset(name, pts, codes, None, sub)


@functools.lru_cache(None)
def whole_list(name, n, mode):
    pts, codes = variant_case(name, n)[:2]
    return H.query_list(backend(), packed(name), pts, codes, MODES[mode])


def check_subset(tag, name, mode, sdf, grad, sub, ref, bound):
    """The kernel on the subset against long double: 8 x float64's own deviation, per quantity; both figures printed."""
    latent = NETS[name]["d_in"] - 3
    ld = lambda t: t.cpu().numpy()[sub].astype(np.longdouble)
    checks = [(0, float(np.abs(ld(sdf) - ref[0]).max()))]
    if grad is not None:
        want = H.expected_grad(ref, latent, MODES[mode])
        assert grad.shape[1] == want.shape[1]
        checks.append((1 if mode == "latent" else 2, float(np.abs(ld(grad) - want).max())))
        assert float(np.abs(want).max(0)[: latent if mode == "latent" else 3].min()) > 1e-3      # (no column passes by being zero)
    for q, err in checks:
        print("%s %s %s: float64 numpy vs long double %.3e, kernel vs long double %.3e" % (tag, mode, QUANTITY[q], bound[q], err))
    for q, err in checks:
        assert err <= 8 * bound[q], (tag, mode, QUANTITY[q], err, bound[q])


CASES = [(name, n) for name in NETS for n in LENGTHS[name]]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name, n", CASES)
def test_variant_matches_long_double(name, n, mode):
    pts, codes, sub, ref, bound = variant_case(name, n)
    sdf, grad = whole_list(name, n, mode)
    assert bool(torch.isfinite(sdf).all()) and (grad is None or bool(torch.isfinite(grad).all()))
    check_subset("%s %s n=%d" % (name, variant(name, n), n), name, mode, sdf, grad, sub, ref, bound)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name, n", CASES)
def test_variant_equals_chunks_of_1024_bit_for_bit(name, n, mode):
    """Every point of the list: the value and every gradient column equal, bit for bit, the same points evaluated 1024 at a
    time (the one-row-group variant <4,1> or <8,1>, the one test_igr_gpu.py and test_igr_shapenet_gpu.py pin at n = 1000)."""
    pts, codes = variant_case(name, n)[:2]
    sdf, grad = whole_list(name, n, mode)
    parts = [H.query_list(backend(), packed(name), pts[a:a + CHUNK], codes, MODES[mode]) for a in range(0, n, CHUNK)]
    s1 = torch.cat([p[0] for p in parts])
    same = torch.equal(sdf, s1) and (grad is None or torch.equal(grad, torch.cat([p[1] for p in parts])))
    print("%s %s n=%d %s: whole list and chunks of %d bit-equal: %s" % (name, variant(name, n), n, mode, CHUNK, same))
    assert same


@functools.lru_cache(None)
def list_case(name, n_cap):
    latent = NETS[name]["d_in"] - 3
    r = np.random.default_rng(2000 + n_cap)
    pts = r.uniform(-1, 1, (n_cap, 3))
    codes = H.poisoned_codes(r, NCODES, latent, STRIDE, DEAD)
    lat_idx = np.asarray(LIVE, np.int32)[r.integers(0, len(LIVE), n_cap)]
    sub = subset(n_cap)
    assert all(set(lat_idx[blk]) == set(LIVE) for blk in sub.reshape(3, 40))
    return (pts, codes, lat_idx, sub) + long_double_subset(name, pts, codes, lat_idx, sub)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name, n_cap", LIST_CAPS)
def test_per_point_codes(name, n_cap, mode):
    """lat_idx with a strided, poisoned table, with the length on the host and in device memory (the striding grid): the
    subset against long double with every point's own code, every point against the same list evaluated one code at a time
    without lat_idx, bit for bit."""
    P = packed(name)
    pts, codes, lat_idx, sub, ref, bound = list_case(name, n_cap)
    single = {c: H.query_list(backend(), P, pts, codes[c:c + 1], MODES[mode]) for c in LIVE}
    for n_dev in (None, n_cap):
        tag = "%s %s n_cap=%d n_dev=%s per-point codes" % (name, variant(name, n_cap), n_cap, n_dev)
        sdf, grad = H.query_list(backend(), P, pts, codes, MODES[mode], lat_idx=lat_idx, n_dev=n_dev)
        assert bool(torch.isfinite(sdf).all()) and (grad is None or bool(torch.isfinite(grad).all())), tag
        check_subset(tag, name, mode, sdf, grad, sub, ref, bound)
        same = True
        for c in LIVE:
            m = torch.as_tensor(lat_idx == c, device=sdf.device)
            same = same and torch.equal(sdf[m], single[c][0][m]) and (grad is None or torch.equal(grad[m], single[c][1][m]))
        print("%s %s: equal to one code at a time, bit for bit: %s" % (tag, mode, same))
        assert same, tag


@pytest.mark.parametrize("length", ["0", "1", "n_cap-3", "n_cap"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name, n_cap", LIST_CAPS)
def test_device_length(name, n_cap, mode, length):
    """The length in device memory.  Entries below it equal the host-length call on the first n_dev points bit for bit;
    entries from it on still hold the sentinel the buffers were filled with -- all gradient columns, for L = 4 in latent mode
    after both passes.  The points beyond the length are NaN and name the NaN row of the table."""
    P = packed(name)
    n_dev = {"0": 0, "1": 1, "n_cap-3": n_cap - 3, "n_cap": n_cap}[length]
    pts, codes, lat_idx = list_case(name, n_cap)[:3]
    pts, lat_idx = pts.copy(), lat_idx.copy()
    pts[n_dev:] = np.nan; lat_idx[n_dev:] = DEAD
    sdf, grad = H.query_list(backend(), P, pts, codes, MODES[mode], lat_idx=lat_idx, n_dev=n_dev, fill=H.SENTINEL)
    kept = bool((sdf[n_dev:] == H.SENTINEL).all()) and (grad is None or bool((grad[n_dev:] == H.SENTINEL).all()))
    print("%s %s n_cap=%d n_dev=%d %s: outputs beyond n_dev unchanged: %s" % (name, variant(name, n_cap), n_cap, n_dev, mode, kept))
    assert kept
    if n_dev:
        s0, g0 = H.query_list(backend(), P, pts[:n_dev], codes, MODES[mode], lat_idx=lat_idx[:n_dev])
        assert bool(torch.isfinite(s0).all())
        same = torch.equal(sdf[:n_dev], s0) and (grad is None or torch.equal(grad[:n_dev], g0))
        print("%s n_cap=%d n_dev=%d %s: equal to the host-length call, bit for bit: %s" % (name, n_cap, n_dev, mode, same))
        assert same
