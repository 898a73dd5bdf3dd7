"""CPU: the list forms of dss_igr_query_list (csrc/igr_mlp.hip) through the emulator -- a latent code per point out of a
strided table, a list length in device memory with a persistent grid, the argument checks -- against the numpy restatement
(tests/implicit_net.py) in float64, with the tolerances of tests/test_igr_shapes_cpu.py (1e-12 values, 1e-11 gradients).
These are what narrowphase_igr.hip and step_bwd_all.hip call; the product's Python surface passes one code and a host length.
The device runs of the same forms are tests/test_igr_variants_gpu.py."""
import functools

import numpy as np
import pytest

import igr_helpers as H
import implicit_net as IN

BADARG, UNSUPPORTED = -1, -3      # DSS_E_BADARG, DSS_E_UNSUPPORTED (include/diffsdfsim_hip.h)
NETS = {"bob_spot": dict(seed=3, radius_init=1.0, **IN.BOB_SPOT), "shapenet": dict(seed=5, radius_init=0.6, **IN.SHAPENET)}
MODES = {"xyz": 0, "latent": 1, "value": 2}      # DSS_IGR_*
N_CAP, NCODES, STRIDE, DEAD = 53, 3, 7, 1      # 53: ragged for the 4-point tangent groups and the 16-point value groups
VTOL, GTOL = 1e-12, 1e-11


@functools.lru_cache(None)
def backend():
    from emu import emu
    return emu.EmuBackend()


@functools.lru_cache(None)
def network(name):
    Ws, bs = IN.geometric_init(**NETS[name])
    return Ws, bs, H.packed_on(backend(), Ws, bs)


@functools.lru_cache(None)
def case(name):
    """53 points, each with one of the two live codes of a 3-row table of stride 7 (row 1 and columns L.. are NaN), and the
    float64 reference with every point's own code."""
    Ws, bs, _P = network(name)
    latent = Ws[0].shape[1] - 3
    r = np.random.default_rng(11)
    pts = r.uniform(-1, 1, (N_CAP, 3))
    codes = H.poisoned_codes(r, NCODES, latent, STRIDE, DEAD)
    lat_idx = np.where(r.random(N_CAP) < 0.5, 0, 2).astype(np.int32)
    assert set(lat_idx[:8]) == {0, 2}      # (both codes within the first two tangent tiles)
    return pts, codes, lat_idx, H.reference(Ws, bs, pts, codes, lat_idx)


@pytest.mark.parametrize("n_dev", [0, 37, 53])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(NETS))
def test_emu_list_forms(name, mode, n_dev):
    """A code per point and a length in device memory (53 = the whole list): entries below the length match the reference
    evaluated with each point's own code, entries from it on still hold what the buffers held before -- in every gradient
    column, for L = 4 in latent mode after both passes.  The points beyond the length are NaN and name the NaN row of the
    table."""
    Ws, bs, P = network(name)
    latent = Ws[0].shape[1] - 3
    pts, codes, lat_idx, ref = case(name)
    n = n_dev
    pts, lat_idx = pts.copy(), lat_idx.copy()
    pts[n:] = np.nan; lat_idx[n:] = DEAD
    sdf, grad = H.query_list(backend(), P, pts, codes, MODES[mode], lat_idx=lat_idx, n_dev=n_dev, fill=H.SENTINEL)
    assert np.all(sdf[n:] == H.SENTINEL) and (grad is None or np.all(grad[n:] == H.SENTINEL))
    if n:
        assert np.abs(sdf[:n] - ref[0][:n]).max() < VTOL
    if grad is not None and n:
        want = H.expected_grad(ref, latent, MODES[mode])
        assert grad.shape == (N_CAP, want.shape[1]) and np.abs(grad[:n] - want[:n]).max() < GTOL
        assert np.abs(want).max(0)[: latent if mode == "latent" else 3].min() > 1e-3      # (no column passes by being zero)


def test_emu_argument_checks():
    B = backend()
    Ws, bs, P = network("shapenet")
    net = H.net_struct(B, P)
    pts = B.from_numpy(np.zeros((4, 3))); codes = B.from_numpy(np.zeros((1, 7)))
    sdf = B.from_numpy(np.zeros(4)); grad = B.from_numpy(np.zeros((4, 4)))
    call = lambda net=net, stride=7, n_cap=4, mode=0, grad=grad, pts=pts, codes=codes, sdf=sdf: \
        H.call_query_list(B, net, pts, None, codes, stride, None, n_cap, mode, sdf, grad)
    assert call() == 0 and call(stride=4) == 0 and call(mode=2, grad=None) == 0
    assert call(stride=3) == BADARG                                  # lat_stride below L
    assert call(mode=3) == BADARG and call(mode=-1) == BADARG
    assert call(mode=0, grad=None) == BADARG and call(mode=1, grad=None) == BADARG
    assert call(n_cap=0) == BADARG and call(n_cap=-5) == BADARG
    assert call(net=None) == BADARG and call(pts=None) == BADARG and call(codes=None) == BADARG and call(sdf=None) == BADARG
    from diffsdfsim_amd import world_abi
    for k in world_abi.IGR_NET_POINTERS:
        broken = H.net_struct(B, P)
        setattr(broken, k, None)
        assert call(net=broken) == BADARG, k
    # shapes no kernel is built for, by net_kind: width 192, and a known width with the other network's latent size
    assert call(net=H.net_struct(B, P, width=192)) == UNSUPPORTED
    assert call(net=H.net_struct(B, P, width=128)) == UNSUPPORTED and call(net=H.net_struct(B, P, latent=2)) == UNSUPPORTED
    # (128, 2): the stride rule with the shape spelled out and with the header's default 0, 0
    Ws2, bs2, P2 = network("bob_spot")
    for shape in (dict(), dict(width=0, latent=0)):
        net2 = H.net_struct(B, P2, **shape)
        assert call(net=net2, stride=2) == 0 and call(net=net2, stride=1) == BADARG
    assert call(net=H.net_struct(B, P2, width=192)) == UNSUPPORTED


def test_emu_two_row_groups_2048_values():
    """2048 value-only points of the (128, 2) network: the shortest list that takes the two-row-group variant <2, 2> (tiles of
    32 points: acc[g][t], aq[..][g] and the X rows 16 g + .. for g = 1).  120 points -- the first, middle and last 40, each
    block spanning both row groups -- against float64 numpy, and every point against two 1024-point calls, which take the
    one-row-group variant <4, 1>: array equality, igr_mlp.hip's 'All variants give bit-identical results'."""
    Ws, bs, P = network("bob_spot")
    r = np.random.default_rng(12)
    n = 2048
    pts = r.uniform(-1, 1, (n, 3)); codes = r.normal(0, 0.1, (1, 2))
    sdf, _ = H.query_list(backend(), P, pts, codes, MODES["value"])
    sub = np.concatenate([np.arange(40), np.arange(n // 2 - 20, n // 2 + 20), np.arange(n - 40, n)])
    for blk in sub.reshape(3, 40):
        assert set((blk // 16) % 2) == {0, 1}
    want = IN.query(pts[sub], codes[0], Ws, bs, jacobian=False)
    assert np.abs(sdf[sub] - want).max() < VTOL
    parts = [H.query_list(backend(), P, pts[a:a + 1024], codes, MODES["value"])[0] for a in (0, 1024)]
    assert np.array_equal(sdf, np.concatenate(parts))
