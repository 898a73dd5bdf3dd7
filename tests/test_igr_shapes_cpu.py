"""CPU: both network shapes through pack_weights / weights_from_module (diffsdfsim_amd/igr.py), and the 256-wide
instantiation of csrc/igr_mlp.hip through the emulator against the numpy restatement (tests/implicit_net.py)."""
import ctypes

import numpy as np
import pytest

import implicit_net as IN


def fragment_order(W, width):
    """[tile][k-step][lane] = W[16 t + (lane & 15)][4 ks + (lane >> 4)], entry by entry."""
    out = np.zeros((width // 16, width // 4, 64))
    for t in range(width // 16):
        for ks in range(width // 4):
            for lane in range(64):
                out[t, ks, lane] = W[16 * t + (lane & 15), 4 * ks + (lane >> 4)]
    return out


def test_pack_weights_shapenet_fragment_order():
    from diffsdfsim_amd.igr import pack_weights
    Ws, bs = IN.geometric_init(seed=5, radius_init=0.6, **IN.SHAPENET)
    bs = [b + 0.01 * np.arange(len(b)) for b in bs]      # (geometric init has zero biases: make the padding visible)
    P = pack_weights(Ws, bs, device="cpu")
    Wp, bh = P["Wp"].numpy(), P["bh"].numpy()
    assert Wp.shape == (7, 16, 64, 64) and bh.shape == (7, 256)
    assert P["W0"].shape == (256, 7) and P["b0"].shape == (256,) and P["W8"].shape == (256,) and P["b8"].shape == (1,)
    for l in range(1, 8):
        W = np.zeros((256, 256)); W[: Ws[l].shape[0]] = Ws[l]
        assert np.array_equal(Wp[l - 1], fragment_order(W, 256)), l
        assert np.array_equal(bh[l - 1, : len(bs[l])], bs[l]) and np.all(bh[l - 1, len(bs[l]):] == 0)
    assert Ws[3].shape == (249, 256)
    rows = 16 * np.arange(16)[:, None] + (np.arange(64) & 15)[None, :]      # [tile][lane] -> neuron
    assert np.all(Wp[2][(rows >= 249)[:, None, :].repeat(64, 1)] == 0) and np.all(bh[2, 249:] == 0) and np.any(bh[2, :249] != 0)


def test_pack_weights_bob_spot_is_unchanged():
    """The 128 / 2 packing, byte for byte, against the formula as the 128-only pack_weights stated it."""
    from diffsdfsim_amd.igr import pack_weights
    Ws, bs = IN.geometric_init(seed=3, radius_init=0.5, **IN.BOB_SPOT)
    bs = [b + 0.01 * np.arange(len(b)) for b in bs]
    P = pack_weights(Ws, bs, device="cpu")
    H = 128
    packed = np.zeros((7, 8, 32, 64)); bh = np.zeros((7, H)); lane = np.arange(64)
    for l in range(1, 8):
        W = np.zeros((H, H)); W[: Ws[l].shape[0]] = Ws[l]
        bh[l - 1, : len(bs[l])] = bs[l]
        for t in range(8):
            for ks in range(32):
                packed[l - 1, t, ks] = W[16 * t + (lane & 15), 4 * ks + (lane >> 4)]
    assert P["Wp"].numpy().tobytes() == packed.tobytes() and P["bh"].numpy().tobytes() == bh.tobytes()
    assert P["W0"].numpy().tobytes() == Ws[0].tobytes() and P["W8"].numpy().tobytes() == Ws[8][0].tobytes()
    assert P["b0"].numpy().tobytes() == bs[0].tobytes() and P["b8"].numpy().tobytes() == bs[8].tobytes()


def test_weights_from_module_accepts_both_shapes():
    from diffsdfsim_amd.igr import weights_from_module
    for shape in (IN.BOB_SPOT, IN.SHAPENET):
        Ws, bs = IN.geometric_init(seed=1, **shape)
        Wm, bm = weights_from_module(IN.torch_module(Ws, bs))
        assert all(np.array_equal(a, b) for a, b in zip(Wm, Ws)) and all(np.array_equal(a, b) for a, b in zip(bm, bs))


@pytest.mark.parametrize("name, shape", [
    ("width 64", dict(d_in=5, dims=[64] * 8, skip_in=(4,))),
    ("skip into layer 3", dict(d_in=5, dims=[128] * 8, skip_in=(3,))),
    ("ten layers", dict(d_in=5, dims=[128] * 9, skip_in=(4,))),
    ("latent 4 on width 128", dict(d_in=7, dims=[128] * 8, skip_in=(4,))),
])
def test_weights_from_module_refuses_other_shapes(name, shape):
    from diffsdfsim_amd.igr import pack_weights, weights_from_module
    Ws, bs = IN.geometric_init(seed=1, **shape)
    with pytest.raises(NotImplementedError):
        weights_from_module(IN.torch_module(Ws, bs))
    with pytest.raises(NotImplementedError):
        pack_weights(Ws, bs, device="cpu")


def _emu_query_list(Ws, bs, pts, latent, mode):
    """dss_igr_query_list of the CPU emulation build (tests/emu) on host arrays."""
    from emu import emu
    from diffsdfsim_amd import igr, world_abi
    L = emu.lib()
    P = {k: np.ascontiguousarray(v.numpy()) for k, v in igr.pack_weights(Ws, bs, device="cpu").items()}
    width, nlat = P["W0"].shape[0], P["W0"].shape[1] - 3
    net = world_abi.DssIgrNet(*[P[k].ctypes.data for k in world_abi.IGR_NET_POINTERS], width, nlat)
    pts = np.ascontiguousarray(pts, np.float64); n = len(pts)
    lat = np.zeros(max(nlat, 3)); lat[:nlat] = latent
    sdf = np.full(n, np.nan); grad = np.full((n, 4 if (mode == igr.MODE_LATENT and nlat > 3) else 3), np.nan)
    rc = L.dss_igr_query_list(ctypes.byref(net), pts.ctypes.data, None, lat.ctypes.data, len(lat), None, n, mode, sdf.ctypes.data,
                              grad.ctypes.data, None)
    assert rc == 0, rc
    return sdf, grad


def test_emu_shapenet_kernel_matches_numpy():
    """Logic of the (256, 4) instantiation -- 16 neuron tiles, 64 k-steps, the 7-wide skip, the two latent passes -- on seeded
    weights; 21 points: ragged for the 4-point tangent groups and the 16-point value groups alike."""
    from diffsdfsim_amd import igr
    Ws, bs = IN.geometric_init(seed=5, radius_init=0.6, **IN.SHAPENET)
    r = np.random.default_rng(1)
    pts = r.uniform(-1, 1, (21, 3)); lat = r.normal(0, 0.1, 4)
    v, gl, gx = IN.query(pts, lat, Ws, bs)
    sdf, grad = _emu_query_list(Ws, bs, pts, lat, igr.MODE_XYZ)
    assert np.abs(sdf - v).max() < 1e-12 and np.abs(grad - gx).max() < 1e-11
    sdf, grad = _emu_query_list(Ws, bs, pts, lat, igr.MODE_LATENT)
    assert grad.shape == (21, 4) and np.abs(sdf - v).max() < 1e-12 and np.abs(grad - gl).max() < 1e-11
    sdf, _ = _emu_query_list(Ws, bs, pts, lat, igr.MODE_VALUE)
    assert np.abs(sdf - v).max() < 1e-12


def test_emu_generic_entry_keeps_the_bob_spot_network():
    """dss_igr_query_list with width / latent spelled out, and with both left 0, is the 128 / 2 evaluation of dss_igr_query."""
    from emu import emu
    from diffsdfsim_amd import igr
    Ws, bs = IN.geometric_init(seed=3, **IN.BOB_SPOT)
    r = np.random.default_rng(2)
    pts = r.uniform(-1, 1, (13, 3)); lat = r.normal(0, 0.1, 2)
    for mode, wrt in ((igr.MODE_XYZ, "xyz"), (igr.MODE_LATENT, "latent")):
        sdf, grad = _emu_query_list(Ws, bs, pts, lat, mode)
        s0, g0 = emu.igr_query(pts, lat, Ws, bs, wrt=wrt)
        assert np.array_equal(sdf, s0) and np.array_equal(grad, g0)
