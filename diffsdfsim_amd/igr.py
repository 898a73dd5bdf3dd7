"""IGR neural SDF on the fp64 matrix cores (C ABI: dss_igr_query, dss_igr_query_list, csrc/igr_mlp.hip).

``pack_weights`` turns the nine Linear layers of the reference's ImplicitNet (PyTorch layout weight[out, in]) into
the operand set of the kernel: layer 0 and layer 8 stay dense, the seven H x H layers go into MFMA fragment order
``[tile t][k-step][lane] = W[16 t + (lane & 15)][4 ks + (lane >> 4)]`` so a wavefront fetches each B fragment with
one coalesced 512-byte load.  Layer 3 has H - (L + 3) outputs (the skip concat appends the L + 3 inputs): its missing
rows are zero.  Two shapes are built (``SHAPES``): hidden width 128 with a 2-number latent code (bob_spot_setup.conf) and
256 with 4 (shapenet.conf: can, mug, camera).  Real IGR checkpoints (`utils.py:310-320`) are not available offline; any
state_dict with the same shapes works.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .world_abi import IGR_NET_POINTERS, DssIgrNet

H = 128                                  # the bob_spot_setup width (dss_igr_query, dss_igr_query_latent_grad)
SHAPES = ((128, 2), (256, 4))            # (hidden width, latent size) the kernels are instantiated for
MODE_XYZ, MODE_LATENT, MODE_VALUE = 0, 1, 2      # DSS_IGR_*


def _refuse():
    return NotImplementedError("only the 5 -> 8 x 128 -> 1 and 7 -> 8 x 256 -> 1 networks with a skip connection into layer 4 "
                               "are built for the device")


def layer_shapes(width, latent):
    """weight[out, in] shapes of lin0 .. lin8 for hidden width `width` and latent size `latent`."""
    din = latent + 3
    return [(width, din)] + [(width - din if l == 3 else width, width) for l in range(1, 8)] + [(1, width)]


def net_shape(Ws):
    """(hidden width, latent size) of nine weight matrices; NotImplementedError unless it is one of SHAPES exactly."""
    if len(Ws) != 9:
        raise _refuse()
    width, latent = int(np.shape(Ws[0])[0]), int(np.shape(Ws[0])[1]) - 3
    if (width, latent) not in SHAPES or [tuple(np.shape(w)) for w in Ws] != layer_shapes(width, latent):
        raise _refuse()
    return width, latent


def packed_shape(P):
    """(hidden width, latent size) of a pack_weights result."""
    return int(P["W0"].shape[0]), int(P["W0"].shape[1]) - 3


def pack_weights(Ws, bs, device="cuda"):
    Ws = [np.asarray(w, np.float64) for w in Ws]
    bs = [np.asarray(b, np.float64) for b in bs]
    width, _latent = net_shape(Ws)
    tiles, ksteps = width // 16, width // 4
    packed = np.zeros((7, tiles, ksteps, 64))
    bh = np.zeros((7, width))
    lane = np.arange(64)
    rows = 16 * np.arange(tiles)[:, None, None] + (lane & 15)[None, None, :]
    cols = 4 * np.arange(ksteps)[None, :, None] + (lane >> 4)[None, None, :]
    for l in range(1, 8):
        W = np.zeros((width, width)); W[: Ws[l].shape[0]] = Ws[l]
        bh[l - 1, : len(bs[l])] = bs[l]
        packed[l - 1] = W[rows, cols]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
    return dict(W0=t(Ws[0]), b0=t(bs[0]), Wp=t(packed), bh=t(bh), W8=t(Ws[8][0]), b8=t(bs[8]))


def net_struct(P):
    """DssIgrNet of a pack_weights result (device pointers + the network's shape)."""
    return DssIgrNet(*[P[k].data_ptr() for k in IGR_NET_POINTERS], *packed_shape(P))


def igr_query_list(pts, latent, P, mode=MODE_XYZ):
    """One evaluation round through dss_igr_query_list, for either network shape: pts [n,3], latent [L] ->
    sdf [n] (MODE_VALUE), or (sdf, grad) with grad [n,3] = d sdf / d xyz (MODE_XYZ) or d sdf / d latent (MODE_LATENT:
    [n,3] = (d/d latent_0, d/d latent_1, 0) for L = 2, [n,4] for L = 4)."""
    _lib.require_device(pts, latent)
    L = _lib.lib()
    n = pts.shape[0]
    _width, nlat = packed_shape(P)
    lat = latent.reshape(-1)
    if lat.numel() != nlat:
        raise ValueError("this network takes a latent code of %d numbers, got %d" % (nlat, lat.numel()))
    stride = max(nlat, 3)
    row = torch.zeros(stride, dtype=torch.float64, device=pts.device)
    row[:nlat] = lat
    sdf = torch.empty(n, dtype=torch.float64, device=pts.device)
    grad = None if mode == MODE_VALUE else torch.empty(n, 4 if (mode == MODE_LATENT and nlat > 3) else 3, dtype=torch.float64, device=pts.device)
    net = net_struct(P)
    rc = L.dss_igr_query_list(ctypes.byref(net), _lib.ptr(pts.contiguous()), None, _lib.ptr(row), stride, None, int(n), int(mode),
                              _lib.ptr(sdf), _lib.ptr(grad) if grad is not None else None, _lib.stream_ptr(pts.device))
    _lib.check(rc, "dss_igr_query_list")
    return sdf if grad is None else (sdf, grad)


def igr_query(pts, latent, P, wrt="xyz"):
    """pts [n,3], latent [2] (float64, HIP device) -> sdf [n], d sdf / d xyz [n,3]
    (wrt="latent": [n,3] = d sdf / d latent_0, d sdf / d latent_1, 0).  With the 256-wide network: latent [4], and
    wrt="latent" gives [n,4]."""
    if packed_shape(P) != (H, 2):
        return igr_query_list(pts, latent, P, MODE_LATENT if wrt == "latent" else MODE_XYZ)
    _lib.require_device(pts, latent)
    L = _lib.lib()
    n = pts.shape[0]
    sdf = torch.empty(n, dtype=torch.float64, device=pts.device)
    grad = torch.empty(n, 3, dtype=torch.float64, device=pts.device)
    fn = L.dss_igr_query_latent_grad if wrt == "latent" else L.dss_igr_query
    rc = fn(_lib.ptr(pts.contiguous()), _lib.ptr(latent.contiguous()), _lib.ptr(P["W0"]), _lib.ptr(P["b0"]),
                         _lib.ptr(P["Wp"]), _lib.ptr(P["bh"]), _lib.ptr(P["W8"]), _lib.ptr(P["b8"]), int(n), _lib.ptr(sdf),
                         _lib.ptr(grad), _lib.stream_ptr(pts.device))
    _lib.check(rc, "dss_igr_query")
    return sdf, grad


def igr_values(pts, latent, P):
    """Values only (query_sdfs with return_grads=False): pts [n,3], latent [2] (or [4], 256-wide network) -> sdf [n].  A
    quarter of the matrix work of `igr_query` (no tangents) -- what sampling the 128^3 grid of a level-set mesh needs
    (bodies.py:657-664)."""
    return igr_query_list(pts, latent, P, MODE_VALUE)


def weights_from_module(network):
    """(Ws, bs) of an IGR ``ImplicitNet``-like torch module: attributes ``lin0 .. lin8`` (torch.nn.Linear), as the
    external IGR repository defines it and the reference loads it (`utils.py:300-320`).  Two shapes run on the device
    kernels: bob_spot_setup (IGR_data/train_configs/bob_spot_setup.conf:38-45: input 2 + 3, eight hidden layers of 128, skip
    at layer 4) and shapenet (IGR_data/train_configs/shapenet.conf: input 4 + 3, eight hidden layers of 256, skip at layer 4)."""
    Ws, bs = [], []
    for l in range(9):
        lin = getattr(network, "lin%d" % l, None)
        if lin is None:
            raise ValueError("decode_igr needs an ImplicitNet with layers lin0..lin8 (got %r)" % type(network))
        Ws.append(lin.weight.detach().cpu().double().numpy())
        bs.append(lin.bias.detach().cpu().double().numpy())
    if getattr(network, "lin9", None) is not None:
        raise _refuse()
    net_shape(Ws)
    return Ws, bs


class IgrNet:
    """A network on the device: packed weights for the kernels + the plain layers (host) for reference."""

    def __init__(self, Ws, bs, device="cuda"):
        self.Ws, self.bs = Ws, bs
        self.packed = pack_weights(Ws, bs, device)

    @classmethod
    def from_module(cls, network, device="cuda"):
        hit = getattr(network, "_dss_igr_net", None)
        if hit is None:
            hit = cls(*weights_from_module(network), device=device)
            try:
                network._dss_igr_net = hit       # pack once per network object
            except Exception:
                pass
        return hit


def decode_igr(network):
    """`decode_igr` (`sdf_physics/physics3d/utils.py:330-350`): network -> ``sdf(pts, latent)``.  The returned function
    evaluates on the device (dss_igr_query) and carries the packed network (``.igr``), which is how ``SDF3D`` recognises a
    neural SDF it can hand to the stepper's kernels."""
    net = network if isinstance(network, IgrNet) else IgrNet.from_module(network)

    def sdf(pts, latent, max_batch=32 ** 3):
        dev = net.packed["W0"].device
        p = torch.as_tensor(pts, dtype=torch.float64).to(dev).contiguous()
        lat = torch.as_tensor(latent, dtype=torch.float64).detach().to(dev).contiguous()
        return igr_query(p, lat, net.packed)[0]

    sdf.igr = net
    return sdf
