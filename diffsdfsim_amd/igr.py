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
from .world_abi import IGR_LATENT_MAX, IGR_NET_POINTERS, DssIgrNet

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


def igr_grid_adjoint(g_grid, dims, lat_idx, latents, P, cap=None, return_nodes=False):
    """The chain from value grids to latent codes (dss_igr_grid_adjoint, csrc/igr_grid_adjoint.h): g_grid, the adjoint of the
    values of `ngrid` lattices over [-1, 1]^3 pooled one after the other (x slowest, float64 on the device); dims [ngrid,3]; lat_idx
    [ngrid] the row of `latents` [nlat,L] whose code grid g was sampled with (< 0: not a neural grid, skipped).
    -> g_latent [nlat,L] = sum over a row's grids and their nodes of g_grid * d f / d latent, bit-reproducible.  Only the
    non-zero nodes reach the network: `cap` is the capacity of their list (default max(4096, samples // 16)); a list that
    does not fit costs one more call with the capacity the first one reported.  return_nodes: also the number of nodes."""
    _lib.require_device(g_grid, latents)
    fn, size = getattr(_lib.lib(), "dss_igr_grid_adjoint", None), getattr(_lib.lib(), "dss_igr_grid_adjoint_workspace_bytes", None)
    if fn is None or size is None:
        raise _lib.HipLibraryError("the library does not export dss_igr_grid_adjoint: rebuild it (python __graft_entry__.py build)")
    dev = g_grid.device
    dims = np.asarray(dims, np.int64).reshape(-1, 3)
    sizes = dims.prod(1)
    ngrid, nsamples = len(dims), int(sizes.sum())
    g = g_grid.detach().to(torch.float64).contiguous().reshape(-1)
    _width, nlat = packed_shape(P)
    lat = latents.detach().to(torch.float64).reshape(-1, nlat)
    rows = np.asarray(lat_idx, np.int64).reshape(-1)
    if g.numel() != nsamples or len(rows) != ngrid or nsamples > 2 ** 31 - 1 or dims.min() < 2 or rows.max() >= lat.shape[0]:
        raise ValueError("g_grid pools the samples of dims (each >= 2, below 2^31 together) and lat_idx names a row of latents per grid: "
                         "dims has %d grids of %d samples together, g_grid %d samples, lat_idx %d entries (largest %d), latents %d rows"
                         % (ngrid, nsamples, g.numel(), len(rows), int(rows.max()) if len(rows) else -1, lat.shape[0]))
    table = torch.zeros(lat.shape[0], IGR_LATENT_MAX, dtype=torch.float64, device=dev)
    table[:, :nlat] = lat
    off = torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)).to(dev)
    dims_d, rows_d = torch.as_tensor(dims.astype(np.int32)).to(dev).contiguous(), torch.as_tensor(rows.astype(np.int32)).to(dev)
    out = torch.zeros(lat.shape[0], IGR_LATENT_MAX, dtype=torch.float64, device=dev)
    n_nodes = torch.zeros(1, dtype=torch.int32, device=dev)
    net = net_struct(P)
    cap = max(4096, nsamples // 16) if cap is None else int(cap)
    # the size function bounds the chunks (2048 samples of one grid) by the samples alone, nsamples / 2048 + nsamples / 8 + 1, and the
    # call checks the workspace against the chunks the tables name: asking for 8 samples per chunk covers those and no more
    nchunk = int((-(-sizes[rows >= 0] // 2048)).sum())
    for attempt in (0, 1):
        nbytes = size(max(min(nsamples, 8 * nchunk), 1), cap, lat.shape[0])
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        rc = fn(ctypes.byref(net), ngrid, _lib.ptr(off), _lib.ptr(dims_d), _lib.ptr(rows_d), _lib.ptr(table), IGR_LATENT_MAX, lat.shape[0],
                _lib.ptr(g), cap, _lib.ptr(out), _lib.ptr(n_nodes), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        if rc != -2 or attempt or int(n_nodes) <= cap:      # DSS_E_WORKSPACE with n_nodes > cap: the list did not fit
            break
        cap = int(n_nodes)
    _lib.check(rc, "dss_igr_grid_adjoint")
    return (out[:, :nlat], int(n_nodes)) if return_nodes else out[:, :nlat]


class _IgrLatticeValues(torch.autograd.Function):
    """igr_values on the res^3 lattice (forward: one network launch per row of the batch, so that each grid has igr_values' bits)
    with a backward by dss_igr_grid_adjoint, one call for all the grids of a batch."""

    @staticmethod
    def forward(ctx, latent, P, res):
        from .meshsdf import _grid_cached
        dev = P["W0"].device
        lat = latent.detach().to(torch.float64).to(dev).reshape(-1, packed_shape(P)[1])
        pts = _grid_cached(res, dev)
        vals = torch.stack([igr_values(pts, row, P).reshape(res, res, res) for row in lat])
        ctx.save_for_backward(lat)
        ctx.P, ctx.res, ctx.like = P, res, (latent.shape, latent.device, latent.dtype)
        return vals if latent.dim() == 2 else vals[0]

    @staticmethod
    def backward(ctx, g):
        (lat,) = ctx.saved_tensors
        B, res = lat.shape[0], ctx.res
        out = igr_grid_adjoint(g.to(lat.device), [[res] * 3] * B, np.arange(B), lat, ctx.P)
        shape, ldev, dtype = ctx.like
        return out.reshape(shape).to(ldev, dtype), None, None


def igr_lattice_values(latent, P, res):
    """The network's values on the res^3 lattice of meshsdf._grid(res), differentiable w.r.t. the latent code: latent [L] ->
    [res,res,res] (the bits of igr_values on that lattice, what depth_camera.body_grid returns), latent [B,L] -> [B,res,res,res].
    The forward pass is one igr_values launch per code; the backward pass is igr_grid_adjoint: one call for the whole batch, over the nodes whose adjoint is not zero -- a depth
    image or a point cloud touches a small part of the lattice.  Float64, on the device of the packed network."""
    latent = torch.as_tensor(latent)
    nlat = packed_shape(P)[1]
    if latent.dim() not in (1, 2) or latent.shape[-1] != nlat or int(res) < 2:
        raise ValueError("latent [%d] or [B,%d] and res >= 2, got %s and %r" % (nlat, nlat, tuple(latent.shape), res))
    return _IgrLatticeValues.apply(latent, P, int(res))


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
