"""Point-cloud loss on the device: `match_pointcloud` of experiments/trajectory_fitting/optim_pointcloud.py:166-201 for a batch
of (scene, observed frame) segments in one call of dss_pointcloud_loss (csrc/pointcloud_loss.hip).

    loss_sum, count = match_pointcloud(pts, seg_off, pose, shape_type, prm)

`pts` [N,3] world-frame points, `seg_off` [nseg+1] int offsets (segment s owns pts[seg_off[s]:seg_off[s+1]]), `pose` [nseg,7]
(quaternion wxyz + position), `shape_type` [nseg] int32, `prm` [nseg,4] (three shape parameters + the corner radius, a constant
of the body).  loss_sum[s] = sum of sdf(R(q)^T (x - pos))^2 over the segment's points inside the body's query cube, count[s] =
how many those are.  Differentiable w.r.t. `pose` and `prm[:, :3]`: the kernel returns the Jacobian with the value, backward
is a multiply.  Device tensors only.

Voxel-grid bodies (shape type 7): pass `grids=` (a grids.GridTable or a list of [n0,n1,n2] arrays) and `grid_id` [nseg] (-1: none);
the call is then dss_pointcloud_loss_grids.  A grid segment's value is the trilinear field times prm[:, 3] (the scale), its pose
Jacobian follows the reference's DiffGridSDF rule, and its prm gradient is zero.  Where a grid of the table requires grad (a
GridTable made of such tensors keeps their graph in `data`), the loss is also differentiable w.r.t. the samples: the value is
linear in the 8 samples of a point's cell, d loss_sum / d sample_c = sum over the points of 2 phi scale w_c, and backward adds
those terms with dss_pointcloud_loss_grids_adjoint (csrc/pointcloud_loss_grid_adj.hip; fp64 atomic adds, so two backward passes
agree to the rounding of each sample's sum, not in bits).  The forward is the same call and returns the same bits; the scale stays a
constant.  With no grid requiring grad nothing differs from before.

Neural bodies (shape type 6, SDF3D with decode_igr): pass `igr=` (a pack_weights result or an IgrNet), `latent` [n_lat, L] and
`latent_id` [nseg] (-1: not neural).  Those segments take prm[:, 3] as the scale and go to dss_pointcloud_loss_igr
(csrc/pointcloud_loss_igr.hip: the points inside the query cube are compacted and the network runs over them alone); the loss
differentiates through the network itself, as the reference's autograd does with query_sdfs(return_grads=False), and is
differentiable w.r.t. `pose` and `latent` (prm gets zero).  All other segments go, as a subset with their own points, to the call
they use without neural segments, so their results are the same bits; the rows are scattered back to [nseg].  That call waits for
the stream once (it reads the length of the compacted list), so it cannot be captured into a graph.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .world_abi import SHAPE_IGR

OUT = 12      # sum, count, d / d pose [7], d / d prm [3]
OUT_IGR = 13  # DSS_PC_IGR_OUT: sum, count, d / d pose [7], d / d latent [4]


def _launch(pts, seg_off, max_len, pose, shape_type, prm, grids=None, grid_id=None):
    """grids: a grids.GridTable with grid_id [nseg] int32 on the device (dss_pointcloud_loss_grids), or None."""
    nseg = pose.shape[0]
    L = _lib.lib()
    name = "dss_pointcloud_loss" if grids is None else "dss_pointcloud_loss_grids"
    out = torch.zeros(nseg, OUT, dtype=torch.float64, device=pose.device)
    nbytes = L.dss_pointcloud_loss_workspace_bytes(nseg, max_len)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=pose.device)
    if grids is None:
        rc = L.dss_pointcloud_loss(nseg, max_len, _lib.ptr(seg_off), _lib.ptr(pts), _lib.ptr(pose), _lib.ptr(shape_type), _lib.ptr(prm),
                                   _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(pose.device))
    else:
        rc = L.dss_pointcloud_loss_grids(nseg, max_len, _lib.ptr(seg_off), _lib.ptr(pts), _lib.ptr(pose), _lib.ptr(shape_type), _lib.ptr(prm),
                                         _lib.ptr(grid_id), grids.ngrid, _lib.ptr(grids.off), _lib.ptr(grids.dims), _lib.ptr(grids.data),
                                         _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(pose.device))
    _lib.check(rc, name)
    return out


class _MatchPointcloud(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, seg_off, max_len, pose, shape_type, prm, grids=None, grid_id=None):
        out = _launch(pts, seg_off, max_len, pose.detach().contiguous(), shape_type, prm.detach().contiguous(), grids, grid_id)
        ctx.save_for_backward(out)
        count = out[:, 1].clone()
        ctx.mark_non_differentiable(count)
        return out[:, 0].clone(), count

    @staticmethod
    def backward(ctx, g_sum, _g_count):
        out, = ctx.saved_tensors
        g = g_sum[:, None]
        g_prm = torch.cat([g * out[:, 9:12], out.new_zeros(out.shape[0], 1)], 1)      # the corner radius is a constant
        return None, None, None, g * out[:, 2:9], None, g_prm, None, None


def _launch_grids_adjoint(pts, seg_off, max_len, pose, shape_type, prm, ngrid, grid_off, grid_dims, grid_data, grid_id, g_sum):
    """dss_pointcloud_loss_grids_adjoint: -> g_data, pooled like grid_data (zeroed here, the call adds into it)."""
    L = _lib.lib()
    g_data = torch.zeros_like(grid_data)
    rc = L.dss_pointcloud_loss_grids_adjoint(pose.shape[0], max_len, _lib.ptr(seg_off), _lib.ptr(pts), _lib.ptr(pose), _lib.ptr(shape_type),
                                             _lib.ptr(prm), _lib.ptr(grid_id), ngrid, _lib.ptr(grid_off), _lib.ptr(grid_dims), _lib.ptr(grid_data),
                                             _lib.ptr(g_sum), _lib.ptr(g_data), _lib.stream_ptr(pose.device))
    _lib.check(rc, "dss_pointcloud_loss_grids_adjoint")
    return g_data


class _MatchPointcloudGridData(torch.autograd.Function):
    """_MatchPointcloud with the table's samples as an input of the graph: `grid_data` is grids.data (a table made of grids that
    require grad).  The forward is the same call on the same memory; the backward adds the samples' gradient."""

    @staticmethod
    def forward(ctx, pts, seg_off, max_len, pose, shape_type, prm, grids, grid_id, grid_data):
        pose_c, prm_c = pose.detach().contiguous(), prm.detach().contiguous()
        out = _launch(pts, seg_off, max_len, pose_c, shape_type, prm_c, grids, grid_id)
        ctx.save_for_backward(out, pts, seg_off, pose_c, shape_type, prm_c, grids.off, grids.dims, grid_id, grid_data)
        ctx.max_len, ctx.ngrid = max_len, grids.ngrid
        count = out[:, 1].clone()
        ctx.mark_non_differentiable(count)
        return out[:, 0].clone(), count

    @staticmethod
    def backward(ctx, g_sum, _g_count):
        out, pts, seg_off, pose, shape_type, prm, grid_off, grid_dims, grid_id, grid_data = ctx.saved_tensors
        g = g_sum[:, None]
        g_prm = torch.cat([g * out[:, 9:12], out.new_zeros(out.shape[0], 1)], 1)      # the corner radius is a constant
        g_data = None
        if ctx.needs_input_grad[8]:
            g_data = _launch_grids_adjoint(pts, seg_off, ctx.max_len, pose, shape_type, prm, ctx.ngrid, grid_off, grid_dims, grid_data, grid_id,
                                           g_sum.detach().to(torch.float64).contiguous())
        return None, None, None, g * out[:, 2:9], None, g_prm, None, None, g_data


def _match_grids(pts, seg_off, max_len, pose, shape_type, prm, table, grid_id):
    """The loss with a grid table: through the samples' graph where the table carries one, else the call as it always was."""
    if table is not None and table.data.requires_grad:
        return _MatchPointcloudGridData.apply(pts, seg_off, max_len, pose, shape_type, prm, table, grid_id, table.data)
    return _MatchPointcloud.apply(pts, seg_off, max_len, pose, shape_type, prm, table, grid_id)


class NeuralSegmentError(_lib.HipLibraryError, ValueError):
    """A neural segment without igr= / latent= / latent_id=.  A ValueError that names the missing argument; also the
    HipLibraryError that match_pointcloud raised for every neural segment while the loss had no network in it."""


def _launch_igr(pts, seg_off, max_len, pose, scale, packed, latent, lat_idx):
    """dss_pointcloud_loss_igr: pose [nseg,7], scale [nseg], latent [n_lat, L] (contiguous), lat_idx [nseg] int32 -> out [nseg,13]."""
    from .igr import net_struct
    nseg, n_pts = pose.shape[0], pts.shape[0]
    L = _lib.lib()
    out = torch.zeros(nseg, OUT_IGR, dtype=torch.float64, device=pose.device)
    nbytes = L.dss_pointcloud_loss_igr_workspace_bytes(nseg, max_len, n_pts)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=pose.device)
    net = net_struct(packed)
    rc = L.dss_pointcloud_loss_igr(ctypes.byref(net), nseg, max_len, _lib.ptr(seg_off), _lib.ptr(pts), _lib.ptr(pose), _lib.ptr(scale),
                                   _lib.ptr(lat_idx), _lib.ptr(latent), latent.shape[1], n_pts, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                   _lib.stream_ptr(pose.device))
    _lib.check(rc, "dss_pointcloud_loss_igr")
    return out


class _MatchPointcloudIgr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, seg_off, max_len, pose, scale, packed, latent, lat_idx):
        out = _launch_igr(pts, seg_off, max_len, pose.detach().contiguous(), scale, packed, latent.detach().contiguous(), lat_idx)
        ctx.save_for_backward(out, lat_idx)
        ctx.lat_shape = tuple(latent.shape)
        count = out[:, 1].clone()
        ctx.mark_non_differentiable(count)
        return out[:, 0].clone(), count

    @staticmethod
    def backward(ctx, g_sum, _g_count):
        out, lat_idx = ctx.saved_tensors
        g = g_sum[:, None]
        g_lat = out.new_zeros(ctx.lat_shape).index_add_(0, lat_idx.to(torch.int64), g * out[:, 9:9 + ctx.lat_shape[1]])
        return None, None, None, g * out[:, 2:9], None, None, g_lat, None


def _subset(pts, off, ids, dev):
    """The points and offsets of the segments `ids` (host int64 array) packed in that order: pts', off' (host), max_len."""
    lens = (off[1:] - off[:-1])[ids]
    sub = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    rows = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in ids] + [torch.zeros(0, dtype=torch.int64)])
    return pts[rows.to(dev)].contiguous(), sub, int(lens.max()) if len(ids) else 0


def _match_with_neural(pts, off, pose, types, prm, grids, grid_id, igr, latent, latent_id, neural):
    from .igr import IgrNet, packed_shape
    dev, nseg = pose.device, pose.shape[0]
    for name, v in (("igr", igr), ("latent", latent), ("latent_id", latent_id)):
        if v is None:
            raise NeuralSegmentError("a segment of shape type %d (a neural body) needs %s=" % (SHAPE_IGR, name))
    packed = igr.packed if isinstance(igr, IgrNet) else igr
    L = packed_shape(packed)[1]
    if latent.dim() != 2 or latent.shape[1] != L or latent.dtype != torch.float64:
        raise ValueError("latent [n_lat, %d] as float64 for this network, got %s" % (L, tuple(latent.shape)))
    lid = torch.as_tensor(latent_id).detach().to("cpu", torch.int64).reshape(-1)
    if lid.numel() != nseg or bool((lid[neural] < 0).any()) or bool((lid[neural] >= latent.shape[0]).any()):
        raise ValueError("latent_id: [nseg] rows of latent, one in range for every neural segment (-1 for the others)")
    ids_n, ids_o = torch.nonzero(neural).reshape(-1), torch.nonzero(~neural).reshape(-1)
    loss = torch.zeros(nseg, dtype=torch.float64, device=dev)
    count = torch.zeros(nseg, dtype=torch.float64, device=dev)
    p_n, off_n, max_n = _subset(pts, off, ids_n, dev) if len(ids_o) else (pts, off - off[0], int((off[1:] - off[:-1]).max()))
    if len(ids_o) == 0 and int(off[0]) != 0:
        p_n = pts[int(off[0]):].contiguous()
    dn = ids_n.to(dev)
    s, n = _MatchPointcloudIgr.apply(p_n, off_n.to(dev, torch.int32), max_n, pose[dn], prm[dn, 3].detach().contiguous(), packed,
                                     latent.to(dev), lid[ids_n].to(dev, torch.int32))
    loss, count = loss.index_copy(0, dn, s), count.index_copy(0, dn, n)
    if len(ids_o):
        p_o, off_o, max_o = _subset(pts, off, ids_o, dev)
        do = ids_o.to(dev)
        T = gid = None
        if grids is not None:
            from .grids import table_and_ids
            T, gid = table_and_ids(grids, grid_id, (nseg,), dev, "nseg")
            gid = gid[do].contiguous()
        s, n = _match_grids(p_o, off_o.to(dev, torch.int32), max_o, pose[do], types[do].contiguous(), prm[do], T, gid)
        loss, count = loss.index_copy(0, do, s), count.index_copy(0, do, n)
    return loss, count.detach()


def match_pointcloud(pts, seg_off, pose, shape_type, prm, grids=None, grid_id=None, igr=None, latent=None, latent_id=None):
    """-> (loss_sum [nseg], count [nseg]), both float64 on the device of `pose`; see the module's text for the arguments."""
    _lib.require_device(pts, pose, prm)
    dev = pose.device
    nseg = pose.shape[0]
    if pose.shape != (nseg, 7) or prm.shape != (nseg, 4) or pose.dtype != torch.float64 or prm.dtype != torch.float64:
        raise ValueError("pose [nseg,7] and prm [nseg,4] as float64, got %s and %s" % (tuple(pose.shape), tuple(prm.shape)))
    off = torch.as_tensor(seg_off).detach().to("cpu", torch.int64).reshape(-1)
    if off.numel() != nseg + 1 or bool((off[1:] < off[:-1]).any()) or int(off[0]) < 0 or int(off[-1]) > pts.shape[0]:
        raise ValueError("seg_off: nseg + 1 ascending offsets into pts")
    max_len = int((off[1:] - off[:-1]).max()) if nseg else 0
    pts = pts.detach().to(torch.float64).contiguous().reshape(-1, 3)
    off_d = off.to(dev, torch.int32)
    types = torch.as_tensor(shape_type).to(dev, torch.int32).reshape(nseg).contiguous()
    neural = torch.as_tensor(shape_type).detach().to("cpu", torch.int64).reshape(nseg) == SHAPE_IGR
    if bool(neural.any()):
        return _match_with_neural(pts, off, pose, types, prm, grids, grid_id, igr, latent, latent_id, neural)
    if grids is None:
        return _MatchPointcloud.apply(pts, off_d, max_len, pose, types, prm, None, None)
    from .grids import table_and_ids
    return _match_grids(pts, off_d, max_len, pose, types, prm, *table_and_ids(grids, grid_id, (nseg,), dev, "nseg"))
