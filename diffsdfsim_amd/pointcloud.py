"""Point-cloud loss on the device: `match_pointcloud` of experiments/trajectory_fitting/optim_pointcloud.py:166-201 for a batch
of (scene, observed frame) segments in one call of dss_pointcloud_loss (csrc/pointcloud_loss.hip).

    loss_sum, count = match_pointcloud(pts, seg_off, pose, shape_type, prm)

`pts` [N,3] world-frame points, `seg_off` [nseg+1] int offsets (segment s owns pts[seg_off[s]:seg_off[s+1]]), `pose` [nseg,7]
(quaternion wxyz + position), `shape_type` [nseg] int32, `prm` [nseg,4] (three shape parameters + the corner radius, a constant
of the body).  loss_sum[s] = sum of sdf(R(q)^T (x - pos))^2 over the segment's points inside the body's query cube, count[s] =
how many those are.  Differentiable w.r.t. `pose` and `prm[:, :3]`: the kernel returns the Jacobian with the value, backward
is a multiply.  Device tensors only; analytic primitives only (a neural or grid body raises).

Voxel-grid bodies (shape type 7): pass `grids=` (a grids.GridTable or a list of [n0,n1,n2] arrays) and `grid_id` [nseg] (-1: none);
the call is then dss_pointcloud_loss_grids.  A grid segment's value is the trilinear field times prm[:, 3] (the scale), its pose
Jacobian follows the reference's DiffGridSDF rule, and its prm gradient is zero.  A neural body still raises.
"""
import numpy as np
import torch

from . import _lib

OUT = 12      # sum, count, d / d pose [7], d / d prm [3]


def _launch(pts, seg_off, max_len, pose, shape_type, prm, grids=None, grid_id=None):
    """grids: a grids.GridTable with grid_id [nseg] int32 on the device (dss_pointcloud_loss_grids), or None."""
    nseg = pose.shape[0]
    L = _lib.lib()
    name = "dss_pointcloud_loss" if grids is None else "dss_pointcloud_loss_grids"
    if not hasattr(L, name):      # (declared in csrc/pointcloud_loss.h, outside the public header's table)
        raise _lib.HipLibraryError("libdiffsdfsim_hip.so does not export %s: rebuild it (python __graft_entry__.py build)" % name)
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


def match_pointcloud(pts, seg_off, pose, shape_type, prm, grids=None, grid_id=None):
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
    if grids is None:
        return _MatchPointcloud.apply(pts, off_d, max_len, pose, types, prm, None, None)
    from .grids import as_table
    if grid_id is None:
        raise ValueError("grids= needs grid_id [nseg] (-1: the segment's body has no grid)")
    T = as_table(grids, dev)
    return _MatchPointcloud.apply(pts, off_d, max_len, pose, types, prm, T, T.ids(grid_id, (nseg,), dev))
