"""Pooled voxel grids on the device, for the depth camera and the point-cloud loss (include/depth_camera.h, include/pointcloud_loss.h).

    table = GridTable([sdf_a, sdf_b, ...])      # each [n0,n1,n2] float64, x slowest, n_d >= 2
    render_depth(..., grids=table, grid_id=...) / match_pointcloud(..., grids=table, grid_id=...)

The layout is the stepper's (DssWorld.grid_off / grid_dims / grid_data): `off` [ngrid] int32 offsets into `data`, `dims`
[ngrid,3] int32, `data` the samples one grid after the other.  The camera also wants the least sample over every block of
BLOCK cells per axis (dss_grid_block_min); `block_min()` computes them on first use and keeps them.

A table made of tensors of which at least one requires grad keeps the graph in `data` (the grids concatenated, undetached):
match_pointcloud then returns a loss that is differentiable w.r.t. those grids' samples.  Such a table holds the samples'
values of the moment it was made; after an optimiser's step make a new one.  Every other table is detached, as before.
"""
import numpy as np
import torch

from . import _lib

BLOCK = 4      # DSS_GRID_BLOCK


def block_counts(dims):
    """Blocks per grid: prod_d ceil((n_d - 1) / BLOCK), dims [ngrid,3]."""
    return np.prod(-(-(np.asarray(dims, np.int64).reshape(-1, 3) - 1) // BLOCK), axis=1)


class GridTable:
    def __init__(self, grids, device=None):
        gs = [torch.as_tensor(g, dtype=torch.float64) for g in grids]
        if not gs or any(g.dim() != 3 or min(g.shape) < 2 for g in gs):
            raise ValueError("grids: a non-empty list of [n0,n1,n2] arrays with at least two samples per axis")
        dev = torch.device(device) if device is not None else next((g.device for g in gs if g.is_cuda), torch.device("cuda"))
        sizes = [g.numel() for g in gs]
        if sum(sizes) > 2 ** 31 - 1:
            raise ValueError("grids: more than 2^31 - 1 samples in one table")
        self.ngrid = len(gs)
        self.shapes = [tuple(g.shape) for g in gs]
        dims = np.array(self.shapes, np.int32)
        self.off = torch.as_tensor(np.cumsum([0] + sizes[:-1]).astype(np.int32)).to(dev)
        self.dims = torch.as_tensor(dims).to(dev)
        if any(g.requires_grad for g in gs):
            # a grid that is being fitted: `data` keeps the graph to the grids it pools (match_pointcloud differentiates the loss
            # w.r.t. it, dss_pointcloud_loss_grids_adjoint); everything else reads its values
            self.data = torch.cat([g.to(dev).reshape(-1) for g in gs]).contiguous()
        else:
            self.data = torch.cat([g.detach().to(dev).reshape(-1) for g in gs]).contiguous()
        nblk = block_counts(dims)
        self.nblk = int(nblk.sum())
        self.blk_off = torch.as_tensor(np.concatenate([[0], np.cumsum(nblk)[:-1]]).astype(np.int32)).to(dev)
        self._blk_min = None
        self.device = dev

    @classmethod
    def from_pooled(cls, dims, data):
        """The table of grids already pooled on the device (an engine's grid_dims [ngrid,3] and grid_data)."""
        shapes = [tuple(int(x) for x in d) for d in torch.as_tensor(dims).cpu().reshape(-1, 3).tolist()]
        flat = data.reshape(-1)
        views, at = [], 0
        for s in shapes:
            views.append(flat[at:at + s[0] * s[1] * s[2]].reshape(s)); at += s[0] * s[1] * s[2]
        return cls(views, data.device)

    def block_min(self):
        """[nblk] float64: per block the least of its corner samples, grid after grid, x slowest (dss_grid_block_min)."""
        if self._blk_min is None:
            L = _lib.lib()
            out = torch.empty(self.nblk, dtype=torch.float64, device=self.device)
            _lib.check(L.dss_grid_block_min(self.ngrid, _lib.ptr(self.off), _lib.ptr(self.dims), _lib.ptr(self.data.detach()), _lib.ptr(self.blk_off),
                                            self.nblk, _lib.ptr(out), _lib.stream_ptr(self.device)), "dss_grid_block_min")
            self._blk_min = out
        return self._blk_min

    def ids(self, grid_id, shape, device):
        """grid_id as a contiguous int32 device tensor of `shape`, every entry checked against the table on the host."""
        ids = torch.as_tensor(grid_id).to("cpu", torch.int32).reshape(shape)
        if bool((ids >= self.ngrid).any()):
            raise ValueError("grid_id: entries must be < %d (the table's grids) or negative for none" % self.ngrid)
        return ids.to(device).contiguous()


def as_table(grids, device=None):
    return grids if isinstance(grids, GridTable) else GridTable(grids, device)


def table_and_ids(grids, grid_id, shape, device, axes):
    """What a call with grids= passes on -> (as_table(grids), its checked ids of `shape` on the device).  axes: the shape in words
    for the error ("nview,nbody", "nseg")."""
    if grid_id is None:
        raise ValueError("grids= needs grid_id [%s] (-1: no grid there)" % axes)
    T = as_table(grids, device)
    return T, T.ids(grid_id, shape, device)
