"""Chamfer distance of vertex clouds on the device, for a batch of scenes in one call, with its gradient: what every experiment
of the reference logs per iteration as `pytorch3d.loss.chamfer_distance(obj.verts, obj_target.verts)` (optim_sphere.py:244), by
the nearest-neighbour kernel of csrc/chamfer.hip (ABI: include/chamfer.h).

    d2, idx = nearest(q, q_off, r, r_off)              # per query: squared distance to, and row of, its segment's nearest point
    c = chamfer_packed(a, a_off, b, b_off)             # [B], differentiable w.r.t. a and b
    c = chamfer_batch(a_list, b_list)                  # the same from lists of [N_s,3] arrays or tensors of any device

Clouds are packed: scene s owns a[a_off[s]:a_off[s+1]] and b[b_off[s]:b_off[s+1]].  Per scene the value is
mean_i min_j |a_i - b_j|^2 + mean_j min_i |a_i - b_j|^2, chamfer_distance's defaults (squared distances, mean over the points,
the two directions summed); the mean over the batch is left to the caller.  Distances are evaluated as (ax-bx)^2 + (ay-by)^2 +
(az-bz)^2, never as |a|^2 + |b|^2 - 2 a.b, so clouds far from the origin keep their relative accuracy.  Device tensors only.
"""
import numpy as np
import torch

from . import _lib

# the launch shape of csrc/chamfer.hip (include/chamfer.h: DSS_CHAMFER_*), for callers and tests that pick sizes from it
TILE = 512             # reference points per LDS tile
QUERIES = 512          # query points per workgroup
SPLIT_TILES = 2        # the fewest tiles a split of the reference range is given
TARGET_WG = 2048       # workgroups the launcher aims at before it stops splitting


def splits(nseg, max_q_len, max_r_len):
    """The number of workgroups the launcher divides a segment's reference range among (include/chamfer.h); above 1 the partial
    minima go through the workspace and the merge kernel."""
    qblocks, tiles = -(-max_q_len // QUERIES), -(-max_r_len // TILE)
    return max(1, min(-(-tiles // SPLIT_TILES), -(-TARGET_WG // (nseg * max(qblocks, 1)))))


def _cloud(x, name, fn):
    if not torch.is_tensor(x):
        raise TypeError("%s: a torch tensor on a HIP device" % name)
    if not x.is_cuda:
        raise _lib.HipLibraryError("%s needs tensors on a HIP device (got %s); there is no CPU fallback" % (fn, x.device))
    if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float64:
        raise ValueError("%s [N,3] float64, got %s %s" % (name, tuple(x.shape), x.dtype))


def _offsets(off, n, name):
    off = torch.as_tensor(off).detach().to("cpu", torch.int64).reshape(-1)
    if off.numel() < 2 or bool((off[1:] < off[:-1]).any()) or int(off[0]) < 0 or int(off[-1]) > n or int(off[-1]) > 2 ** 31 - 1:
        raise ValueError("%s: nseg + 1 >= 2 ascending offsets into its cloud (below 2^31)" % name)
    return off


def nearest(q, q_off, r, r_off):
    """For every query point of q [Nq,3] the nearest reference point of the same segment in r [Nr,3] (float64 on the device;
    segment s owns q[q_off[s]:q_off[s+1]] and r[r_off[s]:r_off[s+1]], offsets ascending, nseg + 1 long).
    -> (d2 [Nq] float64: the squared distance, idx [Nq] int32: the row in r; of equal distances the lowest row).  A query whose
    segment has no reference point gets +inf and -1; rows of q outside every segment get 0 and -1.  The inputs are finite (not
    checked).  Not differentiable by itself (chamfer_packed is); two calls return the same bits."""
    _cloud(q, "q", "nearest"); _cloud(r, "r", "nearest")
    if q.device != r.device:
        raise ValueError("q and r on one device, got %s and %s" % (q.device, r.device))
    qo, ro = _offsets(q_off, q.shape[0], "q_off"), _offsets(r_off, r.shape[0], "r_off")
    if qo.numel() != ro.numel():
        raise ValueError("q_off and r_off: the same number of segments, got %d and %d" % (qo.numel() - 1, ro.numel() - 1))
    nseg, dev = qo.numel() - 1, q.device
    if q.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    max_q, max_r = int((qo[1:] - qo[:-1]).max()), int((ro[1:] - ro[:-1]).max())
    fn, nbytes = _lib.lib().dss_chamfer_nn, _lib.lib().dss_chamfer_nn_workspace_bytes(nseg, max_q, max_r)
    ws = torch.empty(max(nbytes // 8 + 1, 1), dtype=torch.float64, device=dev)
    d2 = torch.zeros(q.shape[0], dtype=torch.float64, device=dev)
    idx = torch.full((q.shape[0],), -1, dtype=torch.int32, device=dev)
    qo_d, ro_d, q, r = qo.to(dev, torch.int32), ro.to(dev, torch.int32), q.detach().contiguous(), r.detach().contiguous()
    _lib.check(fn(nseg, max_q, max_r, _lib.ptr(qo_d), _lib.ptr(q), _lib.ptr(ro_d), _lib.ptr(r), _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(ws),
                  nbytes, _lib.stream_ptr(dev)), "dss_chamfer_nn")
    return d2, idx


def _segment_mean(v, off):
    """out [nseg]: the mean of v[off[s]:off[s+1]] in a fixed order (dss_chamfer_segment_mean); NaN for an empty segment."""
    nseg = off.numel() - 1
    out = torch.full((nseg,), float("nan"), dtype=torch.float64, device=v.device)
    if v.numel():
        off_d = off.to(v.device, torch.int32)
        _lib.check(_lib.lib().dss_chamfer_segment_mean(nseg, _lib.ptr(off_d), _lib.ptr(v), _lib.ptr(out), _lib.stream_ptr(v.device)),
                   "dss_chamfer_segment_mean")
    return out


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, a_off, b_off):
        d_ab, i_ab = nearest(a, a_off, b, b_off)
        d_ba, i_ba = nearest(b, b_off, a, a_off)
        out = _segment_mean(d_ab, a_off) + _segment_mean(d_ba, b_off)
        ctx.save_for_backward(a, b, i_ab, i_ba)
        ctx.off = (a_off, b_off)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, i_ab, i_ba = ctx.saved_tensors
        dev = a.device
        ga, gb = torch.zeros_like(a), torch.zeros_like(b)

        def one_way(x, off, y, nn, gx, gy):      # the terms of mean_i |x_i - y_nn(i)|^2: 2 (x_i - y_nn(i)) / N_s to x_i, the opposite to y_nn(i)
            n = (off[1:] - off[:-1])
            w = (g / n.to(dev, torch.float64)).repeat_interleave(n.to(dev), output_size=int(n.sum()))      # (an empty scene has no rows)
            rows = torch.arange(int(off[0]), int(off[-1]), device=dev)
            j = nn[rows].long()
            ok = j >= 0                                   # (-1: the scene's other cloud is empty, the value is NaN; no rows to read)
            rows, j, w = rows[ok], j[ok], w[ok]
            t = 2.0 * (x[rows] - y[j]) * w[:, None]
            gx.index_add_(0, rows, t)
            gy.index_add_(0, j, -t)
        one_way(a, ctx.off[0], b, i_ab, ga, gb)
        one_way(b, ctx.off[1], a, i_ba, gb, ga)
        return ga, gb, None, None


def chamfer_packed(a, a_off, b, b_off):
    """Chamfer distance per scene of the packed clouds a [Na,3], b [Nb,3] (float64 on the device; scene s owns
    a[a_off[s]:a_off[s+1]] and b[b_off[s]:b_off[s+1]]) -> [B] float64 on the device:
    mean_i min_j |a_i - b_j|^2 + mean_j min_i |a_i - b_j|^2; NaN for a scene one of whose clouds is empty.  Two searches
    (nearest: a in b, b in a) and two per-scene means in a fixed order: two calls return the same bits.
    Differentiable w.r.t. a and b with the nearest neighbours held fixed (as pytorch3d's is): a_i receives 2 (a_i - b_nn(i)) / Na_s
    and, for every b_j whose nearest neighbour it is, 2 (a_i - b_j) / Nb_s; b mirrored.  The backward pass scatters with
    index_add_, whose order of summation, and so the last bits of a gradient row that several terms reach, may vary between calls."""
    _cloud(a, "a", "chamfer_packed"); _cloud(b, "b", "chamfer_packed")
    ao, bo = _offsets(a_off, a.shape[0], "a_off"), _offsets(b_off, b.shape[0], "b_off")
    return _Chamfer.apply(a, b, ao, bo)


def pack(clouds, device=None):
    """A list of [N_s,3] arrays or tensors of any device -> (packed [N,3] float64 on `device` (default: the current HIP device),
    offsets [B+1] int64 on the host).  A tensor's graph is kept."""
    dev = torch.device("cuda" if device is None else device)
    ts = [(c if torch.is_tensor(c) else torch.as_tensor(np.ascontiguousarray(c, dtype=np.float64))).to(dev, torch.float64).reshape(-1, 3)
          for c in clouds]
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([t.shape[0] for t in ts])]).astype(np.int64))
    return (torch.cat(ts) if ts else torch.zeros(0, 3, dtype=torch.float64, device=dev)), off


def chamfer_batch(a_list, b_list, device=None):
    """chamfer_packed of B scenes given as two lists of [N_s,3] clouds (numpy arrays or tensors, host or device, mixed freely)
    -> [B] on the device.  (A cloud list that stays the same over a loop, a target's, is better packed once with `pack` and given
    to chamfer_packed.)"""
    if len(a_list) != len(b_list) or len(a_list) < 1:
        raise ValueError("two lists of B >= 1 clouds, got %d and %d" % (len(a_list), len(b_list)))
    a, a_off = pack(a_list, device)
    b, b_off = pack(b_list, device)
    return chamfer_packed(a, a_off, b, b_off)
