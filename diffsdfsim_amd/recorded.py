"""Recorded RGB-D sequences on the device: the observations of experiments/trajectory_fitting/optim_pointcloud_real.py in the
form that script reads them, the selection of the thrown body's points from them and the statistics it initialises from, by
the kernels of csrc/cloud_select.hip (ABI: include/cloud_select.h).

    rec = load_recording(path)                         # dict(pcs [T,H,W,3], segs [T,H,W], planes [P,4], grav_dir [3], g, ...)
    pts, seg_off = select_points(rec["pcs"], rec["segs"], label=4)
    st = segment_stats(pts, seg_off)                   # count [T], mean / min / max [T,3]

`pcs` is the organised cloud (the world-frame point each pixel sees), `segs` the label image; the thrown body carries label 4
(:153).  A pixel is selected if it has the label and three finite coordinates: the reference keeps a point with a NaN or an
infinite coordinate, which its loss then ignores (it fails |p| < scale) but which turns the initial statistics (:326-331) into
NaN.  Points come in row-major pixel order per frame: `pcs[t][segs[t] == label]`.  Device tensors only; not differentiable:
observations are data.
"""
import pickle

import numpy as np
import torch

from . import _lib

LABEL = 4      # the thrown body's label in the recorded segmentations (optim_pointcloud_real.py:153)
STATS = 10     # count, sum [3], min [3], max [3]


def load_recording(path, device=None):
    """The reference's `real_world_data.pkl` (a dict of lists of per-frame arrays pcs, segs, planes, grav_dirs and optionally
    rgbs, stacked as optim_pointcloud_real.py:317-319 stacks them) or an .npz with the same keys.
    -> dict(pcs [T,H,W,3] float64, segs [T,H,W] int32, planes [P,4] float64 (rows n, d; the mean over the frames, :324),
    grav_dir [3] (the mean over the frames), g (its norm, :322), rgbs [T,H,W,3] uint8 or None), tensors on `device` (default: the
    current HIP device)."""
    dev = torch.device("cuda" if device is None else device)
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            raw = {k: z[k] for k in z.files}
    else:
        with open(path, "rb") as f:
            raw = pickle.load(f)
    obs = {}
    for k, v in raw.items():
        if isinstance(v, (list, tuple)):
            if len(v) == 0:
                continue
            v = np.stack([np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in v])
        obs[k] = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    missing = [k for k in ("pcs", "segs", "planes", "grav_dirs") if k not in obs]
    if missing:
        raise ValueError("%s: a recording holds pcs, segs, planes and grav_dirs; missing %s" % (path, missing))
    pcs, segs = obs["pcs"], obs["segs"]
    if pcs.ndim != 4 or pcs.shape[3] != 3 or segs.shape != pcs.shape[:3]:
        raise ValueError("%s: pcs [T,H,W,3] and segs [T,H,W], got %s and %s" % (path, pcs.shape, segs.shape))
    planes = np.asarray(obs["planes"], np.float64)
    planes = planes.reshape(planes.shape[0], -1, 4).mean(axis=0) if planes.ndim == 3 else planes.reshape(-1, 4)
    grav = np.asarray(obs["grav_dirs"], np.float64).reshape(-1, 3).mean(axis=0)
    T = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    return dict(pcs=T(pcs, np.float64), segs=T(segs, np.int32), planes=T(planes, np.float64), grav_dir=T(grav, np.float64),
                g=float(np.linalg.norm(grav)), rgbs=T(obs["rgbs"], np.uint8) if "rgbs" in obs else None)


def select_points(pcs, segs, label=LABEL):
    """The points of `label` in pcs [T,H,W,3] float64 / segs [T,H,W] int32: pixels of that label with three finite coordinates,
    row-major pixel order per frame.  -> (pts [N,3] float64 on the device, seg_off [T+1] int64 numpy: frame t owns
    pts[seg_off[t]:seg_off[t+1]])."""
    if not (torch.is_tensor(pcs) and torch.is_tensor(segs)):
        raise TypeError("pcs and segs: torch tensors on a HIP device")
    if not (pcs.is_cuda and segs.is_cuda):
        raise _lib.HipLibraryError("select_points needs tensors on a HIP device (got %s, %s); there is no CPU fallback" % (pcs.device, segs.device))
    if pcs.dim() != 4 or pcs.shape[3] != 3 or tuple(segs.shape) != tuple(pcs.shape[:3]) or pcs.dtype != torch.float64 or segs.dtype != torch.int32:
        raise ValueError("pcs [T,H,W,3] float64 and segs [T,H,W] int32, got %s %s and %s %s" %
                         (tuple(pcs.shape), pcs.dtype, tuple(segs.shape), segs.dtype))
    T, H, W = segs.shape
    if T < 1 or H < 1 or W < 1 or T * H * W > 2 ** 31 - 1:
        raise ValueError("at least one pixel and T * H * W < 2^31, got %s" % (tuple(segs.shape),))
    dev = pcs.device
    pcs, segs = pcs.detach().contiguous(), segs.contiguous()
    count, emit = _lib.lib().dss_cloud_select_count, _lib.lib().dss_cloud_select_emit
    rows = torch.zeros(T * H, dtype=torch.int32, device=dev)
    _lib.check(count(T, H, W, int(label), _lib.ptr(pcs), _lib.ptr(segs), _lib.ptr(rows), _lib.stream_ptr(dev)), "dss_cloud_select_count")
    incl = torch.cumsum(rows, 0, dtype=torch.int64)
    row_off = (incl - rows).to(torch.int32)
    seg_off = np.concatenate([[0], incl[H - 1::H].cpu().numpy()]).astype(np.int64)      # (the one read-back: N = seg_off[-1])
    pts = torch.zeros(int(seg_off[-1]), 3, dtype=torch.float64, device=dev)
    _lib.check(emit(T, H, W, int(label), _lib.ptr(pcs), _lib.ptr(segs), _lib.ptr(row_off), _lib.ptr(pts), _lib.stream_ptr(dev)),
               "dss_cloud_select_emit")
    return pts, seg_off


def _stats(pts, seg_off):
    """out [nseg,10] of dss_cloud_stats on the device: count, sum xyz, min xyz, max xyz."""
    if not torch.is_tensor(pts):
        raise TypeError("pts: a torch tensor on a HIP device")
    if not pts.is_cuda:
        raise _lib.HipLibraryError("segment_stats needs tensors on a HIP device (got %s); there is no CPU fallback" % pts.device)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float64:
        raise ValueError("pts [N,3] float64, got %s %s" % (tuple(pts.shape), pts.dtype))
    off = torch.as_tensor(seg_off).detach().to("cpu", torch.int64).reshape(-1)
    nseg = off.numel() - 1
    if nseg < 1 or bool((off[1:] < off[:-1]).any()) or int(off[0]) < 0 or int(off[-1]) > pts.shape[0] or int(off[-1]) > 2 ** 31 - 1:
        raise ValueError("seg_off: nseg + 1 >= 2 ascending offsets into pts (below 2^31)")
    dev = pts.device
    max_len = int((off[1:] - off[:-1]).max())
    fn, nbytes = _lib.lib().dss_cloud_stats, _lib.lib().dss_cloud_stats_workspace_bytes(nseg, max_len)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    out = torch.zeros(nseg, STATS, dtype=torch.float64, device=dev)
    off_d, pts = off.to(dev, torch.int32), pts.detach().contiguous()
    _lib.check(fn(nseg, max_len, _lib.ptr(off_d), _lib.ptr(pts), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev)), "dss_cloud_stats")
    return out


def segment_stats(pts, seg_off):
    """Per segment of pts [N,3] (segment s owns pts[seg_off[s]:seg_off[s+1]]): dict(count [nseg], sum, mean, min, max [nseg,3]),
    float64 on the device.  mean = sum / count there (NaN for an empty segment, whose min is +inf and max -inf)."""
    out = _stats(pts, seg_off)
    return dict(count=out[:, 0], sum=out[:, 1:4], mean=out[:, 1:4] / out[:, :1], min=out[:, 4:7], max=out[:, 7:10])
