"""Depth camera on the device: what the experiment's Recorder3D(record_points=True, record_seg=True) records and what
match_pointcloud (experiments/trajectory_fitting/optim_pointcloud.py:168-187) selects from it, by the kernels of
csrc/depth_camera.hip (ABI: include/depth_camera.h).

    depth, seg = render_depth(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, size=(640, 480))
    pts, seg_off = observed_points(depth, seg, body, cam_pose, fx, fy, cx, cy)
    pts, seg_off = observe(pose, shape_type, prm, body, cam_pose, fx, fy, cx, cy, noise=...)      # both, in chunks of views

A view is one scene at one frame: `pose` [nview,nbody,7] (quaternion wxyz + position), `shape_type` [nview,nbody] int32, `prm`
[nview,nbody,4] (three shape parameters + the corner radius), nbody <= 8.  `cam_pose` is the 4 x 4 camera-to-world matrix, OpenGL
convention; pixel (row, col) looks along the camera-frame direction ((col + 0.5 - cx) / fx, -(row + 0.5 - cy) / fy, -1).
depth [nview,H,W] float64 is the distance along the optical axis (0: nothing hit within [znear, zfar]), seg [nview,H,W] int32 the
body hit (-1 none, -2 the trace ran out of iterations).  Boxes, spheres, cylinders and rounded boxes only: any other shape
raises.  Device tensors only.  Not differentiable: observations are data.

    depth, seg = render_depth_diff(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, size, znear, zfar, grids=None, grid_id=None)

is the same render (the same bits) whose `depth` carries a graph to `pose`, `prm[..., :3]` and, through a GridTable made of grids
that require grad, to their samples, by the adjoint kernel of csrc/depth_adjoint.hip (ABI: csrc/depth_adjoint.h), and
from the samples of a neural body's value grid (igr.igr_lattice_values, body_grid(body, diff=True)) on to its latent code.  It is the
derivative of the visible surface at fixed visibility: the motion of silhouettes is not modelled.

Voxel-grid bodies: `grids=` a grids.GridTable (or a list of [n0,n1,n2] arrays) and `grid_id` [nview,nbody] (-1: none) let bodies of
shape type 7 (SDFGrid3D) and 6 (a neural SDF3D, seen through the value grid its mesh is extracted from: body_grid) into the
same images, by dss_depth_render_grids; brick, bowl and a grid or neural body without a grid still raise.

The colour camera (csrc/shade_camera.hip, ABI: include/shade_camera.h) shades those images: surface normals, Lambert shading by up to
four directional lights with hard shadows, the bodies' colours; physics3d.utils.Recorder3D records through it.

    rgb, normal, shade, flags = shade(depth, seg, pose, shape_type, prm, cam_pose, fx, fy, cx, cy, colors, lights)
    rgb, depth, seg = render_color(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, colors, lights)      # both, in chunks of views
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .grids import as_table, table_and_ids

MAX_BODIES = 8


def _camera(cam_pose, dev):
    cam = torch.as_tensor(np.asarray(cam_pose.detach().cpu() if torch.is_tensor(cam_pose) else cam_pose, np.float64))
    if tuple(cam.shape) != (4, 4):
        raise ValueError("cam_pose: the 4 x 4 camera-to-world matrix, got %s" % (tuple(cam.shape),))
    return cam.to(dev).contiguous()


def _intrinsics(fx, fy, cx, cy):
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    if not (fx != 0.0 and fy != 0.0 and all(np.isfinite([fx, fy, cx, cy]))):
        raise ValueError("fx and fy non-zero, cx and cy finite, got %r" % ((fx, fy, cx, cy),))
    return fx, fy, cx, cy


def _scene(pose, shape_type, prm, nview=None):
    """The validated scene -> (pose, prm, types: detached, contiguous, on the device of `pose`; nview, nbody).  nview: the views that
    images passed beside the scene have."""
    if pose.dim() != 3 or pose.shape[2] != 7 or pose.dtype != torch.float64 or prm.dtype != torch.float64 or \
            tuple(prm.shape) != (pose.shape[0], pose.shape[1], 4) or (nview is not None and pose.shape[0] != nview):
        raise ValueError("pose [nview,nbody,7] and prm [nview,nbody,4] as float64%s, got %s and %s" %
                         ("" if nview is None else " for the %d views of depth" % nview, tuple(pose.shape), tuple(prm.shape)))
    nview, nbody = pose.shape[:2]
    if nview < 1 or not 1 <= nbody <= MAX_BODIES:
        raise ValueError("at least one view of 1 to %d bodies, got %d views of %d" % (MAX_BODIES, nview, nbody))
    types = torch.as_tensor(shape_type).to(pose.device, torch.int32).reshape(nview, nbody).contiguous()
    return pose.detach().contiguous(), prm.detach().contiguous(), types, nview, nbody


def _image_pair(depth, seg):
    """The validated images -> (depth, seg contiguous, nview, H, W)."""
    if depth.dim() != 3 or depth.shape != seg.shape or depth.dtype != torch.float64 or seg.dtype != torch.int32:
        raise ValueError("depth float64 and seg int32, both [nview,H,W], got %s %s and %s %s" %
                         (tuple(depth.shape), depth.dtype, tuple(seg.shape), seg.dtype))
    nview, H, W = depth.shape
    if nview < 1 or H < 1 or W < 1 or nview * H * W > 2 ** 31 - 1:
        raise ValueError("at least one pixel and nview * H * W < 2^31, got %s" % (tuple(depth.shape),))
    return depth.contiguous(), seg.contiguous(), nview, H, W


def _table(grids, grid_id, nview, nbody, dev):
    """-> (the GridTable of `grids`, its checked ids [nview,nbody] on dev), or (None, None) without grids."""
    return (None, None) if grids is None else table_and_ids(grids, grid_id, (nview, nbody), dev, "nview,nbody")


def _grid_args(table, ids, block_min=True):
    """The grid arguments of a camera entry: grid_id, ngrid, grid_off, grid_dims, grid_data and, for the entries that trace,
    blk_off and blk_min; without a table ngrid = 0 and every pointer NULL."""
    if table is None:
        arrays = (None,) * (5 if block_min else 3)
    else:
        arrays = (table.off, table.dims, table.data.detach()) + ((table.blk_off, table.block_min()) if block_min else ())
    return (_lib.ptr(ids), 0 if table is None else table.ngrid) + tuple(_lib.ptr(a) for a in arrays)


def _view_chunks(pose, shape_type, grids, grid_id, per):
    """What observe and render_color walk: types [nview,nbody] on the device, the table (made once: its block minima are shared by
    the chunks) and, per chunk of `per` views, (its slice, its grid ids or None)."""
    nview = pose.shape[0]
    types = torch.as_tensor(shape_type).to(pose.device, torch.int32).reshape(nview, -1)
    if grids is not None:
        grids = as_table(grids, pose.device)
        grid_id = torch.as_tensor(grid_id).reshape(nview, -1)
    slices = [slice(v0, v0 + per) for v0 in range(0, nview, per)]
    return types, grids, [(sl, None if grids is None else grid_id[sl]) for sl in slices]


def render_depth(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, size=(640, 480), znear=0.1, zfar=100.0, grids=None, grid_id=None):
    """-> (depth [nview,H,W] float64, seg [nview,H,W] int32) on the device of `pose`; size = (W, H).  See the module's text."""
    _lib.require_device(pose, prm)
    pose, prm, types, nview, nbody = _scene(pose, shape_type, prm)
    W, H = int(size[0]), int(size[1])
    if W < 1 or H < 1 or nview * W * H > 2 ** 31 - 1:
        raise ValueError("size = (W, H), positive, nview * W * H < 2^31 (render in chunks of views: observe), got %r for %d views" % (size, nview))
    if not 0.0 <= znear < zfar:
        raise ValueError("0 <= znear < zfar, got %r, %r" % (znear, zfar))
    fx, fy, cx, cy = _intrinsics(fx, fy, cx, cy)
    dev = pose.device
    depth = torch.zeros(nview, H, W, dtype=torch.float64, device=dev)
    seg = torch.full((nview, H, W), -1, dtype=torch.int32, device=dev)
    cam = _camera(cam_pose, dev)
    T, ids = _table(grids, grid_id, nview, nbody, dev)
    if T is not None:
        rc = _lib.lib().dss_depth_render_grids(nview, nbody, _lib.ptr(pose), _lib.ptr(types), _lib.ptr(prm), _lib.ptr(cam), fx, fy, cx, cy, W, H,
                                               float(znear), float(zfar), *_grid_args(T, ids), _lib.ptr(depth), _lib.ptr(seg),
                                               _lib.stream_ptr(dev))
        if rc == -3:
            raise _lib.HipLibraryError("dss_depth_render_grids: the renderer takes shape types 0-3 and, with a grid_id >= 0, grid and "
                                       "neural bodies (7, 6); got types %s with grid ids %s" %
                                       (sorted(set(types.reshape(-1).tolist())), sorted(set(ids.reshape(-1).tolist()))))
        _lib.check(rc, "dss_depth_render_grids")
        return depth, seg
    fn = _lib.lib().dss_depth_render
    rc = fn(nview, nbody, _lib.ptr(pose), _lib.ptr(types), _lib.ptr(prm), _lib.ptr(cam),
            fx, fy, cx, cy, W, H, float(znear), float(zfar), _lib.ptr(depth), _lib.ptr(seg), _lib.stream_ptr(dev))
    if rc == -3:
        raise _lib.HipLibraryError("dss_depth_render: the renderer takes boxes, spheres, cylinders and rounded boxes "
                                   "(shape types 0-3), got types %s" % sorted(set(types.reshape(-1).tolist())))
    _lib.check(rc, "dss_depth_render")
    return depth, seg


def observed_points(depth, seg, body, cam_pose, fx, fy, cx, cy):
    """The world-frame points of body index `body` in depth / seg [nview,H,W]: its mask eroded by one pixel, pixels of depth 0
    dropped, back-projected; row-major pixel order per view.  -> (pts [N,3] float64 on the device, seg_off [nview+1] int64 numpy:
    view v owns pts[seg_off[v]:seg_off[v+1]])."""
    _lib.require_device(depth, seg)
    depth, seg, nview, H, W = _image_pair(depth, seg)
    fx, fy, cx, cy = _intrinsics(fx, fy, cx, cy)
    dev = depth.device
    count, emit = _lib.lib().dss_depth_points_count, _lib.lib().dss_depth_points_emit
    rows = torch.zeros(nview * H, dtype=torch.int32, device=dev)
    _lib.check(count(nview, H, W, int(body), _lib.ptr(depth), _lib.ptr(seg), _lib.ptr(rows), _lib.stream_ptr(dev)), "dss_depth_points_count")
    incl = torch.cumsum(rows, 0, dtype=torch.int64)
    row_off = (incl - rows).to(torch.int32)
    seg_off = np.concatenate([[0], incl[H - 1::H].cpu().numpy()]).astype(np.int64)      # (the one read-back: N = seg_off[-1])
    pts = torch.zeros(int(seg_off[-1]), 3, dtype=torch.float64, device=dev)
    cam = _camera(cam_pose, dev)
    _lib.check(emit(nview, H, W, int(body), _lib.ptr(depth), _lib.ptr(seg), _lib.ptr(row_off), _lib.ptr(cam), fx, fy, cx, cy,
                    _lib.ptr(pts), _lib.stream_ptr(dev)), "dss_depth_points_emit")
    return pts, seg_off


def views_per_chunk(size, max_bytes=256 << 20, bytes_per_pixel=12):
    """How many views `observe` renders at a time: 12 bytes (depth and segment) per pixel within max_bytes, at least one.
    render_color counts the images shade writes as well (bytes_per_pixel)."""
    return max(1, int(max_bytes) // (int(bytes_per_pixel) * int(size[0]) * int(size[1])))


def observe(pose, shape_type, prm, body, cam_pose, fx, fy, cx, cy, size=(640, 480), znear=0.1, zfar=100.0, noise=0.0, seed=0,
            max_bytes=256 << 20, grids=None, grid_id=None):
    """render_depth and observed_points over all views, at most `max_bytes` of depth and segment images at a time (a 640 x 480
    view is 3.7 MB).  noise: the reference's depth_noise_factor, applied between the two kernels as Recorder3D.get_pointcloud
    does, depth += randn * noise * depth^2 (a pixel of depth 0 stays 0), from a generator seeded with `seed` on the device.
    grids, grid_id [nview,nbody]: as in render_depth.
    -> (pts [N,3], seg_off [nview+1]) as observed_points returns them."""
    gen = torch.Generator(device=pose.device)
    gen.manual_seed(int(seed))
    types, grids, chunks = _view_chunks(pose, shape_type, grids, grid_id, views_per_chunk(size, max_bytes))
    pts, off = [], [np.zeros(1, np.int64)]
    for sl, gid in chunks:
        depth, seg = render_depth(pose[sl], types[sl], prm[sl], cam_pose, fx, fy, cx, cy, size, znear, zfar, grids, gid)
        if noise > 0:
            depth += torch.randn(depth.shape, dtype=depth.dtype, device=depth.device, generator=gen) * noise * depth ** 2
        p, o = observed_points(depth, seg, body, cam_pose, fx, fy, cx, cy)
        pts.append(p); off.append(o[1:] + off[-1][-1])
    return torch.cat(pts), np.concatenate(off)


def _lights(lights, dev):
    """lights: rows of (direction towards the light [3], intensity) or [nlight,4] -> ([nlight,4] float64 on dev or None, nlight)."""
    rows = [] if lights is None else [np.concatenate([np.asarray(r[0], np.float64).reshape(3), [float(r[1])]]) if len(r) == 2
                                      else np.asarray(r, np.float64).reshape(4) for r in
                                      (lights.detach().cpu().numpy() if torch.is_tensor(lights) else lights)]
    if len(rows) > 4:
        raise ValueError("at most 4 lights, got %d" % len(rows))
    if any(not np.isfinite(r).all() or not np.any(r[:3] != 0.0) for r in rows):
        raise ValueError("a light is (a finite direction towards it that is not 0, its intensity)")
    return (torch.as_tensor(np.array(rows, np.float64).reshape(-1, 4)).to(dev).contiguous() if rows else None), len(rows)


def shade(depth, seg, pose, shape_type, prm, cam_pose, fx, fy, cx, cy, colors, lights, ambient=0.1, background=(1, 1, 1), shadows=True,
          shadow_bias=1e-3, zfar=100.0, grids=None, grid_id=None):
    """Shade the images render_depth returned for the same views (dss_shade_render, include/shade_camera.h): the surface normal at
    every hit, Lambert shading by the lights with hard shadows, the bodies' colours.
    colors [nview,nbody,3] (or [nbody,3] for every view) in [0, 1]; lights: up to four (direction TOWARDS the light, intensity)
    in the world frame; ambient the shade of a surface no light reaches; background the colour of a pixel that hit nothing.
    -> (rgb [nview,H,W,3] uint8, normal [nview,H,W,3] float64 (world frame, 0 where nothing is hit), shade [nview,H,W] float64 =
    min(1, ambient + sum_k I_k V_k max(0, n . l_k)), flags [nview,H,W] uint8: bit 0 a shadow ray used up its iterations, bit 1
    the field's gradient vanished and the normal faces the camera) on the device."""
    _lib.require_device(depth, seg, pose, prm)
    depth, seg, nview, H, W = _image_pair(depth, seg)
    pose, prm, types, nview, nbody = _scene(pose, shape_type, prm, nview)
    if not shadow_bias > 0.0 or not zfar > 0.0:
        raise ValueError("shadow_bias > 0 and zfar > 0, got %r, %r" % (shadow_bias, zfar))
    fx, fy, cx, cy = _intrinsics(fx, fy, cx, cy)
    dev = depth.device
    fn = _lib.lib().dss_shade_render
    col = torch.as_tensor(colors, dtype=torch.float64).to(dev)
    col = (col.expand(nview, nbody, 3) if col.dim() == 2 else col.reshape(nview, nbody, 3)).contiguous()
    lt, nlight = _lights(lights, dev)
    bg = (ctypes.c_double * 3)(*[float(b) for b in background])
    cam = _camera(cam_pose, dev)
    rgb = torch.zeros(nview, H, W, 3, dtype=torch.uint8, device=dev)
    normal = torch.zeros(nview, H, W, 3, dtype=torch.float64, device=dev)
    shd = torch.zeros(nview, H, W, dtype=torch.float64, device=dev)
    flags = torch.zeros(nview, H, W, dtype=torch.uint8, device=dev)
    gargs = _grid_args(*_table(grids, grid_id, nview, nbody, dev))
    rc = fn(nview, nbody, _lib.ptr(pose), _lib.ptr(types), _lib.ptr(prm), _lib.ptr(cam), fx, fy, cx, cy, W, H, float(zfar), *gargs,
            _lib.ptr(depth), _lib.ptr(seg), _lib.ptr(col), nlight, None if lt is None else _lib.ptr(lt), float(ambient),
            ctypes.cast(bg, ctypes.c_void_p), int(bool(shadows)), float(shadow_bias), _lib.ptr(normal), _lib.ptr(shd), _lib.ptr(rgb),
            _lib.ptr(flags), _lib.stream_ptr(dev))
    if rc == -3:
        raise _lib.HipLibraryError("dss_shade_render: the camera takes shape types 0-3 and, with a grid_id >= 0, grid and neural bodies "
                                   "(7, 6); got types %s" % sorted(set(types.reshape(-1).tolist())))
    _lib.check(rc, "dss_shade_render")
    return rgb, normal, shd, flags


# bytes per pixel of a view while render_color works on it: depth 8 + seg 4, and shade's normal 24 + shade 8 + rgb 3 + flags 1
_COLOR_BYTES = 12 + 36


def render_color(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, colors, lights, size=(640, 480), znear=0.1, zfar=100.0, ambient=0.1,
                 background=(1, 1, 1), shadows=True, shadow_bias=1e-3, grids=None, grid_id=None, max_bytes=256 << 20):
    """render_depth, then shade, over all views, at most `max_bytes` of images at a time (views_per_chunk with the 36 further
    bytes per pixel that shade writes).  -> (rgb [nview,H,W,3] uint8, depth [nview,H,W] float64, seg [nview,H,W] int32)."""
    nview = pose.shape[0]
    types, grids, chunks = _view_chunks(pose, shape_type, grids, grid_id, views_per_chunk(size, max_bytes, _COLOR_BYTES))
    col = torch.as_tensor(colors, dtype=torch.float64)
    if col.dim() == 2:
        col = col.expand(nview, *col.shape)
    out = []
    for sl, gid in chunks:
        depth, seg = render_depth(pose[sl], types[sl], prm[sl], cam_pose, fx, fy, cx, cy, size, znear, zfar, grids, gid)
        rgb = shade(depth, seg, pose[sl], types[sl], prm[sl], cam_pose, fx, fy, cx, cy, col[sl], lights, ambient, background, shadows,
                    shadow_bias, zfar, grids, gid)[0]
        out.append((rgb, depth, seg))
    return tuple(torch.cat([o[i] for o in out]) for i in range(3))


def body_grid(body, diff=False):
    """The grid through which the camera sees a level-set body -> (samples [n0,n1,n2] float64, scale).  SDFGrid3D: its own `sdf`.
    A neural SDF3D: the network's values on the res^3 lattice its mesh was extracted from (the same lattice and the same
    igr.igr_values call as meshsdf.igr_mesh), so the camera shows the surface that marching cubes meshed.
    diff=True: the same samples (the same bits) with the graph to `body.latent` (igr.igr_lattice_values), so that a
    render_depth_diff of a table made of them reaches the latent code; an SDFGrid3D's `sdf` carries its own graph either way."""
    from . import igr, meshsdf
    from .physics3d.bodies import SDF3D, SDFGrid3D
    if isinstance(body, SDFGrid3D):
        return body.sdf, float(body.scale.detach())
    if isinstance(body, SDF3D):
        dev = body.igr.packed["W0"].device
        res = int(body.res)
        if diff:
            return igr.igr_lattice_values(body.latent.to(torch.float64), body.igr.packed, res), float(body.scale.detach())
        lat = body.latent.detach().to(torch.float64).to(dev)
        return igr.igr_values(meshsdf._grid_cached(res, dev), lat, body.igr.packed).reshape(res, res, res), float(body.scale.detach())
    raise TypeError("body_grid: an SDFGrid3D or a neural SDF3D, got %s" % type(body).__name__)


class _RenderDepth(torch.autograd.Function):
    """render_depth with a backward by dss_depth_adjoint.  grid_data is grids.data where the table carries a graph, else None."""

    @staticmethod
    def forward(ctx, pose, prm, grid_data, types, cam, intr, size, znear, zfar, grids, ids, min_cos, dropped_out):
        pose_c, prm_c = pose.detach().contiguous(), prm.detach().contiguous()
        depth, seg = render_depth(pose_c, types, prm_c, cam, *intr, size, znear, zfar, grids, ids)
        ctx.save_for_backward(pose_c, prm_c, types, cam, depth, seg, *(() if grids is None else (ids,)))
        ctx.intr, ctx.size, ctx.min_cos, ctx.table, ctx.dropped_out = intr, size, float(min_cos), grids, dropped_out
        ctx.mark_non_differentiable(seg)
        return depth, seg

    @staticmethod
    def backward(ctx, g_depth, _g_seg):
        pose, prm, types, cam, depth, seg, *ids = ctx.saved_tensors
        fn = getattr(_lib.lib(), "dss_depth_adjoint", None)
        if fn is None:
            raise _lib.HipLibraryError("the library does not export dss_depth_adjoint: rebuild it (python __graft_entry__.py build)")
        nview, nbody = pose.shape[:2]
        (W, H), dev = ctx.size, pose.device
        g_depth = g_depth.detach().to(torch.float64).contiguous()
        g_pose = torch.zeros(nview, nbody, 7, dtype=torch.float64, device=dev)
        g_prm = torch.zeros(nview, nbody, 4, dtype=torch.float64, device=dev)      # (the corner radius is a constant: column 3 stays 0)
        g3 = torch.zeros(nview, nbody, 3, dtype=torch.float64, device=dev)
        dropped = torch.zeros(nview, nbody, dtype=torch.int32, device=dev)
        nbytes = _lib.lib().dss_depth_adjoint_workspace_bytes(nview, nbody, W, H)
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        g_grid = torch.zeros_like(ctx.table.data) if ids and ctx.needs_input_grad[2] else None
        gargs = _grid_args(ctx.table, *ids or (None,), block_min=False)
        rc = fn(nview, nbody, _lib.ptr(pose), _lib.ptr(types), _lib.ptr(prm), _lib.ptr(cam), *ctx.intr, W, H, _lib.ptr(depth), _lib.ptr(seg),
                _lib.ptr(g_depth), ctx.min_cos, *gargs, _lib.ptr(g_pose), _lib.ptr(g3), _lib.ptr(g_grid),
                _lib.ptr(dropped), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(rc, "dss_depth_adjoint")
        g_prm[..., :3] = g3
        if ctx.dropped_out is not None:
            ctx.dropped_out.copy_(dropped)
        return g_pose, g_prm, g_grid, None, None, None, None, None, None, None, None, None, None


def render_depth_diff(pose, shape_type, prm, cam_pose, fx, fy, cx, cy, size=(640, 480), znear=0.1, zfar=100.0, grids=None, grid_id=None,
                      min_cos=1e-3, return_dropped=False):
    """render_depth whose depth is differentiable -> (depth [nview,H,W], seg [nview,H,W]) with the bits of render_depth.
    `depth` carries a graph to `pose` [nview,nbody,7] (raw quaternion and position), to `prm[..., :3]` (the corner radius prm[..., 3],
    which is also a grid body's scale, is a constant) and, where `grids` is a grids.GridTable made of tensors that require grad, to
    those grids' samples (fp64 atomic adds: their gradient is reproducible to rounding, the others bit for bit).
    d depth / d theta = -(d F / d theta) / (n . d) at every hit pixel (csrc/depth_adjoint.h): the derivative of the visible surface
    at fixed visibility.  The motion of a silhouette -- a pixel that changes the body it shows -- is NOT modelled, and neither are
    the camera pose or a body's scale.  A neural body's latent code is reached through its value grid: make the table of
    igr.igr_lattice_values(latent, packed, res) (or body_grid(body, diff=True)), whose backward pass carries the samples' gradient
    on to the code (csrc/igr_grid_adjoint.h).  Pixels that hit nothing, and
    hit pixels whose cosine of incidence is below `min_cos`, contribute nothing; the latter are counted per (view, body).
    return_dropped: also return an int32 [nview,nbody] tensor that every backward pass through this render fills with those counts."""
    _lib.require_device(pose, prm)
    if not 0.0 <= float(min_cos) <= 1.0:
        raise ValueError("min_cos in [0, 1], got %r" % (min_cos,))
    dev = pose.device
    _, _, types, nview, nbody = _scene(pose, shape_type, prm)
    W, H = int(size[0]), int(size[1])
    table, ids = _table(grids, grid_id, nview, nbody, dev)
    data = table.data if table is not None and table.data.requires_grad else None
    dropped = torch.zeros(nview, nbody, dtype=torch.int32, device=dev) if return_dropped else None
    depth, seg = _RenderDepth.apply(pose, prm, data, types, _camera(cam_pose, dev), _intrinsics(fx, fy, cx, cy), (W, H), float(znear), float(zfar),
                                    table, ids, float(min_cos), dropped)
    return (depth, seg, dropped) if return_dropped else (depth, seg)
