"""Closed triangle meshes to the samples of voxel grids on the device: the exact signed distance of every sample to its mesh,
by the all-pairs kernel of csrc/mesh_grid.hip (ABI: csrc/mesh_grid.h).  What SDFGrid3D.from_mesh is built on.

    grids = mesh_grid_sdf([verts_a, verts_b], [faces_a, faces_b], dims=[(33, 33, 33), (17, 17, 17)], scale=[1.0, 0.6])
    dims, data = mesh_grid_sdf_pooled(...)              # the same, pooled: grids.GridTable.from_pooled(dims, data)
    verts, faces = check_mesh(verts, faces)             # the host-side validation alone (numpy)

Sample (i, j, k) of a grid sits at scale * (-1 + 2 i / (n0 - 1), ...) in the mesh's frame, the inverse of the grid query's
index rule, and holds sign * distance / scale (the query multiplies by scale): the distance is that to the nearest triangle, the
sign is negative where the generalised winding number exceeds 1/2.  No atomics: two calls return the same bits.  The cost is
samples x faces; there is no acceleration structure.
"""
import numpy as np
import torch

from . import _lib

TILE = 256           # DSS_MESH_GRID_TILE: triangles per LDS tile (= threads per workgroup)
MALFORMED = 1        # DSS_MESH_GRID_MALFORMED


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def centroid(verts, faces):
    """The volume centroid sum (a . (b x c)) (a + b + c) / 24 / vol of a closed mesh (numpy [3])."""
    m = verts.mean(0)
    v = verts - m
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    t = np.einsum("ij,ij->i", a, np.cross(b, c))
    return m + (t[:, None] * (a + b + c)).sum(0) / 24.0 / (t.sum() / 6.0)


def check_mesh(verts, faces, name="mesh"):
    """Host-side validation of one mesh -> (verts [nv,3] float64, faces [nf,3] int64) as numpy arrays, the faces turned
    outward.  ValueError where verts is not [nv,3] or not finite; faces is not [nf,3] of integers, names a vertex outside
    [0, nv) or one vertex twice in a face; the mesh is not watertight (a directed edge (i, j) without its opposite (j, i)) or not
    consistently oriented (a directed edge that occurs twice); the signed volume is zero.  A negative volume (inward normals)
    flips every face instead of raising."""
    f = _host(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError("%s: faces [nf,3] of integers, nf >= 1, got %s %s" % (name, f.shape, f.dtype))
    v = np.ascontiguousarray(_host(verts), dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or not np.isfinite(v).all():
        raise ValueError("%s: verts [nv,3] of finite numbers, got %s" % (name, v.shape))
    f, nv = f.astype(np.int64), v.shape[0]
    if f.min() < 0 or f.max() >= nv:
        raise ValueError("%s: a face index out of range [0, %d): %d" % (name, nv, f.min() if f.min() < 0 else f.max()))
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any():
        raise ValueError("%s: a face names one vertex twice" % name)
    i, j = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    fwd, cnt = np.unique(i * nv + j, return_counts=True)
    if (cnt > 1).any():
        e = fwd[cnt > 1][0]
        raise ValueError("%s: not consistently oriented: the directed edge (%d, %d) occurs %d times" % (name, e // nv, e % nv, cnt[cnt > 1][0]))
    back = np.sort(j * nv + i)
    if not np.array_equal(fwd, back):
        e = np.setdiff1d(fwd, back)[0]
        raise ValueError("%s: not watertight: the directed edge (%d, %d) has no opposite (%d, %d)" % (name, e // nv, e % nv, e % nv, e // nv))
    c = v - v.mean(0)
    t = np.einsum("ij,ij->i", c[f[:, 0]], np.cross(c[f[:, 1]], c[f[:, 2]]))
    if abs(t.sum()) <= 1e-12 * np.abs(t).sum():
        raise ValueError("%s: zero volume (signed volume %.3e)" % (name, t.sum() / 6.0))
    if t.sum() < 0:
        f = np.ascontiguousarray(f[:, [0, 2, 1]])
    return v, f


def _per_mesh(x, n, width, dtype, name):
    a = np.asarray(x, dtype=dtype)
    a = np.broadcast_to(a, (n, width) if width else (n,)) if a.ndim <= (1 if width else 0) else a
    if a.shape != ((n, width) if width else (n,)):
        raise ValueError("%s: one for all meshes or one per mesh (%d), got shape %s" % (name, n, np.shape(x)))
    return np.array(a, copy=True, order="C")      # (a broadcast view is read-only and has zero strides)


def mesh_grid_sdf_pooled(verts_list, faces_list, dims, scale, check=True, device=None):
    """Voxelise nmesh meshes in one call -> (dims [nmesh,3] int32 on the host, data [sum n0 n1 n2] float64 on the device), the
    grids one after the other, x slowest: grids.GridTable.from_pooled(dims, data) is their table.
    verts_list / faces_list: per mesh [nv,3] floats and [nf,3] integers, numpy arrays or tensors of any device; dims: (n0, n1,
    n2) for all meshes or one triple per mesh, every entry >= 2; scale: the grids' half sides, one or one per mesh, > 0.
    check=True: check_mesh on every mesh first (host; closed, consistently oriented, non-zero volume, faces turned outward).
    check=False takes the arrays as they are: an open or inward mesh gives the distance with whatever sign the winding number
    implies, and a face index out of range raises HipLibraryError (the kernel's status word) after the call, naming the mesh."""
    if len(verts_list) != len(faces_list) or len(verts_list) < 1:
        raise ValueError("two lists of nmesh >= 1 meshes, got %d and %d" % (len(verts_list), len(faces_list)))
    nmesh = len(verts_list)
    if check:
        verts_list, faces_list = zip(*[check_mesh(v, f, "mesh %d" % m) for m, (v, f) in enumerate(zip(verts_list, faces_list))])
    dims = _per_mesh(dims, nmesh, 3, np.int64, "dims")
    sc = _per_mesh(scale, nmesh, 0, np.float64, "scale")
    if dims.min() < 2 or not (sc > 0).all() or not np.isfinite(sc).all():
        raise ValueError("dims >= 2 per axis and scale > 0, got %s and %s" % (dims.tolist(), sc.tolist()))
    sizes = dims.prod(1)
    if sizes.sum() > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 samples in one call")
    dev = torch.device(device) if device is not None else \
        next((x.device for x in list(verts_list) + list(faces_list) if torch.is_tensor(x) and x.is_cuda), torch.device("cuda"))
    if dev.type != "cuda":
        raise _lib.HipLibraryError("mesh_grid_sdf needs a HIP device (got %s); there is no CPU fallback" % dev)
    vs = [torch.as_tensor(v).detach().to(dev, torch.float64).reshape(-1, 3) for v in verts_list]
    fs = [torch.as_tensor(f).detach().to(dev, torch.int32).reshape(-1, 3) for f in faces_list]
    nv, nf = [v.shape[0] for v in vs], [f.shape[0] for f in fs]
    if min(nv) < 1 or min(nf) < 1 or sum(nv) > 2 ** 31 - 1 or sum(nf) > 2 ** 31 - 1:
        raise ValueError("every mesh needs a vertex and a face (and all of them fewer than 2^31 in all)")
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(dev)
    verts, faces = torch.cat(vs).contiguous(), torch.cat(fs).contiguous()
    vert_off, face_off = i32(np.concatenate([[0], np.cumsum(nv)])), i32(np.concatenate([[0], np.cumsum(nf)]))
    grid_dims, grid_off = i32(dims), i32(np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    scale_d = torch.as_tensor(sc).to(dev)
    data = torch.empty(int(sizes.sum()), dtype=torch.float64, device=dev)
    status = torch.zeros(nmesh, dtype=torch.int32, device=dev)
    fn = getattr(_lib.lib(), "dss_mesh_grid_sdf", None)
    if fn is None:
        raise _lib.HipLibraryError("the library does not export dss_mesh_grid_sdf: rebuild it (python __graft_entry__.py build)")
    _lib.check(fn(nmesh, _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(vert_off), _lib.ptr(face_off), _lib.ptr(grid_dims), _lib.ptr(grid_off),
                  _lib.ptr(scale_d), int(sizes.max()), max(nf), _lib.ptr(data), _lib.ptr(status), _lib.stream_ptr(dev)), "dss_mesh_grid_sdf")
    bad = np.flatnonzero(status.cpu().numpy())
    if len(bad):
        raise _lib.HipLibraryError("dss_mesh_grid_sdf: mesh %d has a face index outside [0, %d) (status %d); its grid is not that of "
                                   "the mesh" % (bad[0], nv[bad[0]], int(status[bad[0]])))
    return torch.as_tensor(dims.astype(np.int32)), data


def mesh_grid_sdf(verts_list, faces_list, dims, scale, check=True, device=None):
    """mesh_grid_sdf_pooled as a list: per mesh its [n0,n1,n2] float64 grid on the device (views of one pooled buffer)."""
    dims, data = mesh_grid_sdf_pooled(verts_list, faces_list, dims, scale, check, device)
    out, at = [], 0
    for n0, n1, n2 in dims.tolist():
        out.append(data[at:at + n0 * n1 * n2].reshape(n0, n1, n2)); at += n0 * n1 * n2
    return out
