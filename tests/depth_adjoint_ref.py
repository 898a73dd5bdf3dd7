"""float64 numpy restatement of the depth camera's adjoint (csrc/depth_adjoint.hip, ABI csrc/depth_adjoint.h), written
differently from the kernel: no dual numbers and no unit frame -- the gradient of each primitive's distance in closed form in
world units, the trilinear weights of a grid differentiated by hand, d R / d q as four explicit matrices.

adjoint(...) -> dict(g_pose [nview,nbody,7], g_prm [nview,nbody,3], g_grids (one array per grid), dropped [nview,nbody]) and, under
the same names with the prefix `mag_`, the sum over the pixels of the absolute contribution |g_depth d t / d theta| to every output,
the scale of the tests' bound 1e-12 x mag_.  Two kinds of contribution vanish analytically while the kernel (and any float64
restatement) returns the rounding of the summands that cancel, which no multiple of the vanishing result bounds; for them, and for
them alone, the pixel adds the absolute summands that are actually rounded -- the exception tools/gen_pointcloud_golden.py makes:
  a sphere's four quaternion outputs (its field does not depend on the rotation): sum_ab |d_a| |dR_ab/dq_k| |g_b|;
  a parameter that enters this pixel's phi only through the body's scale (d phi / d prm_i = 0 on this face of the body and
  d scale / d prm_i != 0): the two paths through the scale, 2 |p|_1 / scale x |d scale / d prm_i|.

Pixel rule (depth_adjoint.h): seg < 0 or >= nbody adds nothing; a body's pixel whose hit point is outside its query cube, whose
n . d is 0 or whose cosine |n . d| / (|n| |d|) is below min_cos is counted in `dropped`.
The derivative is that of the visible surface at fixed visibility; silhouettes are not modelled."""
import numpy as np

import depth_camera_ref as ref

BOX, SPHERE, CYLINDER, ROUNDED, IGR, GRID = 0, 1, 2, 3, 6, 7


def dR_dq(q):
    """The four matrices d R / d q_k of R = quat_to_mat(q) = 1 + s N(q), s = 2 / q.q, with respect to the raw components."""
    r, i, j, k = q
    s = 2.0 / np.dot(q, q)
    N = np.array([[-(j * j + k * k), i * j - k * r, i * k + j * r], [i * j + k * r, -(i * i + k * k), j * k - i * r],
                  [i * k - j * r, j * k + i * r, -(i * i + j * j)]])
    dN = [np.array([[0, -k, j], [k, 0, -i], [-j, i, 0.0]]),
          np.array([[0, j, k], [j, -2 * i, -r], [k, r, -2 * i]]),
          np.array([[-2 * j, i, r], [i, 0, k], [-r, k, -2 * j]]),
          np.array([[-2 * k, -r, i], [r, -2 * k, j], [i, j, 0.0]])]
    return [s * dN[a] - s * s * q[a] * N for a in range(4)]


def scale_of(kind, prm):
    """-> (the query cube's half edge, its derivative w.r.t. the three parameters)."""
    d = np.zeros(3)
    if kind == SPHERE:
        d[0] = 1.5
        return 1.5 * prm[0], d
    if kind == CYLINDER:
        if prm[0] >= prm[1] / 2:
            d[0] = 1.5
        else:
            d[1] = 0.75
        return 1.5 * max(prm[0], prm[1] / 2), d
    if kind in (GRID, IGR):
        return float(prm[3]), d
    d[int(np.argmax(prm[:3]))] = 0.75
    return 0.75 * prm[:3].max(), d


def _box_like(q):
    """A box in the coordinates a = |.| - half extents, q [n,m]: -> d phi / d a [n,m] (the unit vector of max(q, 0) outside, the
    first largest axis inside)."""
    out = (q > 0).any(1)
    m = np.maximum(q, 0.0)
    nrm = np.linalg.norm(m, axis=1)
    da = np.zeros_like(q)
    da[out] = m[out] / nrm[out, None]
    da[~out, q[~out].argmax(1)] = 1.0
    return da


def primitive(kind, prm, p):
    """Closed forms at body-frame points p [n,3]: -> (g = d phi / d p [n,3], d phi / d prm [n,3])."""
    gp = np.zeros_like(p)
    if kind == SPHERE:
        gp[:, 0] = -1.0
        return p / np.linalg.norm(p, axis=1, keepdims=True), gp
    if kind == CYLINDER:
        rho = np.hypot(p[:, 0], p[:, 1])
        da = _box_like(np.stack([rho - prm[0], np.abs(p[:, 2]) - prm[1] / 2], 1))
        g = np.stack([da[:, 0] * p[:, 0] / rho, da[:, 0] * p[:, 1] / rho, da[:, 1] * np.sign(p[:, 2])], 1)
        gp[:, 0], gp[:, 1] = -da[:, 0], -0.5 * da[:, 1]
        return g, gp
    r = prm[3] if kind == ROUNDED else 0.0
    da = _box_like(np.abs(p) - (prm[:3] / 2 - r))
    return da * np.sign(p), -0.5 * da


def grid_terms(grid, scale, p):
    """-> (g = the gradient of scale * trilinear(samples) within the point's cell [n,3], corner indices [n,8,3], scale x
    weights [n,8])."""
    n = np.array(grid.shape)
    u = (p / scale + 1.0) * 0.5 * (n - 1)
    c = np.clip(np.floor(u), 0, n - 2).astype(np.int64)
    w = u - c
    g = np.zeros_like(p)
    idx, wt = [], []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                f = [w[:, 0] if dx else 1 - w[:, 0], w[:, 1] if dy else 1 - w[:, 1], w[:, 2] if dz else 1 - w[:, 2]]
                sg = [1.0 if dx else -1.0, 1.0 if dy else -1.0, 1.0 if dz else -1.0]
                v = grid[c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz]
                g[:, 0] += v * sg[0] * f[1] * f[2]
                g[:, 1] += v * f[0] * sg[1] * f[2]
                g[:, 2] += v * f[0] * f[1] * sg[2]
                idx.append(c + [dx, dy, dz]); wt.append(scale * f[0] * f[1] * f[2])
    return g * (0.5 * (n - 1)), np.stack(idx, 1), np.stack(wt, 1)


def adjoint(pose, kind, prm, cam, fx, fy, cx, cy, W, H, depth, seg, g_depth, min_cos=1e-3, grids=None, grid_id=None):
    pose, prm = np.asarray(pose, np.float64), np.asarray(prm, np.float64)
    nview, nbody = np.asarray(kind).shape
    out = dict(g_pose=np.zeros((nview, nbody, 7)), g_prm=np.zeros((nview, nbody, 3)), dropped=np.zeros((nview, nbody), np.int32),
               g_grids=[np.zeros_like(np.asarray(g, np.float64)) for g in (grids or [])])
    out.update(mag_pose=np.zeros((nview, nbody, 7)), mag_prm=np.zeros((nview, nbody, 3)), mag_grids=[np.zeros_like(g) for g in out["g_grids"]],
               count=np.zeros((nview, nbody), np.int64), cos=np.zeros(np.asarray(depth).shape))
    o, d, L = ref.rays(cam, fx, fy, cx, cy, W, H)
    for v in range(nview):
        for b in range(nbody):
            m = seg[v] == b
            if not m.any():
                continue
            k_, pr, q, pos = int(kind[v, b]), prm[v, b], pose[v, b, :4], pose[v, b, 4:]
            R = ref.quat_to_mat(q)
            t, gd, dw, Lm = depth[v][m], g_depth[v][m], d[m], L[m]
            e = o + t[:, None] * dw - pos
            p = e @ R
            sc, dsc = scale_of(k_, pr)
            gid = -1 if grid_id is None else int(grid_id[v, b])
            if k_ in (GRID, IGR):
                g, idx, wt = grid_terms(np.asarray(grids[gid], np.float64), sc, p)
                gp = np.zeros_like(p)
            else:
                g, gp = primitive(k_, pr, p)
            nd = (g * (dw @ R)).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                cos = np.abs(nd) / (np.linalg.norm(g, axis=1) * Lm)
                keep = (np.abs(p) <= sc).all(1) & (cos >= min_cos) & (nd != 0)
                k = np.where(keep, -gd / nd, 0.0)
            out["cos"][v][m] = np.where(np.isfinite(cos), cos, 0.0)
            out["dropped"][v, b] = int((~keep).sum())
            out["count"][v, b] = int(keep.sum())
            g, gp, e, p, ak = g[keep], gp[keep], e[keep], p[keep], np.abs(k[keep])
            k = k[keep]
            out["g_pose"][v, b, 4:] = -(k[:, None] * (g @ R.T)).sum(0)
            out["mag_pose"][v, b, 4:] = np.abs(k[:, None] * (g @ R.T)).sum(0)
            for a, dR in enumerate(dR_dq(q)):
                out["g_pose"][v, b, a] = (k * ((e @ dR) * g).sum(1)).sum()
                out["mag_pose"][v, b, a] = (ak * ((np.abs(e) @ np.abs(dR)) * np.abs(g)).sum(1)).sum() if k_ == SPHERE else \
                    np.abs(k * ((e @ dR) * g).sum(1)).sum()
            out["g_prm"][v, b] = (k[:, None] * gp).sum(0)
            out["mag_prm"][v, b] = (ak[:, None] * np.where(gp != 0, np.abs(gp), 2.0 * np.abs(p).sum(1, keepdims=True) / sc * np.abs(dsc))).sum(0)
            if k_ in (GRID, IGR):
                idx, wt = idx[keep], wt[keep]
                flat = np.ravel_multi_index((idx[..., 0], idx[..., 1], idx[..., 2]), out["g_grids"][gid].shape).reshape(-1)
                np.add.at(out["g_grids"][gid].reshape(-1), flat, (k[:, None] * wt).reshape(-1))
                np.add.at(out["mag_grids"][gid].reshape(-1), flat, (ak[:, None] * wt).reshape(-1))
    return out


# ---- the scenes shared by tests/test_emu_depth_adjoint.py and tests/test_depth_adjoint_gpu.py -----------------------------------
def camera(dist=20.0):
    """depth_camera_ref.experiment_camera at another distance from the origin (same direction of view)."""
    g = np.pi / 4
    Ry = np.array([[np.cos(g), 0, np.sin(g), 0], [0, 1, 0, 0], [-np.sin(g), 0, np.cos(g), 0], [0, 0, 0, 1.0]])
    Rx = np.array([[1, 0, 0, 0], [0, np.cos(-g), -np.sin(-g), 0], [0, np.sin(-g), np.cos(-g), 0], [0, 0, 0, 1.0]])
    T = np.eye(4); T[2, 3] = float(dist)
    return Ry @ Rx @ T


def intrinsics(W, H):
    """The experiment's field of view across W columns, the principal point at the image's centre."""
    return dict(fx=64.375 * W / 80.0, fy=64.375 * W / 80.0, cx=W / 2.0, cy=H / 2.0, W=W, H=H)


def disc_grid(n=9, rad=0.62, half=0.27):
    """The distance to a flat cylinder (a disc) around the unit cube's z axis on n^3 samples."""
    x, y, z = np.meshgrid(*[np.linspace(-1.0, 1.0, n)] * 3, indexing="ij")
    q = np.stack([np.hypot(x, y) - rad, np.abs(z) - half], -1)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


DISC_SCALE = 1.3
# the bodies whose derivatives are checked against finite differences, seen from camera(8.0) above the floor: no face of theirs is
# at a grazing angle (the tests assert the share of pixels with cosine >= 0.2).  The box's quaternion is not of unit length.
FD_BODIES = {
    "sphere": (SPHERE, [1.3, 0, 0, 0], _unit([0.9, 0.2, -0.3, 0.1]), [0.2, 1.4, -0.1]),
    "box": (BOX, [2.0, 1.6, 1.2, 0], 1.3 * _unit([0.95, 0.2, 0.15, 0.2]), [0.1, 1.3, 0.2]),
    "cylinder": (CYLINDER, [0.9, 1.8, 0, 0], _unit([0.8, 0.45, 0.2, 0.1]), [0.0, 1.5, 0.1]),
    "rounded": (ROUNDED, [2.0, 1.6, 1.4, 0.25], _unit([0.95, 0.1, 0.25, -0.1]), [-0.1, 1.3, 0.0]),
    "disc": (GRID, [0, 0, 0, DISC_SCALE], _unit([0.85, 0.4, 0.25, 0.15]), [0.0, 1.5, 0.0]),
}
LIVE_PRM = {"sphere": 1, "box": 3, "cylinder": 2, "rounded": 3, "disc": 0}


def fd_view(name):
    """Floor and one body of FD_BODIES -> pose [1,2,7], kind [1,2], prm [1,2,4], grids, grid_id [1,2] (body 1 is the one under test)."""
    k, p, q, pos = FD_BODIES[name]
    pose = np.array([[ref.FLOOR[0], np.concatenate([q, pos])]], np.float64)
    kind = np.array([[ref.FLOOR[1], k]], np.int32)
    prm = np.array([[ref.FLOOR[2], p]], np.float64)
    return pose, kind, prm, [disc_grid()], np.array([[-1, 0 if k == GRID else -1]], np.int32)


def seam_scene(nview, nbody):
    """nbody 1: a sphere at the origin.  nbody 8: floor, wall, a sphere, a rounded box, a cylinder, a box, the disc grid and a sphere
    that the wall hides (no pixel shows it), seen by depth_camera_ref.experiment_camera.  With three views the second shows nothing
    (every body lifted out of the frustum) and the third is the first with the bodies moved a little.
    -> pose [nview,nbody,7], kind, prm [nview,nbody,4], grids, grid_id"""
    if nbody == 1:
        rows = [(np.concatenate([_unit([0.9, 0.1, 0.3, -0.2]), [0.0, 1.0, 0.0]]), SPHERE, [1.5, 0, 0, 0])]
        gid = [-1]
    else:
        at = lambda q, pos: np.concatenate([_unit(q), pos])
        rows = [ref.FLOOR, ref.WALL,
                (at([0.9, 0.2, -0.3, 0.1], [0.0, 1.5, 5.0]), SPHERE, [1.5, 0, 0, 0]),
                (at([0.95, 0.1, 0.25, -0.1], [-3.0, 1.2, 1.0]), ROUNDED, [2.0, 1.6, 1.4, 0.25]),
                (at([0.8, 0.45, 0.2, 0.1], [2.0, 1.2, 6.5]), CYLINDER, [0.7, 1.6, 0, 0]),
                (at([0.95, 0.2, 0.15, 0.2], [-4.0, 1.3, 4.0]), BOX, [2.0, 1.6, 1.2, 0]),
                (at([0.85, 0.4, 0.25, 0.15], [7.0, 1.6, 3.0]), GRID, [0, 0, 0, DISC_SCALE]),
                ref.HIDDEN]
        gid = [-1, -1, -1, -1, -1, -1, 0, -1]
    pose = np.array([[np.asarray(r[0], np.float64) for r in rows]] * nview)
    if nview > 1:
        pose[1, :, 5] += 100.0
    if nview > 2:
        pose[2, 2:, 4:] += 0.05 * np.random.default_rng(5).standard_normal((len(rows) - 2, 3)) if nbody > 1 else 0.05
    kind = np.array([[r[1] for r in rows]] * nview, np.int32)
    prm = np.array([[r[2] for r in rows]] * nview, np.float64)
    return pose, kind, prm, [disc_grid()], np.array([gid] * nview, np.int32)
