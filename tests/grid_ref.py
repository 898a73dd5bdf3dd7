"""float64 numpy oracle of voxel-grid bodies in the depth camera (csrc/depth_camera.hip: dss_depth_render_grids,
dss_grid_block_min), for tests/test_emu_depth_grid.py and tests/test_depth_grid_gpu.py.

field(grid, scale, p)   the trilinear field of geom.h's SHAPE_GRID branch: scale * trilinear(samples) at index position
                        (p / scale + 1) / 2 (n_d - 1), the cell index clamped to [0, n_d - 2].
walk(...)               one grid body under every pixel: the ray is clipped against the query cube and walked cell by cell
                        (vectorised over pixels, at most n0 + n1 + n2 steps, every plane crossing from its integer index).  Along
                        a ray the interpolant of one cell is a cubic in t; it is recovered from four samples in the cell and its
                        first real root in the cell's interval is the hit (polished by Newton steps on the field itself).
render(...)             one view of analytic (depth_camera_ref.body_hits) and grid bodies -> depth, seg, the slope
                        -(d field / dt) / |d| at the hit (the cosine of incidence where the field is a distance) and a mask of
                        DELICATE pixels:
                          a root in a cell with no sign change between the cell's ends (the kernel does not see it, by design);
                          the least of the field along the walked ray within NEAR of 0 without a hit;
                          a hit with slope below COS_MIN;
                          two bodies' hits within NEAR in depth;
                          a value at the slab entry within NEAR of 0.
block_min(grid)         numpy minimum over the corner samples of every block of BLOCK cells per axis.
NEAR, COS_MIN, the rays, the camera and the back-projection are those of tests/depth_camera_ref.py."""
import numpy as np

import depth_camera_ref as ref

NEAR, COS_MIN = ref.NEAR, ref.COS_MIN
GRID, IGR, BLOCK = 7, 6, 4
# tau = 0, 1/3, 2/3, 1 -> coefficients of c0 + c1 tau + c2 tau^2 + c3 tau^3
_VINV = np.linalg.inv(np.vander(np.array([0.0, 1 / 3, 2 / 3, 1.0]), 4, increasing=True))


def field(grid, scale, p):
    grid = np.asarray(grid, np.float64)
    n = np.array(grid.shape)
    u = (np.asarray(p, np.float64) / scale + 1.0) * 0.5 * (n - 1)
    c = np.clip(np.floor(u), 0, n - 2).astype(np.int64)
    return scale * _cell_value(grid, c, u - c)


def _cell_value(grid, c, w):
    """Trilinear value (grid units) in cell c [...,3] at weights w [...,3] (not clamped)."""
    out = 0.0
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wt = (w[..., 0] if dx else 1 - w[..., 0]) * (w[..., 1] if dy else 1 - w[..., 1]) * (w[..., 2] if dz else 1 - w[..., 2])
                out = out + grid[c[..., 0] + dx, c[..., 1] + dy, c[..., 2] + dz] * wt
    return out


def block_min(grid):
    grid = np.asarray(grid, np.float64)
    nb = [-(-(n - 1) // BLOCK) for n in grid.shape]
    out = np.zeros(nb)
    for i in range(nb[0]):
        for j in range(nb[1]):
            for k in range(nb[2]):
                out[i, j, k] = grid[BLOCK * i:BLOCK * i + BLOCK + 1, BLOCK * j:BLOCK * j + BLOCK + 1, BLOCK * k:BLOCK * k + BLOCK + 1].min()
    return out.reshape(-1)


def _first_root(coef):
    """First real root in [0, 1] of c0 + c1 x + c2 x^2 + c3 x^3, or None."""
    r = np.roots(coef[::-1]) if np.any(coef[1:] != 0) else np.array([])
    r = r[np.abs(r.imag) < 1e-9].real
    r = r[(r >= -1e-12) & (r <= 1 + 1e-12)]
    return float(np.clip(r.min(), 0.0, 1.0)) if len(r) else None


def walk(grid, scale, pose, o, d, L, znear=0.1, zfar=100.0):
    """One grid body: t [H,W] (inf: no hit), slope [H,W], delicate [H,W], entry [H,W] the field at the slab entry (inf where the
    ray misses the query cube)."""
    grid = np.asarray(grid, np.float64)
    shape = L.shape
    n = np.array(grid.shape)
    R = ref.quat_to_mat(np.asarray(pose[:4], np.float64))
    ob = R.T @ (o - np.asarray(pose[4:], np.float64))
    db = (d @ R).reshape(-1, 3)
    Lf = L.reshape(-1)
    N = len(db)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-scale - ob) / db, (scale - ob) / db
    par = db == 0
    tlo = np.where(par, np.where(np.abs(ob) <= scale, -np.inf, np.inf), np.minimum(ta, tb))
    thi = np.where(par, np.where(np.abs(ob) <= scale, np.inf, -np.inf), np.maximum(ta, tb))
    t0, t1 = np.maximum(tlo.max(1), znear), np.minimum(thi.min(1), zfar)
    t, slope = np.full(N, np.inf), np.zeros(N)
    delicate, entry = np.zeros(N, bool), np.full(N, np.inf)
    least = np.full(N, np.inf)
    live = np.nonzero(t0 <= t1)[0]
    h = 0.5 * (n - 1)
    xo, xd = (ob / scale + 1.0) * h, db / scale * h
    s = np.sign(xd).astype(np.int64)
    c = np.clip(np.floor(xo + t0[:, None] * xd), 0, n - 2).astype(np.int64)
    t_in = t0.copy()
    # the entry value
    entry[live] = scale * _cell_value(grid, c[live], (xo + t_in[live, None] * xd[live]) - c[live])
    inside = live[entry[live] <= 0]
    t[inside] = t0[inside]
    delicate[live] |= np.abs(entry[live]) < NEAR
    live = live[entry[live] > 0]
    for _ in range(int(n.sum()) + 1):
        if not len(live):
            break
        cl, sl = c[live], s[live]
        with np.errstate(divide="ignore", invalid="ignore"):
            tn = np.where(sl != 0, (cl + (sl > 0) - xo) / xd[live], np.inf)
        axis = tn.argmin(1)
        t_out = tn[np.arange(len(live)), axis]
        t_ex = np.minimum(np.maximum(t_out, t_in[live]), t1[live])
        dt = t_ex - t_in[live]
        # four samples of the cell's cubic along the ray
        f = np.stack([_cell_value(grid, cl, (xo + (t_in[live] + k / 3 * dt)[:, None] * xd[live]) - cl) for k in range(4)], 1) * scale
        least[live] = np.minimum(least[live], np.minimum(f[:, 0], f[:, 3]))
        corner_min = np.min([grid[cl[:, 0] + a, cl[:, 1] + b, cl[:, 2] + e] for a in (0, 1) for b in (0, 1) for e in (0, 1)], 0) * scale
        done = np.zeros(len(live), bool)
        for i in np.nonzero(corner_min < NEAR)[0]:      # (a cell whose corners are all positive holds no root: a convex combination)
            coef = _VINV @ f[i]
            if dt[i] > 0:      # the least of the cubic inside the cell
                crit = np.roots((coef[1:] * np.arange(1, 4))[::-1]) if coef[3] != 0 or coef[2] != 0 else np.array([])
                for x in crit[np.abs(crit.imag) < 1e-12].real:
                    if 0 < x < 1:
                        least[live[i]] = min(least[live[i]], float(np.polyval(coef[::-1], x)))
            x = _first_root(coef)
            if x is None:
                continue
            g = live[i]
            der = lambda y: coef[1] + 2 * coef[2] * y + 3 * coef[3] * y * y
            for _k in range(3):      # Newton on the field itself (the cubic's derivative is exact up to rounding)
                if der(x) != 0:
                    fx = scale * _cell_value(grid, cl[i], (xo + (t_in[g] + x * dt[i]) * xd[g]) - cl[i])
                    x = min(max(x - fx / der(x), 0.0), 1.0)
            t[g] = t_in[g] + x * dt[i]
            slope[g] = -der(x) / dt[i] / Lf[g] if dt[i] > 0 else 0.0
            if f[i, 3] > 0:
                delicate[g] = True      # in and out again within one cell
            done[i] = True
        # next cell
        ended = done | ~(t_out < t1[live])
        cl = cl.copy()
        cl[np.arange(len(live)), axis] += sl[np.arange(len(live)), axis]
        ended |= ((cl < 0) | (cl > n - 2)).any(1)
        c[live], t_in[live] = cl, t_ex
        live = live[~ended]
    miss = ~np.isfinite(t)
    delicate |= miss & (least < NEAR)
    delicate |= ~miss & (t > t0) & (slope < COS_MIN)
    return t.reshape(shape), slope.reshape(shape), delicate.reshape(shape), entry.reshape(shape)


def render(pose, shape_type, prm, grids, grid_id, cam, fx, fy, cx, cy, W, H, znear=0.1, zfar=100.0):
    """One view: pose [nb,7], shape_type [nb], prm [nb,4], grids a list of arrays, grid_id [nb] ->
    dict(depth, seg, cos, delicate [H,W]; entry [nb,H,W], the field at the slab entry of the grid bodies)."""
    o, d, L = ref.rays(cam, fx, fy, cx, cy, W, H)
    ts, cosines, entries, delicate = [], [], [], np.zeros((H, W), bool)
    for j in range(len(shape_type)):
        if int(shape_type[j]) in (GRID, IGR):
            t, c, dl, en = walk(grids[int(grid_id[j])], float(prm[j][3]), pose[j], o, d, L, znear, zfar)
            delicate |= dl
        else:
            t, c, clear = ref.body_hits(int(shape_type[j]), prm[j], pose[j], o, d, L, zfar)
            delicate |= (np.isfinite(t) & (c < COS_MIN)) | (np.abs(clear) < NEAR)
            en = np.full((H, W), np.inf)
        hit = np.isfinite(t)
        assert not hit.any() or (t[hit].min() > znear + 1.0 and t[hit].max() < zfar - 1.0), "a surface near the clipping planes"
        ts.append(t); cosines.append(c); entries.append(en)
    ts, cosines = np.stack(ts), np.stack(cosines)
    order = np.sort(ts, 0)
    if len(ts) > 1:
        both = np.isfinite(order[1])
        delicate[both] |= order[1][both] - order[0][both] < NEAR
    seg = ts.argmin(0)
    depth = np.take_along_axis(ts, seg[None], 0)[0]
    cos = np.take_along_axis(cosines, seg[None], 0)[0]
    miss = ~np.isfinite(depth)
    return dict(depth=np.where(miss, 0.0, depth), seg=np.where(miss, -1, seg).astype(np.int32), cos=cos, delicate=delicate,
                entry=np.stack(entries))


# ---- the scene shared by the emulator and the GPU test ---------------------------------------------------------------------------
def torus_grid(shape=(33, 25, 21), major=0.55, minor=0.22):
    """Grid A: the sampled distance to a torus around the unit cube's z axis; non-cubic, 8 x 6 x 5 whole blocks."""
    x, y, z = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")
    return np.hypot(np.hypot(x, y) - major, z) - minor


def sphere_grid(n=12, centre=(0.15, -0.1, 0.2), rad=0.5):
    """Grid B: an off-centre sphere on 12^3 samples: 11 cells per axis, so the last block of every axis is partial."""
    x, y, z = np.meshgrid(*[np.linspace(-1.0, 1.0, n)] * 3, indexing="ij")
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - rad


TORUS_SCALE, SPHERE_SCALE = 2.5, 1.5


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def grid_views():
    """Three views of floor, wall, the torus (grid 0) and a fourth body: the sphere grid (grid 1) beside it; the sphere grid with
    the torus partly behind the wall; an analytic rounded box next to the torus.
    -> pose [3,4,7], shape_type [3,4], prm [3,4,4], grids, grid_id [3,4]"""
    tilt = _unit([0.83, 0.41, -0.23, 0.30])
    torus = lambda pos, q=tilt: (np.concatenate([q, pos]), GRID, [0.0, 0.0, 0.0, TORUS_SCALE])
    ball = lambda pos: (np.concatenate([_unit([0.9, -0.2, 0.3, 0.1]), pos]), GRID, [0.0, 0.0, 0.0, SPHERE_SCALE])
    box = (np.concatenate([_unit([0.95, 0.1, 0.25, -0.1]), [0.3, 1.6, 6.3]]), ref.ROUNDED, [2.0, 1.6, 1.2, 0.2])
    rows = [(ref.FLOOR, ref.WALL, torus([1.5, 3.2, 5.0]), ball([3.2, 1.4, 7.2])),
            (ref.FLOOR, ref.WALL, torus([3.0, 4.0, 2.6], _unit([0.7, -0.3, 0.55, 0.2])), ball([0.5, 2.5, 6.5])),
            (ref.FLOOR, ref.WALL, torus([2.2, 3.0, 4.6]), box)]
    pose = np.array([[b[0] for b in r] for r in rows], np.float64)
    kind = np.array([[b[1] for b in r] for r in rows], np.int32)
    prm = np.array([[b[2] for b in r] for r in rows], np.float64)
    gid = np.array([[-1, -1, 0, 1], [-1, -1, 0, 1], [-1, -1, 0, -1]], np.int32)
    return pose, kind, prm, [torus_grid(), sphere_grid()], gid


def pooled(grids):
    """-> off [ngrid] int32, dims [ngrid,3] int32, data, blk_off [ngrid] int32, nblk: the layout the kernels take."""
    sizes = [g.size for g in grids]
    dims = np.array([g.shape for g in grids], np.int32)
    nblk = np.prod(-(-(dims.astype(np.int64) - 1) // BLOCK), axis=1)
    return (np.cumsum([0] + sizes[:-1]).astype(np.int32), dims, np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in grids]),
            np.concatenate([[0], np.cumsum(nblk)[:-1]]).astype(np.int32), int(nblk.sum()))


def check_view(depth, seg, want, pose, shape_type, prm, grids, grid_id, cam, fx, fy, cx, cy, W=None, H=None, name=""):
    """The checks of one rendered view against render()'s result `want`; prints the observed worst values before it asserts."""
    npx = depth.size
    ok = ~want["delicate"]
    is_grid = np.isin(shape_type, (GRID, IGR))
    on_grid = ok & (want["seg"] >= 0) & is_grid[np.maximum(want["seg"], 0)]
    on_prim = ok & (want["seg"] >= 0) & ~is_grid[np.maximum(want["seg"], 0)] & (want["cos"] >= COS_MIN)
    err = np.abs(depth - want["depth"])
    gerr = err[on_grid].max() if on_grid.any() else 0.0
    perr = err[on_prim].max() if on_prim.any() else 0.0
    wrong = int((seg != want["seg"])[ok].sum())
    world = ref.backproject(depth, cam, fx, fy, cx, cy)
    gphi = pphi = 0.0
    for j in range(len(shape_type)):
        m = seg == j
        if not m.any():
            continue
        pb = (world[m] - pose[j][4:]) @ ref.quat_to_mat(pose[j][:4])
        if is_grid[j]:
            gphi = max(gphi, np.abs(field(grids[int(grid_id[j])], float(prm[j][3]), pb)).max())
        else:
            pphi = max(pphi, np.abs(ref.sdf(int(shape_type[j]), prm[j], pb)).max())
    ndel, ncap = int(want["delicate"].sum()), int((seg == -2).sum())
    print("%s: %d pixels, %d delicate, %d capped, hits per body %s, class errors %d, depth err grid %.2e analytic %.2e, "
          "surface |field| grid %.2e analytic %.2e" % (name, npx, ndel, ncap, [int((seg == j).sum()) for j in range(len(shape_type))],
                                                       wrong, gerr, perr, gphi, pphi))
    assert ndel <= 0.01 * npx, "more than 1 % delicate pixels: choose other poses"
    assert ncap == 0, "a pixel with seg = -2"
    assert wrong == 0, "hit / miss / body differs from the oracle outside the delicate pixels"
    assert gerr <= 1e-10 and gphi <= 1e-10, (gerr, gphi)
    assert perr <= 1e-8 and pphi <= 1e-9, (perr, pphi)
    assert np.all(depth[seg < 0] == 0.0)
