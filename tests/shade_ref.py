"""float64 numpy oracle of the colour camera (csrc/shade_camera.hip: dss_shade_render), and the checks that
tests/test_emu_shade.py (emulator) and tests/test_shade_gpu.py (device) both run.

shade_view(...)   one view, from the depth / seg images of the depth camera itself: per pixel the normal, per light the cosine c_k
                  and the visibility V_k, the shade min(1, ambient + sum_k I_k V_k max(0, c_k)), rgb = floor(255 colour shade + 0.5),
                  and a mask of DELICATE pixels.
                    normals   analytic bodies: central differences of depth_camera_ref.sdf, h = 1e-5; grid bodies: the closed-form
                              gradient of the trilinear interpolant of grid_ref.field's cell;
                    shadows   the least of every body's field along the ray from x + bias n towards the light: ternary search for the
                              four convex fields (depth_camera_ref._ray_min), dense samples of grid_ref.field (at most 2.5e-3 apart, a
                              sixtieth of the smallest cell used here) with a ternary search around the least sample for a grid;
                    delicate  delicate for the depth oracle already; the normal changes by more than 1e-5 when the hit moves 1e-7 along
                              either tangent (a crease, or the face between two grid cells); some |n . l| < 1e-6; some shadow-ray minimum
                              within 1e-6 of zero.

A `backend` is a function call(args) -> rc: args maps the C argument names of dss_shade_render to numpy arrays (None: a null
pointer) and scalars, the four outputs are numpy arrays it fills in place; and render(pose, kind, prm, grids, gid, cam, fx, fy, cx, cy,
W, H) -> (depth, seg) of the depth camera behind it.  Every call here allocates the outputs with one view more than it asks for,
filled with FILL, and asserts that this guard view is unchanged."""
import numpy as np

import depth_camera_ref as ref
import grid_ref as G

H_DIFF, CREASE_STEP, CREASE_TOL, NEAR = 1e-5, 1e-7, 1e-5, 1e-6
FILL = dict(normal=-7.0, shade=-7.0, rgb=7, flags=7)
BIAS = 1e-3


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def grid_gradient(grid, scale, p):
    """Body-frame gradient (not normalised) of grid_ref.field at p [N,3]: d/dp of scale * trilinear((p / scale + 1) / 2 (n - 1))."""
    grid = np.asarray(grid, np.float64)
    n = np.array(grid.shape)
    u = (np.asarray(p, np.float64) / scale + 1.0) * 0.5 * (n - 1)
    c = np.clip(np.floor(u), 0, n - 2).astype(np.int64)
    w = u - c
    v = lambda a, b, e: grid[c[:, 0] + a, c[:, 1] + b, c[:, 2] + e]
    g = np.zeros_like(w)
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        for b1 in (0, 1):
            for b2 in (0, 1):
                hi, lo = [0, 0, 0], [0, 0, 0]
                hi[ax], lo[ax] = 1, 0
                hi[o1] = lo[o1] = b1; hi[o2] = lo[o2] = b2
                wt = (w[:, o1] if b1 else 1 - w[:, o1]) * (w[:, o2] if b2 else 1 - w[:, o2])
                g[:, ax] += wt * (v(*hi) - v(*lo))
    return g * 0.5 * (n - 1)


def body_normals(kind, prm, grid, pb):
    """Unit body-frame normals at body-frame points pb [N,3]."""
    if kind in (G.GRID, G.IGR):
        g = grid_gradient(grid, float(prm[3]), pb)
    else:
        g = np.stack([(ref.sdf(kind, prm, pb + H_DIFF * u) - ref.sdf(kind, prm, pb - H_DIFF * u)) / (2 * H_DIFF) for u in np.eye(3)], -1)
    return _unit(g)


def _grid_ray_min(grid, scale, ob, db, T):
    """Least of grid_ref.field along ob + t db (|db| = 1), t in [0, T] within the query cube; inf where the ray misses the cube."""
    N = len(ob)
    out = np.full(N, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-scale - ob) / db, (scale - ob) / db
    par = db == 0
    tlo = np.where(par, np.where(np.abs(ob) <= scale, -np.inf, np.inf), np.minimum(ta, tb)).max(1)
    thi = np.where(par, np.where(np.abs(ob) <= scale, np.inf, -np.inf), np.maximum(ta, tb)).min(1)
    t0, t1 = np.maximum(tlo, 0.0), np.minimum(thi, T)
    live = np.nonzero(t0 <= t1)[0]
    K = int(np.ceil(2 * np.sqrt(3.0) * scale / 2.5e-3)) + 1
    f = lambda i, t: G.field(grid, scale, np.clip(ob[i, None] + t[..., None] * db[i, None], -scale, scale))
    for s in range(0, len(live), 128):
        i = live[s:s + 128]
        t = t0[i, None] + (t1[i] - t0[i])[:, None] * np.linspace(0.0, 1.0, K)[None]
        v = np.stack([f(j, tt) for j, tt in zip(i, t)])
        k = v.argmin(1)
        lo, hi = t[np.arange(len(i)), np.maximum(k - 1, 0)], t[np.arange(len(i)), np.minimum(k + 1, K - 1)]
        g = lambda tt: G.field(grid, scale, np.clip(ob[i] + tt[:, None] * db[i], -scale, scale))
        for _ in range(60):
            a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
            left = g(a) <= g(b)
            hi = np.where(left, b, hi); lo = np.where(left, lo, a)
        out[i] = np.minimum(v.min(1), g(0.5 * (lo + hi)))
    return out


def shadow_minima(pose, kind, prm, grids, gid, so, l, zfar):
    """[nbody, N]: the least of every body's field along so [N,3] + t l, t in [0, zfar]."""
    out = []
    for j in range(len(kind)):
        R = ref.quat_to_mat(np.asarray(pose[j][:4], np.float64))
        ob, db = (so - pose[j][4:]) @ R, np.broadcast_to(l @ R, so.shape).copy()
        if int(kind[j]) in (G.GRID, G.IGR):
            out.append(_grid_ray_min(grids[int(gid[j])], float(prm[j][3]), ob, db, zfar))
        else:
            out.append(ref._ray_min(int(kind[j]), np.asarray(prm[j], np.float64), ob, db, zfar)[1])
    return np.array(out)


def world_normals(pose, kind, prm, grids, gid, x, seg):
    n = np.zeros(x.shape)
    for j in range(len(kind)):
        m = seg == j
        if m.any():
            R = ref.quat_to_mat(np.asarray(pose[j][:4], np.float64))
            grid = grids[int(gid[j])] if int(kind[j]) in (G.GRID, G.IGR) else None
            n[m] = body_normals(int(kind[j]), np.asarray(prm[j], np.float64), grid, (x[m] - pose[j][4:]) @ R) @ R.T
    return n


def shade_view(depth, seg, pose, kind, prm, grids, gid, cam, fx, fy, cx, cy, W, H, color, lights, ambient, background, shadows=True,
               bias=BIAS, zfar=100.0, depth_delicate=None):
    """One view -> dict(normal [H,W,3], c, V, dark [nlight,H,W] (dark: the least shadow-ray field per body [nlight,nbody,H,W]), shade,
    rgb, delicate)."""
    lights = np.asarray(lights, np.float64).reshape(-1, 4)
    hit = (seg >= 0) & (seg < len(kind))
    x = ref.backproject(depth, cam, fx, fy, cx, cy)      # o + depth d
    sg = np.where(hit, seg, -1)
    n = world_normals(pose, kind, prm, grids, gid, x, sg)
    delicate = np.zeros((H, W), bool) if depth_delicate is None else depth_delicate.copy()
    # creases: the normal 1e-7 to either side along two tangents
    a = np.where(np.abs(n[..., :1]) < 0.9, [1.0, 0, 0], [0, 1.0, 0])
    t1 = np.cross(n, a); t1 = t1 / np.maximum(np.linalg.norm(t1, axis=-1, keepdims=True), 1e-300)
    t2 = np.cross(n, t1)
    for t in (t1, -t1, t2, -t2):
        delicate |= hit & (np.abs(world_normals(pose, kind, prm, grids, gid, x + CREASE_STEP * t, sg) - n).max(-1) > CREASE_TOL)
    nl = len(lights)
    c = np.zeros((nl, H, W)); V = np.ones((nl, H, W)); dark = np.full((nl, len(kind), H, W), np.inf)
    so = x + bias * n
    for k in range(nl):
        l = _unit(lights[k, :3])
        c[k] = n @ l
        delicate |= hit & (np.abs(c[k]) < NEAR)
        m = hit & (c[k] > 0)
        if shadows and m.any():
            mins = shadow_minima(pose, kind, prm, grids, gid, so[m], l, zfar)
            dark[k][:, m] = mins
            V[k][m] = (mins >= 0).all(0)
            delicate[m] |= (np.abs(mins) < NEAR).any(0)
    shade = np.minimum(1.0, ambient + (lights[:, 3, None, None] * V * np.maximum(c, 0.0)).sum(0))
    shade = np.where(hit, shade, 0.0)
    col = np.asarray(color, np.float64)[np.maximum(sg, 0)]
    rgb = np.where(hit[..., None], np.floor(255.0 * col * shade[..., None] + 0.5), np.floor(255.0 * np.asarray(background, np.float64) + 0.5))
    return dict(normal=n, c=c, V=V, dark=dark, shade=shade, rgb=rgb.astype(np.uint8), delicate=delicate, hit=hit, seg=sg)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
LIGHT = [[-1.0, 2.0, 1.5, 0.8]]      # towards the light (not unit), intensity: from behind the wall, over it, onto the floor in front
FOUR_LIGHTS = LIGHT + [[1.0, 1.0, 0.2, 0.3], [0.3, 1.0, -1.0, 0.25], [0.1, -1.0, 0.2, 0.5]]      # (the last one shines from below)
AMBIENT, BACKGROUND = 0.1, (0.2, 0.4, 1.0)
COLORS = np.array([[0.8, 0.8, 0.8], [0.9, 0.6, 0.3], [0.2, 0.7, 0.3], [0.3, 0.3, 0.9], [1.0, 1.0, 1.0], [0.5, 0.1, 0.6], [0.1, 0.9, 0.9],
                   [0.7, 0.7, 0.1]])
_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)


def eight_bodies():
    """One view of DC_MAX_BODY bodies: floor, wall, a rounded cube and five small spheres above the floor in front of the wall."""
    pose, kind, prm = ref.bounce_views()
    rows = [(pose[1, j], kind[1, j], prm[1, j]) for j in range(3)]
    for i in range(5):
        rows.append(([1.0, 0, 0, 0, 6.5 + 0.5 * i, 0.6 + 0.3 * i, 4.0 - 1.7 * i], ref.SPHERE, [0.35 + 0.05 * i, 0, 0, 0]))
    return (np.array([[r[0] for r in rows]], np.float64), np.array([[r[1] for r in rows]], np.int32), np.array([[r[2] for r in rows]], np.float64))


def torus_scene(shape):
    """Floor and a torus sampled on `shape`, tilted, above it -> pose [1,2,7], kind, prm, grids, gid."""
    q = G._unit([0.83, 0.41, -0.23, 0.30])
    rows = [ref.FLOOR, (np.concatenate([q, [1.5, 3.2, 5.0]]), G.GRID, [0.0, 0.0, 0.0, G.TORUS_SCALE])]
    return (np.array([[r[0] for r in rows]], np.float64), np.array([[r[1] for r in rows]], np.int32), np.array([[r[2] for r in rows]], np.float64),
            [G.torus_grid(shape)], np.array([[-1, 0]], np.int32))


TORUS_LIGHT = [[-1.0, 0.35, 0.4, 0.9]]      # from the side


def arguments(pose, kind, prm, cam, depth, seg, grids=None, gid=None, lights=LIGHT, shadows=1, fx=64.375, fy=64.375, cx=39.5, cy=29.5,
              W=80, H=60, ambient=AMBIENT, background=BACKGROUND, bias=BIAS, zfar=100.0, colors=None):
    """The argument dict of one call, outputs with a guard view."""
    nview, nbody = kind.shape
    lights = np.asarray(lights, np.float64).reshape(-1, 4)
    A = dict(nview=nview, nbody=nbody, pose=_c(pose), shape_type=_c(kind, np.int32), prm=_c(prm), cam=_c(cam), fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H,
             zfar=zfar, grid_id=None, ngrid=0, grid_off=None, grid_dims=None, grid_data=None, blk_off=None, blk_min=None,
             depth=_c(depth), seg=_c(seg, np.int32),
             color=np.array(np.broadcast_to(COLORS[:nbody] if colors is None else colors, (nview, nbody, 3)), np.float64, order="C"), nlight=len(lights),
             light=_c(lights) if len(lights) else None, ambient=ambient, background=_c(background), shadows=int(shadows), shadow_bias=bias)
    if grids is not None:
        off, dims, data, blk_off, nblk = G.pooled(grids)
        bmin = np.concatenate([G.block_min(g) for g in grids])      # (equal to dss_grid_block_min's: the depth tests assert it)
        A.update(grid_id=_c(gid, np.int32), ngrid=len(grids), grid_off=off, grid_dims=dims, grid_data=data, blk_off=blk_off, blk_min=_c(bmin))
    A.update(outputs(nview, H, W))
    return A


def outputs(nview, H, W):
    return dict(normal=np.full((nview + 1, H, W, 3), FILL["normal"]), shade=np.full((nview + 1, H, W), FILL["shade"]),
                rgb=np.full((nview + 1, H, W, 3), FILL["rgb"], np.uint8), flags=np.full((nview + 1, H, W), FILL["flags"], np.uint8))


def untouched(A, views=None):
    """Are the outputs (all of them, or from view `views` on) still at their fill?"""
    return all(np.all(A[k][views:] == FILL[k]) for k in FILL if A[k] is not None)


def run(call, A):
    """-> the outputs without their guard view, which must have kept its fill."""
    rc = call(A)
    assert rc == 0, rc
    assert untouched(A, A["nview"]), "written past the last view"
    return {k: A[k][:A["nview"]] for k in FILL}


def check_view(got, want, kind, name="", cap=True):
    """The checks of one shaded view (got: normal, shade, rgb, flags [H,W,..]) against shade_view()'s result; prints before it asserts."""
    ok, hit = ~want["delicate"], want["hit"]
    npx = hit.size
    is_grid = np.isin(kind, (G.GRID, G.IGR))
    on_grid = hit & is_grid[np.maximum(want["seg"], 0)]
    nerr = np.abs(got["normal"] - want["normal"]).max(-1)
    ea = nerr[ok & hit & ~on_grid].max() if (ok & hit & ~on_grid).any() else 0.0
    eg = nerr[ok & on_grid].max() if (ok & on_grid).any() else 0.0
    unit = np.abs(np.linalg.norm(got["normal"], axis=-1) - 1.0)[hit].max() if hit.any() else 0.0
    serr = np.abs(got["shade"] - want["shade"])[ok].max()
    # (shade to 1e-7 pins the visibility: outside the delicate pixels a light's own term I_k c_k is at least 0.25 * 1e-6)
    cerr =np.abs(got["rgb"].astype(int) - want["rgb"].astype(int)).max(-1)
    print("%s: %d pixels, %d hit, %d delicate, normal err analytic %.2e grid %.2e, |n| - 1 %.2e, shade err %.2e, colour levels off %d, flags %s"
          % (name, npx, int(hit.sum()), int(want["delicate"].sum()), ea, eg, unit, serr, int(cerr[ok].max()), np.unique(got["flags"]).tolist()))
    assert not cap or want["delicate"].sum() <= 0.01 * npx, "more than 1 % delicate pixels: choose another seed or light"
    assert ea <= 1e-7 and eg <= 1e-9, (ea, eg)
    assert unit <= 1e-12, unit
    assert np.all(got["normal"][~hit] == 0.0) and np.all(got["shade"][~hit] == 0.0)
    assert serr <= 1e-7, serr
    assert cerr[ok].max() <= 1
    assert np.array_equal(got["rgb"][~hit], want["rgb"][~hit]), "a miss is not the background colour"
    assert not got["flags"].any(), "a flag is set"


def visibility(got_shade, want, lights, ambient):
    """The device's V for a single light, from its shade: (shade - ambient) / (I c) where that is defined (c > 1e-6, no clamp)."""
    lights = np.asarray(lights, np.float64).reshape(-1, 4)
    assert len(lights) == 1
    full = lights[0, 3] * want["c"][0]
    m = want["hit"] & ~want["delicate"] & (want["c"][0] > 1e-6) & (ambient + full < 1.0)
    return m, np.where(m, (got_shade - ambient) / np.where(m, full, 1.0), 0.0)
