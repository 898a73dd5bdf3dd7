"""float64 numpy oracle of the depth camera (csrc/depth_camera.hip) for the tests.

render(...)            per pixel the exact depth of the nearest surface, the body hit, the cosine of incidence and a mask of
                       DELICATE pixels, whose class (hit or miss, which body) an error of 1e-6 could change:
                         a hit with cosine < 0.05, a ray whose least distance to a body is within 1e-6 of zero (a miss passing
                         that near a surface, or a hit no deeper than that), two bodies' hits within 1e-6 in depth.
                       Sphere and box: closed form (quadratic, slab test).  Rounded box and cylinder: the SDF along a ray is
                       convex, so its minimum comes from a ternary search; where it is negative the root is bracketed from
                       below by numpy sphere tracing and finished by bisection to 1e-13.
observed_points(...)   match_pointcloud lines 168-187 (experiments/trajectory_fitting/optim_pointcloud.py) in float64:
                       scipy.ndimage.binary_erosion itself, pixels of depth 0 dropped, back-projection, y and z flipped, cam.
The SDFs here are the plain Euclidean distances in world units (no unit frame, no query cube): the fields of the four shapes
the renderer accepts are exactly these inside their query cubes, and every surface lies inside its cube."""
import numpy as np
import scipy.ndimage

BOX, SPHERE, CYLINDER, ROUNDED = 0, 1, 2, 3
COS_MIN, NEAR = 0.05, 1e-6


def quat_to_mat(q):
    r, i, j, k = q
    s = 2.0 / np.dot(q, q)
    return np.array([[1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
                     [s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)],
                     [s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]])


def sdf(kind, prm, p):
    """Distance of body-frame points p [..., 3] to the body; prm [4] = three parameters + the corner radius."""
    if kind == SPHERE:
        return np.linalg.norm(p, axis=-1) - prm[0]
    if kind == CYLINDER:
        q = np.stack([np.hypot(p[..., 0], p[..., 1]) - prm[0], np.abs(p[..., 2]) - prm[1] / 2], -1)
        r = 0.0
    else:
        r = prm[3] if kind == ROUNDED else 0.0
        q = np.abs(p) - (np.asarray(prm[:3]) / 2 - r)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0) - r


def rays(cam, fx, fy, cx, cy, W, H):
    """-> origin [3], direction [H,W,3] = Rc (nx, -ny, -1) (a hit at parameter t has depth t), its length [H,W]."""
    cam = np.asarray(cam, np.float64).reshape(4, 4)
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    nx, ny = (col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy
    d = np.stack([nx, -ny, -np.ones_like(nx)], -1) @ cam[:3, :3].T
    return cam[:3, 3].copy(), d, np.sqrt(nx * nx + ny * ny + 1.0)


def _ray_min(kind, prm, ob, db, T):
    """Least SDF along p(t) = ob + t db, 0 <= t <= T (convex in t) -> (t_min, phi_min)."""
    lo, hi = np.zeros(db.shape[:-1]), np.full(db.shape[:-1], float(T))
    f = lambda t: sdf(kind, prm, ob + t[..., None] * db)
    for _ in range(130):      # (2/3)^130 T < 1e-20
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        left = f(a) <= f(b)
        hi = np.where(left, b, hi); lo = np.where(left, lo, a)
    t = 0.5 * (lo + hi)
    return t, f(t)


def body_hits(kind, prm, pose, o, d, L, zfar=100.0):
    """One body: t [H,W] (inf where the ray misses), cos [H,W] of incidence at the hit, clear [H,W] the least SDF along the
    ray (inf where it was not needed: box hits, and box misses that also miss the box grown by 1e-3)."""
    prm = np.asarray(prm, np.float64)
    R = quat_to_mat(np.asarray(pose[:4], np.float64))
    ob = R.T @ (o - np.asarray(pose[4:], np.float64))
    db = d @ R
    a, b = (db * db).sum(-1), db @ ob
    t = np.full(L.shape, np.inf); cos = np.zeros(L.shape); clear = np.full(L.shape, np.inf)
    if kind == SPHERE:
        r = prm[0]
        disc = b * b - a * (ob @ ob - r * r)
        hit = (disc >= 0) & (b < 0)
        th = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
        n = (ob + th[..., None] * db) / r
        t[hit] = th[hit]
        cos[hit] = (-(n * db).sum(-1) / L)[hit]
        tc = np.maximum(-b / a, 0.0)
        clear = np.linalg.norm(ob + tc[..., None] * db, axis=-1) - r
    elif kind == BOX:
        h = prm[:3] / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (-h - ob) / db, (h - ob) / db
        par = db == 0
        tlo = np.where(par, np.where(np.abs(ob) <= h, -np.inf, np.inf), np.minimum(ta, tb))
        thi = np.where(par, np.where(np.abs(ob) <= h, np.inf, -np.inf), np.maximum(ta, tb))
        tin, tout = tlo.max(-1), thi.min(-1)
        hit = (tin <= tout) & (tin > 0)
        t[hit] = tin[hit]
        axis = tlo.argmax(-1)
        cos[hit] = (np.abs(np.take_along_axis(db, axis[..., None], -1))[..., 0] / L)[hit]
        with np.errstate(divide="ignore", invalid="ignore"):      # misses that hit the box grown by 1e-3: the silhouette's rim
            ta, tb = (-h - 1e-3 - ob) / db, (h + 1e-3 - ob) / db
        glo = np.where(par, np.where(np.abs(ob) <= h + 1e-3, -np.inf, np.inf), np.minimum(ta, tb)).max(-1)
        ghi = np.where(par, np.where(np.abs(ob) <= h + 1e-3, np.inf, -np.inf), np.maximum(ta, tb)).min(-1)
        near = ~hit & (glo <= ghi) & (ghi > 0)
        if near.any():
            clear[near] = _ray_min(kind, prm, ob, db[near], zfar)[1]
    else:
        tmin, fmin = _ray_min(kind, prm, ob, db, zfar)
        clear = fmin
        hit = fmin < 0
        if hit.any():
            dh, lo, hi = db[hit], np.zeros(int(hit.sum())), tmin[hit]
            f = lambda s: sdf(kind, prm, ob + s[..., None] * dh)
            for _ in range(64):      # sphere tracing: never passes the surface
                lo = lo + np.maximum(f(lo), 0.0) / L[hit]
            lo = np.minimum(lo, hi)
            while (hi - lo).max() > 1e-13:
                mid = 0.5 * (lo + hi)
                out = f(mid) > 0
                lo = np.where(out, mid, lo); hi = np.where(out, hi, mid)
            th = 0.5 * (lo + hi)
            p = ob + th[..., None] * dh
            e = 1e-6      # the normal by central differences (it only decides cos < 0.05)
            g = np.stack([(sdf(kind, prm, p + e * u) - sdf(kind, prm, p - e * u)) / (2 * e) for u in np.eye(3)], -1)
            g /= np.linalg.norm(g, axis=-1, keepdims=True)
            t[hit] = th
            cos[hit] = -(g * dh).sum(-1) / L[hit]
    return t, cos, clear


def render(pose, shape_type, prm, cam, fx, fy, cx, cy, W, H, znear=0.1, zfar=100.0):
    """One view: pose [nb,7], shape_type [nb], prm [nb,4] -> dict(depth, seg, cos, delicate) of [H,W] images."""
    o, d, L = rays(cam, fx, fy, cx, cy, W, H)
    ts, delicate = [], np.zeros((H, W), bool)
    cosines = []
    for j in range(len(shape_type)):
        t, c, clear = body_hits(int(shape_type[j]), prm[j], pose[j], o, d, L, zfar)
        hit = np.isfinite(t)
        assert not hit.any() or (t[hit].min() > znear + 1.0 and t[hit].max() < zfar - 1.0), "a surface near the clipping planes"
        delicate |= (hit & (c < COS_MIN)) | (np.abs(clear) < NEAR)
        ts.append(t); cosines.append(c)
    ts, cosines = np.stack(ts), np.stack(cosines)
    order = np.sort(ts, 0)
    if len(ts) > 1:
        both = np.isfinite(order[1])
        delicate[both] |= order[1][both] - order[0][both] < NEAR
    seg = ts.argmin(0)
    depth = np.take_along_axis(ts, seg[None], 0)[0]
    cos = np.take_along_axis(cosines, seg[None], 0)[0]
    miss = ~np.isfinite(depth)
    return dict(depth=np.where(miss, 0.0, depth), seg=np.where(miss, -1, seg).astype(np.int32), cos=cos, delicate=delicate)


def backproject(depth, cam, fx, fy, cx, cy):
    """World-frame points [H,W,3] of a depth image (Recorder3D.get_pointcloud in float64, then match_pointcloud's flip and cam)."""
    cam = np.asarray(cam, np.float64).reshape(4, 4)
    H, W = depth.shape
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    nx, ny = (col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy
    pc = np.stack([nx * depth, -(ny * depth), -depth, np.ones_like(depth)], -1)
    return (pc @ cam.T)[..., :3]


def observed_points(depth, seg, body, cam, fx, fy, cx, cy):
    """-> (pts [N,3], seg_off [nview+1]) of depth / seg [nview,H,W], row-major pixel order per view."""
    pts, off = [], [0]
    for dimg, simg in zip(depth, seg):
        mask = scipy.ndimage.binary_erosion(simg == body) & (dimg != 0)
        pts.append(backproject(dimg, cam, fx, fy, cx, cy)[mask])
        off.append(off[-1] + int(mask.sum()))
    return np.concatenate(pts).reshape(-1, 3), np.asarray(off, np.int64)


# ---- the scenes and checks shared by tests/test_emu_depth_camera.py and tests/test_depth_camera_gpu.py ---------------------------
def experiment_camera():
    """The experiment's camera (optim_pointcloud.py:408-415): at (10, 14.1, 10), looking at the origin; camera to world."""
    g = np.pi / 4
    Ry = np.array([[np.cos(g), 0, np.sin(g), 0], [0, 1, 0, 0], [-np.sin(g), 0, np.cos(g), 0], [0, 0, 0, 1.0]])
    Rx = np.array([[1, 0, 0, 0], [0, np.cos(-g), -np.sin(-g), 0], [0, np.sin(-g), np.cos(-g), 0], [0, 0, 0, 1.0]])
    T = np.eye(4); T[2, 3] = 20.0
    return Ry @ Rx @ T


SMALL = dict(fx=64.375, fy=64.375, cx=39.5, cy=29.5, W=80, H=60)      # the experiment's 640 x 480, fx = fy = 515, at 1/8 size
FULL = dict(fx=515.0, fy=515.0, cx=319.5, cy=239.5, W=640, H=480)
FLOOR = ([1.0, 0, 0, 0, 0.0, -0.5, 0.0], BOX, [20.0, 1.0, 20.0, 0.0])
WALL = ([1.0, 0, 0, 0, 5.0, 5.0, 0.0], BOX, [1.0, 10.0, 10.0, 0.0])
OBJECTS = [(SPHERE, [1.0, 0, 0, 0]), (ROUNDED, [2.0, 2.0, 2.0, 0.2]), (CYLINDER, [0.4, 1.2, 0, 0]), (BOX, [1.5, 1.0, 0.7, 0])]
HIDDEN = ([1.0, 0, 0, 0, 3.5, 6.17, -0.4], SPHERE, [0.5, 0, 0, 0])      # behind the wall on the camera's line through (5, 8, 2)


def bounce_views(seed=3):
    """Floor, wall and one object per view, the object at a seeded random pose beside the wall as the camera sees it (a sphere, a rounded cube, a
    small cylinder, a tilted box), and a fifth view whose object the wall hides.  -> pose [5,3,7], shape_type [5,3], prm [5,3,4]"""
    r = np.random.default_rng(seed)
    pose, kind, prm = [], [], []
    for k, p in OBJECTS:
        q = r.standard_normal(4)
        obj = (np.concatenate([q / np.linalg.norm(q), r.uniform([0.0, 2.0, 3.5], [3.0, 6.0, 7.0])]), k, p)
        rows = (FLOOR, WALL, obj)
        pose.append([b[0] for b in rows]); kind.append([b[1] for b in rows]); prm.append([b[2] for b in rows])
    rows = (FLOOR, WALL, HIDDEN)
    pose.append([b[0] for b in rows]); kind.append([b[1] for b in rows]); prm.append([b[2] for b in rows])
    return np.array(pose, np.float64), np.array(kind, np.int32), np.array(prm, np.float64)


def check_view(depth, seg, ref, pose, shape_type, prm, cam, fx, fy, cx, cy, W=None, H=None, name=""):
    """The issue's checks of one rendered view against render()'s result `ref`; prints the counts before it asserts."""
    npx = depth.size
    ok = ~ref["delicate"]
    ndel, ncap = int(ref["delicate"].sum()), int((seg == -2).sum())
    firm = ok & (ref["seg"] >= 0) & (ref["cos"] >= COS_MIN)
    derr = np.abs(depth - ref["depth"])[firm].max() if firm.any() else 0.0
    wrong = int((seg != ref["seg"])[ok].sum())
    world = backproject(depth, cam, fx, fy, cx, cy)
    phi = 0.0
    for j in range(len(shape_type)):
        m = seg == j
        if m.any():
            pb = (world[m] - pose[j][4:]) @ quat_to_mat(pose[j][:4])
            phi = max(phi, np.abs(sdf(int(shape_type[j]), prm[j], pb)).max())
    print("%s: %d pixels, %d delicate, %d capped, %d hit, class errors %d, depth err %.2e, surface |phi| %.2e" %
          (name, npx, ndel, ncap, int((seg >= 0).sum()), wrong, derr, phi))
    assert ndel <= 0.01 * npx, "more than 1 % delicate pixels: choose another seed"
    assert ncap == 0, "pixels that used up the iteration cap"
    assert wrong == 0, "hit / miss / body differs from the oracle outside the delicate pixels"
    assert derr <= 1e-8, derr
    assert phi <= 1e-9, phi
    assert np.all(depth[seg < 0] == 0.0)
