"""The checks of dss_shade_render that tests/test_emu_shade.py (through the emulator) and tests/test_shade_gpu.py (on the device) both
run, against the oracle of tests/shade_ref.py.  A test module supplies `call` and `render` (shade_ref's backend) and wraps these
functions; the oracle's views are computed once per process and shared (ORACLE below), and never changed.

Tolerances (outside the oracle's delicate pixels, at most 1 % of a view; all stated by the oracle's errors, not by the kernel's):
normals of analytic bodies 1e-7 (central differences with h = 1e-5 err by h^2 |phi'''| <= 1e-10 at radii >= 0.2, round at 3e-10 at
magnitude 30, and the hit lies within 2e-9 of the surface), of grid bodies 1e-9 (both sides evaluate one closed form), unit length
1e-12, shade 1e-7 (which pins the visibility: a light's term is I c >= 2.5e-7 outside the delicate pixels), colour within one level,
the background exact, no flag."""
import numpy as np

import depth_camera_ref as ref
import grid_ref as G
import shade_ref as S

_CACHE = {}


def _views(render):
    """The five views of bounce_views(seed=3) at 80 x 60: the device's depth / seg and the depth oracle's delicate masks."""
    if "views" not in _CACHE:
        pose, kind, prm = ref.bounce_views(3)
        cam = ref.experiment_camera()
        depth, seg = render(pose, kind, prm, None, None, cam, **ref.SMALL)
        deli = [ref.render(pose[v], kind[v], prm[v], cam, **ref.SMALL)["delicate"] for v in range(5)]
        _CACHE["views"] = (pose, kind, prm, cam, depth, seg, deli)
    return _CACHE["views"]


def _want(render, v, lights, tag):
    key = ("want", v, tag)
    if key not in _CACHE:
        pose, kind, prm, cam, depth, seg, deli = _views(render)
        _CACHE[key] = S.shade_view(depth[v], seg[v], pose[v], kind[v], prm[v], None, None, cam, color=S.COLORS[:3], lights=lights,
                                   ambient=S.AMBIENT, background=S.BACKGROUND, depth_delicate=deli[v], **ref.SMALL)
    return _CACHE[key]


def _got(call, render, lights, tag, **kw):
    key = ("got", tag)
    if key not in _CACHE:
        pose, kind, prm, cam, depth, seg, deli = _views(render)
        _CACHE[key] = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg, lights=lights, **kw))
    return _CACHE[key]


def view_matches_the_oracle(call, render, v):
    got, want = _got(call, render, S.LIGHT, "one"), _want(render, v, S.LIGHT, "one")
    S.check_view({k: a[v] for k, a in got.items()}, want, _views(render)[1][v], "view %d" % v)


def views_are_not_vacuous(call, render):
    """From the oracle alone: floor pixels in the object's and in the wall's shadow, object pixels facing away from the light."""
    wants = [_want(render, v, S.LIGHT, "one") for v in range(4)]
    obj = [int(((w["seg"] == 0) & ~w["delicate"] & (w["dark"][0, 2] < 0)).sum()) for w in wants]
    wall = [int(((w["seg"] == 0) & ~w["delicate"] & (w["dark"][0, 1] < 0)).sum()) for w in wants]
    away = [int(((w["seg"] == 2) & ~w["delicate"] & (w["c"][0] <= 0)).sum()) for w in wants]
    lit = [int(((w["seg"] == 2) & ~w["delicate"] & (w["c"][0] > 0) & (w["V"][0] > 0)).sum()) for w in wants]
    print("floor pixels in the object's shadow %s, in the wall's %s; object pixels facing away %s, lit %s" % (obj, wall, away, lit))
    assert max(obj) > 10 and max(wall) > 10 and sum(away) > 10 and max(lit) > 10


def four_lights_match_the_oracle(call, render):
    got = _got(call, render, S.FOUR_LIGHTS, "four")
    for v in (0, 3):
        S.check_view({k: a[v] for k, a in got.items()}, _want(render, v, S.FOUR_LIGHTS, "four"), _views(render)[1][v], "view %d, 4 lights" % v)


def two_calls_return_the_same_bits(call, render):
    pose, kind, prm, cam, depth, seg, deli = _views(render)
    a = _got(call, render, S.LIGHT, "one")
    b = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg))
    assert all(np.array_equal(a[k], b[k]) for k in S.FILL)


def switches(call, render):
    pose, kind, prm, cam, depth, seg, deli = _views(render)
    hit = seg >= 0
    # shadows = 0: the unshadowed shade
    off = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg, shadows=0))
    for v in (0, 2):
        w = _want(render, v, S.LIGHT, "one")
        plain = np.where(w["hit"], np.minimum(1.0, S.AMBIENT + S.LIGHT[0][3] * np.maximum(w["c"][0], 0.0)), 0.0)
        assert np.abs(off["shade"][v] - plain)[~w["delicate"]].max() <= 1e-7
    on = _got(call, render, S.LIGHT, "one")
    assert (off["shade"] > on["shade"] + 0.01).sum() > 10 and not (off["shade"] < on["shade"]).any()
    # nlight = 0: ambient wherever something is hit
    none = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg, lights=[]))
    assert np.all(none["shade"][hit] == S.AMBIENT) and np.all(none["shade"][~hit] == 0.0) and np.array_equal(none["normal"], on["normal"])


def a_convex_body_does_not_shadow_itself(call, render):
    pose = np.array([[ref.FLOOR[0], [1.0, 0, 0, 0, 1.0, 2.0, 5.0]]], np.float64)
    kind, prm = np.array([[ref.BOX, ref.SPHERE]], np.int32), np.array([[ref.FLOOR[2], [1.0, 0, 0, 0]]], np.float64)
    cam = ref.experiment_camera()
    depth, seg = render(pose, kind, prm, None, None, cam, **ref.SMALL)
    got = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg))
    want = S.shade_view(depth[0], seg[0], pose[0], kind[0], prm[0], None, None, cam, color=S.COLORS[:2], lights=S.LIGHT, ambient=S.AMBIENT,
                        background=S.BACKGROUND, **ref.SMALL)
    m, V = S.visibility(got["shade"][0], want, S.LIGHT, S.AMBIENT)
    ball = m & (seg[0] == 1)
    print("lit pixels of the sphere: %d, least V %.9f" % (int(ball.sum()), V[ball].min()))
    assert ball.sum() > 30 and np.abs(V[ball] - 1.0).max() <= 1e-6
    assert ((seg[0] == 0) & m & (V < 0.5)).sum() > 10      # (and the sphere's shadow lies on the floor)


def grid_self_shadow(call, render, shape):
    pose, kind, prm, grids, gid = S.torus_scene(shape)
    cam = ref.experiment_camera()
    key = ("torus", shape)
    if key not in _CACHE:
        depth, seg = render(pose, kind, prm, grids, gid, cam, **ref.SMALL)
        deli = G.render(pose[0], kind[0], prm[0], grids, gid[0], cam, **ref.SMALL)["delicate"]
        want = S.shade_view(depth[0], seg[0], pose[0], kind[0], prm[0], grids, gid[0], cam, color=S.COLORS[:2], lights=S.TORUS_LIGHT,
                            ambient=S.AMBIENT, background=S.BACKGROUND, depth_delicate=deli, **ref.SMALL)
        _CACHE[key] = (depth, seg, want)
    depth, seg, want = _CACHE[key]
    got = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg, grids=grids, gid=gid, lights=S.TORUS_LIGHT))
    own = (want["seg"] == 1) & ~want["delicate"] & (want["c"][0] > 0) & (want["dark"][0, 1] < 0)
    print("torus %s: %d pixels, %d lit side in its own shadow" % (shape, int((seg[0] == 1).sum()), int(own.sum())))
    assert own.sum() > 10
    S.check_view({k: a[0] for k, a in got.items()}, want, kind[0], "torus %s" % (shape,))
    m, V = S.visibility(got["shade"][0], want, S.TORUS_LIGHT, S.AMBIENT)
    assert np.abs(V - want["V"][0])[m].max() <= 1e-6


def _boundary_scene(nview, nbody):
    if nbody == 8:
        pose, kind, prm = S.eight_bodies()
        return np.repeat(pose, nview, 0), np.repeat(kind, nview, 0), np.repeat(prm, nview, 0)
    pose, kind, prm = ref.bounce_views(3)
    return pose[:nview, 3 - nbody:], kind[:nview, 3 - nbody:], prm[:nview, 3 - nbody:]      # (nbody = 1: the object alone)


BOUNDARIES = [(67, 5, 5, 3, 4), (16, 16, 1, 1, 1), (80, 60, 1, 8, 1), (67, 5, 1, 8, 4), (16, 16, 5, 3, 1)]      # W, H, nview, nbody, nlight


def launch_boundary(call, render, W, H, nview, nbody, nlight):
    """Every view against the oracle, the guard view (S.run), and a seg image with -2, nbody and 1000 in it."""
    pose, kind, prm = _boundary_scene(nview, nbody)
    cam = ref.experiment_camera()
    f = dict(fx=64.375, fy=64.375, cx=(W - 1) / 2, cy=(H - 1) / 2, W=W, H=H)
    if nbody == 1:      # the object alone: the principal point moved so that the image's centre looks at it
        pc = cam[:3, :3].T @ (pose[0, 0, 4:] - cam[:3, 3])
        f.update(cx=W / 2 - f["fx"] * pc[0] / -pc[2], cy=H / 2 - f["fy"] * pc[1] / pc[2])
    lights = S.FOUR_LIGHTS[:nlight]
    depth, seg = render(pose, kind, prm, None, None, cam, **f)
    got = S.run(call, S.arguments(pose, kind, prm, cam, depth, seg, lights=lights, **f))
    assert (seg >= 0).sum() > 10
    for v in range(nview if nbody < 8 else 1):
        deli = ref.render(pose[v], kind[v], prm[v], cam, **f)["delicate"]
        want = S.shade_view(depth[v], seg[v], pose[v], kind[v], prm[v], None, None, cam, color=S.COLORS[:nbody], lights=lights,
                            ambient=S.AMBIENT, background=S.BACKGROUND, depth_delicate=deli, **f)
        # (cap=False: a strip of 67 x 5 pixels may run along an edge; the 1 % cap on delicate pixels is asserted on the 80 x 60 views)
        S.check_view({k: a[v] for k, a in got.items()}, want, kind[v], "%d x %d view %d, %d bodies, %d lights" % (W, H, v, nbody, nlight),
                     cap=W * H >= 4800)
    bad = seg.copy()
    at = [(0, 0, 0), (nview - 1, H - 1, W - 1), (0, H // 2, W // 2)]
    for (v, r, c), val in zip(at, (-2, nbody, 1000)):
        bad[v, r, c] = val
    other = S.run(call, S.arguments(pose, kind, prm, cam, depth, bad, lights=lights, **f))
    mask = np.zeros(seg.shape, bool)
    for a in at:
        mask[a] = True
    bg = np.floor(255.0 * np.asarray(S.BACKGROUND) + 0.5).astype(np.uint8)
    assert np.all(other["rgb"][mask] == bg) and np.all(other["normal"][mask] == 0.0) and np.all(other["shade"][mask] == 0.0) and not other["flags"][mask].any()
    assert all(np.array_equal(other[k][~mask], got[k][~mask]) for k in S.FILL)


def statuses(call, render):
    """Each refusal of shade_camera.h, the outputs still at their fill."""
    pose, kind, prm, cam, depth, seg, deli = _views(render)
    base = lambda **kw: S.arguments(pose[:2], kind[:2], prm[:2], cam, depth[:2], seg[:2], **kw)

    def refused(A, what):
        rc = call(A)
        assert rc != 0 and S.untouched(A), what
        return rc

    codes = {}
    for name in ("pose", "shape_type", "prm", "cam", "depth", "seg", "color", "light", "background", "normal", "shade", "rgb", "flags"):
        A = base()
        keep = A[name]
        A[name] = None
        codes[name] = refused(A, "null " + name)
        A[name] = keep
    for name, val in (("nview", 0), ("nbody", 0), ("W", 0), ("H", -1), ("nlight", -1), ("nlight", 5), ("shadow_bias", 0.0), ("shadow_bias", -1e-3),
                      ("ngrid", -1)):
        A = base()
        A[name] = val
        codes[(name, val)] = refused(A, "%s = %r" % (name, val))
    assert set(codes.values()) == {-1}, codes      # DSS_E_BADARG
    un = {}
    for ty in (4, 5, 6, 7):      # brick, bowl, and a neural and a grid body without a grid (ngrid = 0)
        k2 = kind[:2].copy(); k2[1, 2] = ty
        A = S.arguments(pose[:2], k2, prm[:2], cam, depth[:2], seg[:2])
        un[ty] = refused(A, "type %d" % ty)
    grids = [G.sphere_grid()]
    for ty in (6, 7):      # the same beside a table of grids, with grid_id = -1
        k2 = kind[:2].copy(); k2[1, 2] = ty
        A = S.arguments(pose[:2], k2, prm[:2], cam, depth[:2], seg[:2], grids=grids, gid=np.full((2, 3), -1))
        un[(ty, -1)] = refused(A, "type %d, grid_id -1" % ty)
    nine = S.arguments(np.repeat(pose[:1, :1], 9, 1), np.repeat(kind[:1, :1], 9, 1), np.repeat(prm[:1, :1], 9, 1), cam, depth[:1], seg[:1],
                       colors=np.ones((9, 3)))
    un["nine bodies"] = refused(nine, "nbody = 9")
    big = base()
    big.update(nview=1, W=65536, H=32768)      # 2^31 pixels: refused before anything is read
    un["2^31 pixels"] = refused(big, "too many pixels")
    assert set(un.values()) == {-3}, un      # DSS_E_UNSUPPORTED
