"""Contact-detection capacities at, below and above the exact need: the scenes, the measurement of the need and the
assertions, stated once on numpy arrays.  test_emu_capacity.py runs them on the CPU emulation of the kernels,
test_capacity_gpu.py on the device through the product backend.

The narrow phase writes into fixed-size buffers, each behind a clamp `slot < capacity` and a sticky bit of DssWorld.overflow
(1 max_cand, 2 the 1024 movers / contacts of one normal cluster, 4 max_pc, 8 maxc, 32 the neural lists).  The buffers are
packed ([B][npair][max_pc], [B][10][maxc], [slot][28][max_cand]), so a clamp that is off by one either drops a contact or
writes into the next pair's, field's or scene's row.  Every case therefore runs a batch of three scenes with distinct needs,
the neediest in the middle, on a backend whose arrays end in a sentinel guard (`guarded`), and compares every output with an
ample run of the same batch with `==`: scene 2 is where an overrun of scene 1 lands, scene 0 shows nothing went backwards.
"""
import ctypes
import functools
import re

import numpy as np

from diffsdfsim_amd import meshes, scenes
from diffsdfsim_amd import world_abi as abi
from diffsdfsim_amd.engine import BatchEngine

SENTINEL = 0xA5
BITS = {"max_cand": 1, "hcap": 2, "max_pc": 4, "maxc": 8, "igr_qcap": 32}
AMPLE = dict(max_cand=4096, max_pc=2048, maxc=96)      # (maxc: the contact LCP keeps its columns in LDS)


# ---- 1. the guarded backend ----------------------------------------------------------------------------------------------
def guard_elems(shape):
    """THE RULE for the length of the guard behind an array of `shape`, in elements: one entry of the leading axis (the next
    scene's / slot's whole block), and never less than DSS_CAND_FIELDS rows of the last axis -- the largest group of rows a
    kernel addresses from one base pointer is a candidate slot, DSS_CAND_FIELDS x max_cand; the per-pair and per-scene
    contact rows are 10 x max_pc and 10 x maxc.  A one-dimensional array gets 64 elements."""
    if len(shape) < 2:
        return 64
    return max(int(np.prod(shape[1:])), abi.CAND_FIELDS * int(shape[-1]))


class _CountingLib:
    """The backend's library with the detections counted: `calls` is the index of the last attempt (construction's
    dss_find_contacts is attempt 0, the k-th dss_step_attempt attempt k)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, -1

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("dss_find_contacts", "dss_step_attempt"):
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


class Guarded:
    """A TorchBackend or emu.EmuBackend whose zeros() returns the leading view of a longer flat buffer; the tail is filled
    with a sentinel and checked by assert_guards_intact(): an overrun lands in memory the test owns and is reported as an
    assertion."""

    def __init__(self, inner):
        self.inner, self.lib, self.registry = inner, _CountingLib(inner.lib), []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    @staticmethod
    def _bytes(flat):
        if hasattr(flat, "data_ptr"):
            import torch
            return flat.view(torch.uint8)
        return flat.view(np.uint8)

    def zeros(self, shape, dtype):
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape))
        flat = self.inner.zeros((n + guard_elems(shape),), dtype)
        raw = self._bytes(flat)
        raw[n * (len(raw) // len(flat)):] = SENTINEL
        view = flat[:n].reshape(shape)
        self.registry.append([None, flat, view, n, shape])
        return view

    def name_arrays(self, E):
        """Names for the messages: an engine array is the very view zeros() returned."""
        by_id = {id(r[2]): r for r in self.registry}
        for group in (E.arr, getattr(E, "adj", None) or {}, {"lcp_ws": getattr(E, "lcp_ws", None)}):
            for name, a in group.items():
                if id(a) in by_id:
                    by_id[id(a)][0] = name

    def assert_guards_intact(self):
        for k, (name, flat, _view, n, shape) in enumerate(self.registry):
            raw = self._bytes(flat)
            tail = self.inner.to_numpy(raw[n * (len(raw) // len(flat)):])
            bad = np.nonzero(tail != SENTINEL)[0]
            assert bad.size == 0, "guard behind %s %s overwritten: %d bytes, the first %d bytes past the end" % (
                name or "array #%d" % k, shape, bad.size, int(bad[0]))


def guarded(backend):
    return Guarded(backend)


def build_engine(spec, be, **kw):
    """BatchEngine(spec, backend=be, **kw) that hands the engine back even where construction raises the capacity error
    (its arrays are bound before the first detection): -> (engine, error or None)."""
    E = BatchEngine.__new__(BatchEngine)
    err = None
    try:
        E.__init__(spec, backend=be, **kw)
    except RuntimeError as e:
        err = e
    be.name_arrays(E)
    return E, err


# ---- 2. scenes with a dialled need ---------------------------------------------------------------------------------------
PLATE_DIMS = (1.0, 0.05, 1.0)
FLOOR_DIMS = (2.0, 1.0, 2.0)
GAP = 5e-4      # < eps = 1e-3: in contact, not penetrating
KW = dict(dt=1.0 / 30, eps=1e-3, tol=1e-8, fric_dirs=8)


def plate_mesh(N, ntop=2):
    """A box of PLATE_DIMS whose bottom face is a fan of exactly N coplanar triangles (rim point i, rim point i + 1, centre;
    the rim points are the four corners and N - 4 points on the edges, at most one apart in count from edge to edge) and
    whose top face is a fan of `ntop` triangles (2: the two triangles of a plain face); the four sides are two triangles
    each.  -> verts, faces, the indices of the bottom faces whose first vertex is a corner."""
    assert N >= 4 and (ntop == 2 or ntop >= 4)
    hx, hy, hz = (0.5 * d for d in PLATE_DIMS)
    corners = np.array([[-hx, -hz], [hx, -hz], [hx, hz], [-hx, hz]])

    def rim(n):
        per = [(n - 4) // 4 + (1 if e < (n - 4) % 4 else 0) for e in range(4)]
        pts, is_corner = [], []
        for e in range(4):
            a, b = corners[e], corners[(e + 1) % 4]
            for k in range(per[e] + 1):
                # one coordinate of an edge is the corner's own, bit for bit: the rim points are exactly collinear
                pts.append(a + (b - a) * (k / (per[e] + 1.0)))
                is_corner.append(k == 0)
        return np.array(pts), np.array(is_corner)

    V, F = [], []
    # sides and (ntop == 2) top from the eight corners
    c8 = np.array([[x, y, z] for y in (-hy, hy) for (x, z) in corners])      # 0-3 bottom ring, 4-7 top ring
    V.append(c8)
    for e in range(4):
        a, b = e, (e + 1) % 4
        F += [[a, b, b + 4], [a, b + 4, a + 4]]
    nv = 8
    if ntop == 2:
        F += [[4, 6, 5], [4, 7, 6]]
    else:
        r, _ = rim(ntop)
        V.append(np.column_stack([r[:, 0], np.full(ntop, hy), r[:, 1]])); V.append(np.array([[0.0, hy, 0.0]]))
        F += [[nv + (i + 1) % ntop, nv + i, nv + ntop] for i in range(ntop)]
        nv += ntop + 1
    first_bottom = len(F)
    r, is_corner = rim(N)
    V.append(np.column_stack([r[:, 0], np.full(N, -hy), r[:, 1]])); V.append(np.array([[0.0, -hy, 0.0]]))
    F += [[nv + i, nv + (i + 1) % N, nv + N] for i in range(N)]
    return np.concatenate(V), np.array(F, np.int64), first_bottom + np.nonzero(is_corner)[0]


def _floor(spec, dims, pitch):
    v, f, _tie = meshes.box_mesh(np.array(dims), max_tri_length=pitch)
    spec["meshes"].append((v, f)); spec["mesh_vgrad"].append(np.zeros_like(v))
    spec["pose"][:, 0, 4:] = (0.0, -dims[1] / 2, 0.0)
    spec["shape_prm"][:, 0] = dims
    spec["inertia"][:, 0] = scenes.box_inertia(1.0, dims)
    spec["fric"][:, 0] = 0.5


def plate_batch(Ns, ntop=2, full=None):
    """One scene per entry of Ns: plate(N) resting GAP above a pinned floor box (2 x 1 x 2, 4 x 4 cells a face).  Every
    bottom face of the plate is a candidate and a contact of one normal cluster.  mesh_vgrad is given, as zeros."""
    B = len(Ns)
    spec = scenes._base(B, 2)
    _floor(spec, FLOOR_DIMS, 0.5)
    for s, N in enumerate(Ns):
        v, f, _c = plate_mesh(N, ntop)
        spec["meshes"].append((v, f)); spec["mesh_vgrad"].append(np.zeros_like(v))
        spec["mesh_id"][s, 1] = s + 1
        spec["pose"][s, 1, 4:] = (0.0, GAP + PLATE_DIMS[1] / 2, 0.0)
        spec["shape_prm"][s, 1] = PLATE_DIMS
        spec["inertia"][s, 1] = scenes.box_inertia(1.0, PLATE_DIMS)
        spec["fric"][s, 1] = 0.5
        spec["fext"][s, 1, 4] = -10.0
    if full is not None:
        spec["full_kernels"] = full
    return spec


STACK_DIMS = ((0.2, 0.2, 0.2), (0.3, 0.3, 0.3), (0.3, 0.25, 0.2))


def little_stack():
    """Three scenes in the initial pose of scenes.box_stack(3, nbox=2) with small boxes (grid pitch 0.1) on a 1 x 1 x 1 floor
    of 1200 faces.  Scene 1 is the stack with side 0.3 (3 x 3 cells = 18 triangles a face), the upper box yawed; scene 0 stacks
    boxes of side 0.2, scene 2 boxes of 0.3 x 0.25 x 0.2 (STACK_DIMS): three distinct needs in every limit, the largest in the
    middle (assert_dialled)."""
    spec = scenes._base(3, 3)
    _floor(spec, (1.0, 1.0, 1.0), 0.1)
    place = [((0.01, 0.0), (0.03, 0.02), 0.3), ((0.01, 0.0), (0.02, 0.01), 0.5), ((0.0, 0.0), (0.02, 0.01), 0.15)]
    for s, (o1, o2, yaw) in enumerate(place):
        d = np.array(STACK_DIMS[s])
        v, f, _tie = meshes.box_mesh(d)
        spec["meshes"].append((v, f)); spec["mesh_vgrad"].append(np.zeros_like(v))
        for k, off in ((1, o1), (2, o2)):
            y = GAP + d[1] / 2 + ((GAP + d[1]) if k == 2 else 0.0)
            spec["mesh_id"][s, k] = s + 1
            spec["pose"][s, k, :4] = scenes._quat_from_euler(0.0, yaw if k == 2 else 0.0, 0.0)
            spec["pose"][s, k, 4:] = (off[0], y, off[1])
            spec["shape_prm"][s, k] = d
            spec["inertia"][s, k] = scenes.box_inertia(1.0, d)
            spec["fric"][s, k] = 0.5
            spec["fext"][s, k, 4] = -10.0
    return spec


# ---- 3. measuring the need -----------------------------------------------------------------------------------------------
OUT = ("overflow", "nc", "c_body", "c_face", "c_abc", "c_geom", "n_nc", "n_body", "n_face", "n_abc", "n_geom",
       "pc_count", "pc_stats", "pc_face", "pc_abc", "pc_geom", "pose", "vel", "t", "nsub", "lam", "slack", "n_active", "n_pairs")


def snapshot(E):
    return {k: np.array(E.get(k), copy=True) for k in OUT}


def measure_need(spec, nsteps, make_backend, **kw):
    """The batch on generous capacities, one attempt at a time as BatchEngine._attempt_until_idle drives it; construction's
    detection is attempt 0.  -> (need, snaps): need[k] the per-scene maximum over all attempts of the candidate count
    pc_stats[..., 1] ('max_cand'), |pc_count| ('max_pc') and nc, n_nc ('maxc'); snaps[i] every output array after attempt i."""
    cap = dict(AMPLE); cap.update(kw)
    be = guarded(make_backend())
    E, err = build_engine(spec, be, **cap)
    assert err is None, err
    snaps = [snapshot(E)]
    L, W = be.lib, E.W
    for _ in range(nsteps):
        W.step_mask = None
        E._check(L.dss_step_begin(ctypes.byref(W), be.stream()), "dss_step_begin")
        n, k = E.B, 0
        while n > 0:
            E._check(L.dss_step_attempt(ctypes.byref(W), be.ptr(E.lcp_ws), E.lcp_ws_bytes, be.stream()), "dss_step_attempt")
            n = be.read_int(E.arr["n_active"])
            snaps.append(snapshot(E))
            assert not n & abi.N_ACTIVE_OVERFLOW, "the ample run overflowed: %s" % snaps[-1]["overflow"]
            E._update_igr_hint(k == 0, n == 0)
            k += 1
            assert k < 4096
    be.assert_guards_intact()
    assert all((s["overflow"] == 0).all() for s in snaps)
    need = dict(max_cand=np.max([s["pc_stats"][..., 1].max(axis=1) for s in snaps], axis=0),
                max_pc=np.max([np.abs(s["pc_count"]).max(axis=1) for s in snaps], axis=0),
                maxc=np.max([np.maximum(s["nc"], s["n_nc"]) for s in snaps], axis=0))
    return need, snaps


# ---- 4. the assertions ---------------------------------------------------------------------------------------------------
def _scene_equal(a, b, s, what, skip=()):
    """Scene s of two snapshots, bit for bit on the used columns (the arrays' widths differ with the capacities)."""
    for pre, cnt in (("c", "nc"), ("n", "n_nc")):
        n = int(a[cnt][s])
        assert n == int(b[cnt][s]), (what, s, cnt, n, int(b[cnt][s]))
        for k in ("body", "abc", "geom"):
            assert np.array_equal(a["%s_%s" % (pre, k)][s][:, :n], b["%s_%s" % (pre, k)][s][:, :n], equal_nan=True), (what, s, pre + "_" + k)
        assert np.array_equal(a[pre + "_face"][s][:n], b[pre + "_face"][s][:n]), (what, s, pre + "_face")
    for k in ("pc_count", "pc_stats", "pose", "vel", "t", "nsub", "overflow"):
        if k not in skip:
            assert np.array_equal(a[k][s], b[k][s]), (what, s, k, a[k][s], b[k][s])
    for p, c in enumerate(np.abs(a["pc_count"][s])):
        assert np.array_equal(a["pc_face"][s, p, :c], b["pc_face"][s, p, :c]), (what, s, p, "pc_face")
        assert np.array_equal(a["pc_abc"][s, p, :, :c], b["pc_abc"][s, p, :, :c]), (what, s, p, "pc_abc")
        assert np.array_equal(a["pc_geom"][s, p, :, :c], b["pc_geom"][s, p, :, :c]), (what, s, p, "pc_geom")
    w = min(a["lam"].shape[2], b["lam"].shape[2])
    for k in ("lam", "slack"):
        assert np.array_equal(a[k][s][:, :w], b[k][s][:, :w], equal_nan=True), (what, s, k)


def run_enough(spec, nsteps, make_backend, snaps, **cap):
    """Capacities that suffice: no flag anywhere, and after construction and after every step every output equals the ample
    run's with ==; guards intact."""
    be = guarded(make_backend())
    E, err = build_engine(spec, be, **cap)
    assert err is None, err
    for s in range(E.B):
        _scene_equal(snapshot(E), snaps[0], s, "construction")
    for _ in range(nsteps):
        E.step()
    assert be.lib.calls == len(snaps) - 1, (be.lib.calls, len(snaps))
    now = snapshot(E)
    assert (now["overflow"] == 0).all(), now["overflow"]
    for s in range(E.B):
        _scene_equal(now, snaps[-1], s, "after %d steps" % nsteps)
    be.assert_guards_intact()
    return E


def limit_named(err):
    m = re.search(r"in scene (\d+) \((.*)\): raise the limit", str(err))
    assert m, str(err)
    return int(m.group(1)), m.group(2)


def run_short(spec, nsteps, make_backend, snaps, limit, flagged, caps, name=None):
    """One short of the need in `limit`: construction or a step raises RuntimeError naming exactly that limit; the overflow
    word holds exactly its bit in the scenes of `flagged` and 0 elsewhere; n_active carries the overflow mark after an attempt;
    the clamped counts obey the capacities; what is present of the flagged scenes' lists is the head of the ample run's lists
    at the same attempt, in order; the other scenes equal the ample run bit for bit; guards intact."""
    be = guarded(make_backend())
    E, err = build_engine(spec, be, **caps)
    for _ in range(nsteps):
        if err is not None:
            break
        try:
            E.step()
        except RuntimeError as e:
            err = e
    be.assert_guards_intact()
    assert err is not None, "no capacity error with %s one short of the need" % limit
    scene, names = limit_named(err)
    assert names == (name or limit), str(err)
    at = be.lib.calls
    now, ref = snapshot(E), snaps[at]
    bit = BITS[limit]
    want = np.array([bit if s in flagged else 0 for s in range(E.B)])
    assert np.array_equal(now["overflow"], want), (now["overflow"], want)
    assert scene == min(flagged)
    if at > 0:
        assert int(now["n_active"][0]) & abi.N_ACTIVE_OVERFLOW
    assert (now["pc_stats"][..., 1] <= caps["max_cand"]).all() and (np.abs(now["pc_count"]) <= caps["max_pc"]).all()
    assert (now["nc"] <= caps["maxc"]).all() and (now["n_nc"] <= caps["maxc"]).all()
    for s in range(E.B):
        if s not in flagged:
            _scene_equal(now, ref, s, "unflagged scene at attempt %d" % at)
            continue
        pre, cnt = ("c", "nc") if at == 0 else ("n", "n_nc")
        if limit in ("max_pc", "hcap"):
            cut = 0
            for p, (c, cr) in enumerate(zip(now["pc_count"][s], ref["pc_count"][s])):
                assert abs(c) == min(abs(cr), caps["max_pc"]) if limit == "max_pc" else abs(c) <= abs(cr), (s, p, c, cr)
                cut += abs(c) < abs(cr)
                c = abs(c)
                if limit == "max_pc":       # (a truncated cluster keeps the hull of its first 1024 points: another set)
                    assert np.array_equal(now["pc_face"][s, p, :c], ref["pc_face"][s, p, :c]), (s, p)
                    assert np.array_equal(now["pc_abc"][s, p, :, :c], ref["pc_abc"][s, p, :, :c]), (s, p)
                    assert np.array_equal(now["pc_geom"][s, p, :, :c], ref["pc_geom"][s, p, :, :c]), (s, p)
            assert cut >= 1 or limit == "hcap"
        if limit == "maxc":
            n = int(now[cnt][s])
            assert n == caps["maxc"] == int(ref[cnt][s]) - 1, (n, caps["maxc"], int(ref[cnt][s]))
            for k in ("body", "abc", "geom"):
                assert np.array_equal(now["%s_%s" % (pre, k)][s][:, :n], ref["%s_%s" % (pre, k)][s][:, :n]), (s, k)
            assert np.array_equal(now[pre + "_face"][s][:n], ref[pre + "_face"][s][:n])
            assert np.array_equal(now["pc_count"][s], ref["pc_count"][s])
    return E, now, ref


def caps_for(need, limit, delta):
    """Ample capacities with `limit` at the batch's largest need + delta -> (caps, the scenes whose own need that is)."""
    k = int(need[limit].max())
    caps = dict(AMPLE); caps[limit] = k + delta
    return caps, [s for s in range(len(need[limit])) if int(need[limit][s]) == k]


def assert_dialled(need, limit):
    """Distinct needs, the largest in the middle scene."""
    n = [int(x) for x in need[limit]]
    assert len(set(n)) == len(n) and n[1] == max(n), (limit, n)


@functools.lru_cache(None)
def oracle_contacts(key):
    """The initial contact set of scene s of a named batch from the whole-step CPU oracle: (body [n, 2], geom [n, 10])."""
    from oracle import step_oracle as SO
    name, s = key
    spec = hcap_batch(name[1], True) if isinstance(name, tuple) else SPECS[name]()     # ("hcap", M): the HCAP plates
    W = SO.World(spec, s, hull="scipy", **KW)
    body, geom, _st, _lap = W.contacts()
    W.close()
    return body, geom


def check_against_oracle(name, snap0, tol=1e-9):
    """The ample run's initial contacts against oracle/step_oracle, per ordered pair as sets (rollout_helpers.check_contacts'
    comparison on arrays)."""
    for s in range(len(snap0["nc"])):
        body_ref, geom_ref = oracle_contacts((name, s))
        nc = int(snap0["nc"][s])
        body, geom = snap0["c_body"][s][:, :nc].T, snap0["c_geom"][s][:, :nc].T
        assert [tuple(r) for r in body] == [tuple(r) for r in body_ref], (name, s, nc, len(body_ref))
        for pair in sorted(set(map(tuple, body))):
            a, b = geom[(body == pair).all(axis=1)], geom_ref[(body_ref == pair).all(axis=1)]
            ia = np.lexsort(np.round(a[:, 3:6], 6).T[::-1]); ib = np.lexsort(np.round(b[:, 3:6], 6).T[::-1])
            assert np.abs(a[ia] - b[ib]).max() < tol, (name, s, pair, np.abs(a[ia] - b[ib]).max())


PLATE_N = 40      # plate(35), plate(40), plate(31)
HCAP = 1024       # BlockGroup::HCAP (np_common.h)
HCAP_TOP = 1100   # top-face triangles of the HCAP plates: more than 2048 faces, so a batch of three starts the pair on a workgroup
HCAP_NAME = ("more than 1024 moving Frank-Wolfe candidates -- or, with the lean kernels (spec['full_kernels'] unset/False), "
             "contacts of one normal cluster, or more than 8192 contacts -- in a body pair")


def hcap_batch(M, full=None):
    """Plates whose normal cluster has M - 5, M, M - 9 contacts: the bottom fan and the eight side triangles, which touch
    the floor along their lower edge (the top fan is a candidate and no contact)."""
    return plate_batch((M - 8 - 5, M - 8, M - 8 - 9), ntop=HCAP_TOP, full=full)


# ---- more than 32 rounds of a workgroup (32 x 256 contacts) in clusters that each stay below HCAP ------------------------------
MASK_ROUNDS = 32 * 256      # contacts the lean variant's kept-contact mask holds for a workgroup (np_filter_emit.inc)
FANS_RA, FANS_RB, FANS_GAP, FANS_EPS = 1.0, 0.5, 1e-3, 5e-3


def fans_mesh(sizes, theta=0.04, delta=1e-4):
    """len(sizes) apex points on the lower cap of a sphere of radius FANS_RA, on a ring `theta` rad off its lowest point (so
    the sphere's normals at two of them are 2 sin(theta) sin(pi / n) > 1e-2 rad apart: one normal cluster per apex); apex j
    carries a fan of sizes[j] triangles (apex, w_k, w_k+1) of edge `delta` in the tangent plane, all opening away from the
    lowest point.  The apex is the vertex nearest the sphere underneath and the linear minimisation at it picks it again, so
    no candidate moves, every triangle is a contact, and the contact points of a fan coincide."""
    V, F = [], []
    n = len(sizes)
    for j, m in enumerate(sizes):
        phi = 2 * np.pi * j / n
        d = np.array([np.sin(theta) * np.cos(phi), -np.cos(theta), np.sin(theta) * np.sin(phi)])
        tr = np.array([np.cos(theta) * np.cos(phi), np.sin(theta), np.cos(theta) * np.sin(phi)])
        tp = np.array([-np.sin(phi), 0.0, np.cos(phi)])
        al = np.linspace(-1.0, 1.0, m + 1)
        base = sum(len(v) for v in V)
        V.append(np.concatenate([[FANS_RA * d], FANS_RA * d + delta * (np.cos(al)[:, None] * tr + np.sin(al)[:, None] * tp)]))
        F += [[base, base + 1 + k, base + 2 + k] for k in range(m)]
    return np.concatenate(V), np.array(F, np.int64)


def fans_batch(totals=(MASK_ROUNDS, MASK_ROUNDS + 1, MASK_ROUNDS - 92), nfan=9, full=None):
    """One scene per total: a sphere of radius FANS_RA whose mesh is fans_mesh with that many triangles in nine fans (each
    below HCAP = 1024), FANS_GAP above a pinned sphere of radius FANS_RB with a coarse icosphere mesh."""
    B = len(totals)
    spec = scenes._base(B, 2)
    v0, f0 = meshes.sphere_mesh(FANS_RB, subdivisions=1)
    spec["meshes"].append((v0, f0)); spec["mesh_vgrad"].append(np.zeros_like(v0))
    spec["shape_type"][:] = abi.SHAPE_SPHERE
    spec["shape_prm"][:, 0, 0] = FANS_RB
    spec["shape_prm"][:, 1, 0] = FANS_RA
    spec["pose"][:, 1, 4:] = (0.0, FANS_RB + FANS_GAP + FANS_RA, 0.0)
    for b, r in ((0, FANS_RB), (1, FANS_RA)):
        spec["inertia"][:, b] = 0.4 * r * r * np.eye(3)
    for s, tot in enumerate(totals):
        sizes = [tot // nfan + (1 if j < tot % nfan else 0) for j in range(nfan)]
        assert max(sizes) < HCAP
        v, f = fans_mesh(sizes)
        spec["meshes"].append((v, f)); spec["mesh_vgrad"].append(np.zeros_like(v))
        spec["mesh_id"][s, 1] = s + 1
    if full is not None:
        spec["full_kernels"] = full
    return spec


FANS_KW = dict(KW, eps=FANS_EPS)
FANS_CAPS = dict(max_cand=3 * 4096, max_pc=64, maxc=64)


def check_mask_rounds(make_backend):
    """np_filter_emit.inc:97-104, 124-131: the lean variant keeps the hull's verdict on a thread's contacts in a 32-bit mask,
    one bit per round of the group.  Scene 0 has exactly 32 x 256 contacts in nine clusters (the last round the mask holds:
    no flag, equal to the full variant with ==), scene 1 one more (bit 2 in that scene alone: the lean variant stops there
    instead of emitting a wrong set), scene 2 fewer."""
    key = ("fans", getattr(make_backend, "__name__", str(make_backend)))
    if key not in _NEED:
        _NEED[key] = measure_need(fans_batch(full=True), 0, make_backend, **dict(FANS_KW, **FANS_CAPS))
    need, snaps = _NEED[key]
    search_path(snaps, "workgroup")
    s0 = snaps[0]
    # every triangle is a candidate, one kept contact per fan
    assert s0["pc_stats"][:, 1, 1].tolist() == [MASK_ROUNDS, MASK_ROUNDS + 1, MASK_ROUNDS - 92], s0["pc_stats"][:, 1, 1]
    assert s0["pc_count"][:, 1].tolist() == [9, 9, 9], s0["pc_count"]
    E, now, ref = run_short(fans_batch(), 0, make_backend, snaps, "hcap", [1], dict(FANS_CAPS, **FANS_KW), name=HCAP_NAME)
    assert int(E.W.shape_rare) == 0 and int(E.W.shape_box) == 0


# ---- the neural narrow phase's query lists (bits 32 and 64), device only -------------------------------------------------------
IGR_QCAP_NAME = "igr_qcap (query list of the neural narrow phase)"


def igr_spec():
    """rollout_igr_small, the smallest neural-body scene of test_igr_stepper_gpu.py, twice along the batch axis."""
    import igr_helpers as H
    import rollout_helpers as R
    g = R.load_rollout("rollout_igr_small")
    return H.spec_from_golden(g, 2), H.engine_kwargs(g)


def igr_reference(make_backend):
    """One detection (construction) with the engine's own sizing of igr_items_cap and igr_qcap: it never flags, the item list
    fits, and the rounds in use stay below IGR_ROUNDS = 42 (so bit 64, narrowphase_igr.hip:578, is out of reach of this
    scene; IGR_ROUNDS is not shrunk to get there).  -> (the largest igr_qn entry, rounds in use, the outputs)."""
    key = ("igr", getattr(make_backend, "__name__", str(make_backend)))
    if key not in _NEED:
        spec, kw = igr_spec()
        be = guarded(make_backend())
        E, err = build_engine(spec, be, **kw)
        assert err is None, err
        snap, qn = snapshot(E), np.array(E.get("igr_qn"), copy=True)
        assert (snap["overflow"] == 0).all(), snap["overflow"]
        assert 0 < int(snap["n_pairs"][6]) <= E.igr_items_cap, (snap["n_pairs"], E.igr_items_cap)     # narrowphase.hip:133-136
        rounds = int(qn.reshape(-1, 2).any(axis=1).sum())
        print("igr_qn max %d of igr_qcap %d, %d rounds in use of %d" % (qn.max(), E.igr_qcap, rounds, abi.IGR_ROUNDS))
        assert 0 < rounds < abi.IGR_ROUNDS, rounds
        be.assert_guards_intact()
        _NEED[key] = (int(qn.max()), rounds, snap)
    return _NEED[key]


def check_igr_qcap(delta, make_backend):
    """spec['igr_qcap'] = the largest list of the detection + delta.  The lists are shared by the batch and their slots are
    reserved with atomics (narrowphase_igr.hip:66-75), so the need is the batch's: with one slot short at least one scene is
    flagged with bit 32 alone (which one is the order of the reservations), the error names igr_qcap, the list lengths stay
    within the capacity and a scene that is not flagged equals the ample run; with enough, no flag and every output ==."""
    need, _rounds, ref = igr_reference(make_backend)
    spec, kw = igr_spec()
    spec["igr_qcap"] = need + delta
    be = guarded(make_backend())
    E, err = build_engine(spec, be, **kw)
    be.assert_guards_intact()
    now = snapshot(E)
    assert int(np.max(E.get("igr_qn"))) <= need + delta
    if delta >= 0:
        assert err is None and (now["overflow"] == 0).all(), (err, now["overflow"])
        for s in range(E.B):
            _scene_equal(now, ref, s, "igr_qcap = need + %d" % delta)
        return
    assert err is not None, "no capacity error with igr_qcap one short of the need"
    scene, names = limit_named(err)
    assert names == IGR_QCAP_NAME, str(err)
    ov = now["overflow"]
    assert set(ov.tolist()) <= {0, BITS["igr_qcap"]} and ov.any() and scene == int(np.nonzero(ov)[0][0]), ov
    for s in range(E.B):
        if ov[s] == 0:
            _scene_equal(now, ref, s, "unflagged scene, igr_qcap one short")


def fast_sphere():
    import rollout_helpers as R
    return R.spec_from_golden(R.load_rollout("rollout_fast_sphere"), 3)


def fast_sphere_kw():
    import rollout_helpers as R
    kw = R.engine_kwargs(R.load_rollout("rollout_fast_sphere"))
    return {k: v for k, v in kw.items() if k not in AMPLE}


SPECS = {
    "plate": lambda: plate_batch((PLATE_N - 5, PLATE_N, PLATE_N - 9)),
    "plate_wg": lambda: plate_batch((PLATE_N - 5, PLATE_N, PLATE_N - 9), ntop=2100),
    "little_stack": little_stack,
    "fast_sphere": fast_sphere,
}
NSTEPS = {"plate": 2, "plate_wg": 1, "little_stack": 2, "fast_sphere": 3}
_NEED = {}


def need_of(name, make_backend):
    """measure_need of a named batch, once per backend class."""
    key = (name, getattr(make_backend, "__name__", str(make_backend)))
    if key not in _NEED:
        kw = fast_sphere_kw() if name == "fast_sphere" else KW
        _NEED[key] = measure_need(SPECS[name](), NSTEPS[name], make_backend, **kw)
    return _NEED[key]


def search_path(snaps, path):
    """Which search path the plate -> floor / box -> floor items took, from the work lists of the last detection: n_pairs =
    {workgroup-list length, wavefront-list length, ., ., deferred-list length}."""
    for s in snaps:
        n = s["n_pairs"]
        if path == "wave":
            assert n[0] == 0 and n[1] > 0 and n[4] == 0, n
        else:
            assert n[0] == len(s["nc"]) and n[4] == 0, n


def check_limit(name, limit, delta, make_backend):
    """Section 4 for one batch, one limit and K = K* + delta.  The plates need the same max_pc and maxc in every scene (the
    hull keeps the corners whatever N is) and rollout_fast_sphere is one scene three times: there every scene is flagged at
    K* - 1 and the neighbour comparison has nothing to compare -- for max_pc and maxc it runs on little_stack; the clamp of
    emit_unfiltered is checked by the flag, the clamped count, the head of the ample list and the guards only."""
    need, snaps = need_of(name, make_backend)
    kw = fast_sphere_kw() if name == "fast_sphere" else KW
    if name != "fast_sphere" and not (name.startswith("plate") and limit != "max_cand"):
        assert_dialled(need, limit)
    caps, flagged = caps_for(need, limit, delta)
    if delta >= 0:
        return run_enough(SPECS[name](), NSTEPS[name], make_backend, snaps, **caps, **kw)
    return run_short(SPECS[name](), NSTEPS[name], make_backend, snaps, limit, flagged, dict(caps, **kw))[0]


def assert_takes_emit_unfiltered(need, snaps):
    """rollout_fast_sphere's largest per-pair count is written by emit_unfiltered (np_common.h:889-904: the count is stored
    negative), and no thinned list is as long: one short of it crosses that clamp and no other."""
    k = int(need["max_pc"].max())
    assert min(int(s["pc_count"].min()) for s in snaps) == -k
    assert max(int(s["pc_count"].max()) for s in snaps) < k


def corner_faces(M):
    """What the hull of the middle plate's contact cluster keeps, from the mesh: Frank-Wolfe starts a face whose vertices are
    equally far from the floor at the first of them, so the cluster's points are the rim points of the bottom face, the
    corners several times over (bottom fan and side triangles).  The rim points on the edges are collinear with the corners:
    the hull's vertices -- Qhull's vertex semantics -- are the four corners, and of coincident points the first in
    ascending face order is kept: per corner, the lowest face id whose first vertex lies there."""
    v, f, _c = plate_mesh(M - 8, HCAP_TOP)
    hx, hy, hz = (0.5 * d for d in PLATE_DIMS)
    first = v[f[:, 0]]
    return sorted(int(np.nonzero((first == np.array([x, -hy, z])).all(axis=1))[0][0]) for x in (-hx, hx) for z in (-hz, hz))


def hcap_reference(M, make_backend):
    """The full variant on the HCAP plates (no cluster limit: the reference of the lean runs), one detection."""
    key = ("hcap", M, getattr(make_backend, "__name__", str(make_backend)))
    if key not in _NEED:
        _NEED[key] = measure_need(hcap_batch(M, True), 0, make_backend, **KW)
    return _NEED[key]


def check_hcap_lean(M, make_backend):
    """Lean variant, clusters of M - 5, M, M - 9 contacts.  M <= 1024: no flag, every output equal to the full variant's
    with ==.  M = 1025: bit 2 alone in scene 1 alone (np_filter_emit.inc:91), the neighbours intact."""
    _need, snaps = hcap_reference(M, make_backend)
    search_path(snaps, "workgroup")
    if M <= HCAP:
        E = run_enough(hcap_batch(M), 0, make_backend, snaps, **AMPLE, **KW)
        assert int(E.W.shape_rare) == 0
        return
    run_short(hcap_batch(M), 0, make_backend, snaps, "hcap", [1], dict(AMPLE, **KW), name=HCAP_NAME)


def check_hcap_full(M, make_backend):
    """Full variant, a cluster of 1025 contacts: no flag (the hull in the global scratch, np_filter_emit.inc:65-80); the kept
    contacts of plate -> floor are corner_faces, and the contact set is the step oracle's."""
    _need, snaps = hcap_reference(M, make_backend)
    s0 = snaps[0]
    assert (s0["overflow"] == 0).all()
    got = sorted(int(x) & 0x3fffffff for x in s0["pc_face"][1, 1, :s0["pc_count"][1, 1]])
    assert got == corner_faces(M), (got, corner_faces(M))
    check_against_oracle(("hcap", M), s0)
