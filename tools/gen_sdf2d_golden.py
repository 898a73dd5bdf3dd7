"""Golden vectors of the reference's 2-D SDF layer (sdf_physics/physics/bodies.py, contacts.py), recorded by running the
reference itself through oracle.refshim -> tests/golden/sdf2d_{query,surface,contacts,contacts_grad,rollouts}.npz (float64).
Run where the reference tree is present:  python tools/gen_sdf2d_golden.py [query surface contacts grad rollouts]

Conditions on the recorded pairs (checked here, a pair that misses one is drawn again), so that a comparison decided by the
last bits of a matrix product cannot separate an implementation from the reference:
  * every cull comparison (phi < radius of the edge) is an exact tie (axis-aligned rects: exact arithmetic on both sides) or
    off its threshold by more than 1e-7 x the body's scale, every phi <= eps is off by that much; every singular value of the thinning is a factor 10 away from 1e-5;
  * every end-point comparison of every Frank-Wolfe iteration of a kept contact is an exact tie or separated by more than
    1e-9 x the scale;
  * with dimension 1, the two extremes along the principal direction are unique by more than 1e-7 x the scale.
torch is seeded before each pair (pca_lowrank draws random numbers)."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

refshim.install()
from lcp_physics.physics.constraints import TotalConstraint  # noqa: E402
from lcp_physics.physics.forces import Gravity  # noqa: E402
from lcp_physics.physics.world import World  # noqa: E402
from sdf_physics.physics.bodies import SDFBowl, SDFCircle, SDFGrid, SDFRect  # noqa: E402
from sdf_physics.physics.contacts import SDFContactHandler  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS = 0.1
WHY = []      # why the last rejected pair was rejected
CIRCLE, RECT, BOWL, GRID = 0, 1, 2, 3
CAP, CANDCAP = 40, 160
T = lambda x, g=False: torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=g)      # noqa: E731


def grid_samples():
    """Three sample arrays over [-0.5, 0.5]^2 in unit-frame distances: a disc (33 x 33), a rounded square (17 x 17) and an
    L-shape (21 x 33: concave, its sides on sample rows, so values hit the 1e-5 snap of the outline)."""
    def axes(n0, n1):
        return np.meshgrid(np.linspace(-0.5, 0.5, n0), np.linspace(-0.5, 0.5, n1), indexing="ij")
    x, y = axes(33, 33)
    disc = np.sqrt(x * x + y * y) - 0.3
    x, y = axes(17, 17)
    qx, qy = np.abs(x) - 0.2, np.abs(y) - 0.2
    rsq = np.sqrt(np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2) + np.minimum(np.maximum(qx, qy), 0) - 0.1
    x, y = axes(21, 33)
    box = lambda cx, cy, hx, hy: np.maximum(np.abs(x - cx) - hx, np.abs(y - cy) - hy)      # noqa: E731
    ell = np.minimum(box(-0.15, 0.0, 0.1, 0.25), box(0.0, -0.1875, 0.25, 0.0625))
    return [disc, rsq, ell]


GRIDS = grid_samples()


def make(rec, grad=False):
    """A reference body from a record (kind, pose [3], prm [2], scale, grid); grad: every number is a leaf.  Returns the body
    and its leaves {pose, prm, scale}."""
    kind = int(rec["kind"])
    pose, prm = T(rec["pose"], grad), T(rec["prm"], grad)
    if kind == CIRCLE:
        b = SDFCircle(pose, prm[0])
    elif kind == RECT:
        b = SDFRect(pose, prm)
    elif kind == BOWL:
        b = SDFBowl(pose, prm[0], prm[1])
    else:
        b = SDFGrid(pose, T(rec["scale"], grad), T(GRIDS[int(rec["grid"])]))
    scale = b.scale
    if kind != GRID:
        assert abs(float(b.scale) - float(rec["scale"])) <= 1e-12 * float(rec["scale"])
        if grad:      # the scale as a leaf of its own, beside the parameters it was computed from
            scale = b.scale = T(float(rec["scale"]), True)
    return b, dict(pose=pose, prm=prm, scale=scale)


def record(kind, rng, pos=(0.0, 0.0), rot=None, grid=None):
    rot = rng.uniform(-math.pi, math.pi) if rot is None else rot
    rec = dict(kind=kind, pose=np.array([rot, pos[0], pos[1]]), prm=np.zeros(2), scale=0.0, grid=0)
    if kind == CIRCLE:
        rec["prm"][0] = rng.uniform(1.0, 3.0); rec["scale"] = rec["prm"][0] * 2 * 1.3333
    elif kind == RECT:
        rec["prm"] = rng.uniform(2.0, 6.0, 2); rec["scale"] = rec["prm"].max() * 1.5
    elif kind == BOWL:
        rec["prm"] = np.array([rng.uniform(2.0, 4.0), rng.uniform(0.2, 0.6)]); rec["scale"] = (rec["prm"][0] + rec["prm"][1]) * 2 * 1.3333
    else:
        rec["grid"] = int(rng.integers(0, 3)) if grid is None else grid
        rec["scale"] = rng.uniform(4.0, 8.0)
    return rec


def extent(rec):
    k = int(rec["kind"])
    return {CIRCLE: rec["prm"][0], RECT: 0.5 * np.hypot(*rec["prm"]), BOWL: rec["prm"][0] + rec["prm"][1], GRID: 0.36 * rec["scale"]}[k]


class Stub:
    def __init__(self, bodies):
        self.bodies, self.eps, self.contacts = bodies, EPS, []


class Geom:
    def __init__(self, i):
        self.body, self.no_contact = i, set()


def flat(c):
    return torch.cat([c[0].reshape(-1), c[1].reshape(-1), c[2].reshape(-1), c[3].reshape(-1)])


def trace(verts, edges, body, direction, pos1, pos2):
    """The search of one direction step by step on the reference's own queries: tuples, (direction, edge), t of the contacts,
    and whether the conditions of the module docstring hold."""
    sc = float(body.scale)
    ab = verts[edges]
    x = ab.mean(dim=1)
    phi, g = body.query_sdfs(x)
    rads = (x.unsqueeze(1) - ab).norm(dim=2).max(dim=1)[0]
    ok = bool(((phi == rads) | ((phi - rads).abs() > 1e-7 * sc)).all())
    keep = (phi < rads) & ~torch.all(g == 0, dim=1)
    idx = torch.nonzero(keep).reshape(-1)
    if len(idx) == 0:
        return np.zeros((0, 7)), np.zeros((0, 2), np.int32), np.zeros(0), ok
    x, ab = x[keep], ab[keep]
    t = torch.full((len(idx),), 0.5, dtype=torch.float64)
    fine = torch.ones(len(idx), dtype=torch.bool)
    for it in range(32):
        _, g = body.query_sdfs(x)
        dab = (ab @ g.unsqueeze(2)).squeeze(2)
        diff = dab[:, 0] - dab[:, 1]
        fine &= (diff == 0) | (diff.abs() > 1e-9 * sc)
        ind = dab.argmin(dim=1)
        gamma = 2.0 / (it + 2.0)
        x = (1.0 - gamma) * x + gamma * ab[torch.arange(len(idx)), ind]
        t = (1.0 - gamma) * t + gamma * ind.double()
    phi, g = body.query_sdfs(x)
    hit = phi <= EPS
    if not bool(((phi - EPS).abs() > 1e-7 * sc).all()) or not bool(fine[hit].all()):
        WHY.append("eps margin %s, end-point margin %s" % (bool(((phi - EPS).abs() > 1e-7 * sc).all()), bool(fine[hit].all())))
        ok = False
    x, phi, g = x[hit], phi[hit], g[hit]
    rows = torch.cat([-g if direction else g, (x - pos1) - phi[:, None] * g, (x - pos2) - phi[:, None] * g, -phi[:, None]], 1)
    tags = np.stack([np.full(int(hit.sum()), direction), idx[hit].numpy()], 1).astype(np.int32)
    return rows.detach().numpy(), tags, t[hit].detach().numpy(), ok


def run_pair(r1, r2, seed, grad=False):
    """The reference's handler on one pair -> a record, or None if a condition of the module docstring fails."""
    torch.manual_seed(seed)
    (b1, l1), (b2, l2) = make(r1, grad), make(r2, grad)
    w = Stub([b1, b2])
    try:
        SDFContactHandler()([w], Geom(0), Geom(1))
    except Exception as e:      # the hull of tensors that require grad (the reference's defect): no such pair in the grad file
        if grad:
            return None
        raise e
    with torch.no_grad():
        v1, e1 = b1.get_surface()
        v2, e2 = b2.get_surface()
        ca, ta, pa, oka = trace(v1, e1, b2, 0, b1.pos, b2.pos)
        cb, tb, pb, okb = trace(v2, e2, b1, 1, b1.pos, b2.pos)
    cand, ctag, ct = np.concatenate([ca, cb]), np.concatenate([ta, tb]), np.concatenate([pa, pb])
    if not (oka and okb) or len(cand) > CANDCAP or len(w.contacts) > CAP:
        WHY.append("margins %s %s, %d candidates, %d contacts" % (oka, okb, len(cand), len(w.contacts)))
        return None
    out = np.stack([flat(c[0]).detach().numpy() for c in w.contacts]) if w.contacts else np.zeros((0, 7))
    dim = -1
    if len(cand) > 1:
        p = cand[:, 2:4] - cand[:, 2:4].mean(0)
        s = np.linalg.svd(p, compute_uv=False)
        if np.any((s > 1e-6) & (s < 1e-4)):
            return None
        dim = int((s > 1e-5).sum())
        if dim == 1:
            proj = np.sort(p @ np.linalg.svd(p)[2][0])
            if proj[1] - proj[0] < 1e-7 * float(b1.scale) or proj[-1] - proj[-2] < 1e-7 * float(b1.scale):
                return None
    # every contact the handler kept is one of the traced candidates, bit for bit
    which = []
    for row in out:
        m = np.nonzero((cand == row).all(1))[0]
        assert len(m) >= 1, "a kept contact is not among the traced candidates"
        which.append(int(m[0]))
    assert len(set(which)) == len(which) == (len(out) if len(cand) > 1 else len(cand))
    pad = lambda a, n, dt=np.float64: np.concatenate([a, np.zeros((n - len(a),) + a.shape[1:], dt)]).astype(dt)      # noqa: E731
    rec = dict(kind=np.array([r1["kind"], r2["kind"]], np.int32), pose=np.stack([r1["pose"], r2["pose"]]),
               prm=np.stack([r1["prm"], r2["prm"]]), scale=np.array([r1["scale"], r2["scale"]]),
               grid=np.array([r1["grid"], r2["grid"]], np.int32), seed=np.int64(seed), dim=np.int32(dim),
               count=np.int32(len(out)), out=pad(out, CAP), tag=pad(ctag[which].reshape(-1, 2), CAP, np.int32), tpar=pad(ct[which], CAP),
               ncand=np.int32(len(cand)), cand=pad(cand, CANDCAP), cand_tag=pad(ctag, CANDCAP, np.int32),
               nedge=np.array([len(e1), len(e2)], np.int32))
    if grad:
        if len(out) == 0 or dim > 1:
            return None
        gout = np.random.default_rng(seed).normal(size=(CAP, 7))
        loss = sum((flat(c[0]) * T(gout[q])).sum() for q, c in enumerate(w.contacts))
        leaves = [l1["pose"], l1["prm"], l1["scale"], l2["pose"], l2["prm"], l2["scale"]]
        try:
            gr = torch.autograd.grad(loss, leaves, allow_unused=True)
        except RuntimeError:      # the reference's bowl query writes in place into what its backward needs: no recorded autograd
            return None
        gr = [np.zeros(tuple(l.shape)) if x is None else x.numpy() for x, l in zip(gr, leaves)]
        rec.update(gout=gout, g_pose=np.stack([gr[0], gr[3]]), g_prm=np.stack([gr[1], gr[4]]), g_scale=np.array([float(gr[2]), float(gr[5])]))
    return rec


def pack(d):
    """Ragged storage: the contacts before thinning of all pairs row after row (`ncand` per pair), the kept contacts as row
    numbers into their pair's candidates (`count` per pair) with their edge coordinate, `gout` only for rows that exist.
    tests/sdf2d_helpers.py unpacks.  Keeps the files well under the largest golden of the suite."""
    n, m = d["ncand"], d["count"]
    keep = []
    for p in range(len(n)):
        for q in range(m[p]):
            hit = np.nonzero((d["cand_tag"][p, :n[p]] == d["tag"][p, q]).all(1))[0]
            assert len(hit) == 1 and np.array_equal(d["cand"][p, hit[0]], d["out"][p, q])
            keep.append(hit[0])
    rows = lambda a, k: np.concatenate([a[p, :k[p]] for p in range(len(k))])      # noqa: E731
    out = {k: v for k, v in d.items() if k not in ("out", "tag", "tpar", "cand", "cand_tag", "gout")}
    # (p2 is left out: it is p1 + pos1 - pos2 to a few ulps of the coordinates, and is rebuilt so when the file is read)
    out.update(cand_rows=rows(d["cand"], n)[:, [0, 1, 2, 3, 6]], cand_tag_rows=rows(d["cand_tag"], n).astype(np.int16), keep_rows=np.array(keep, np.int16),
               tpar_rows=rows(d["tpar"], m))
    if "gout" in d:
        out["gout_rows"] = rows(d["gout"], m)
    return out


def random_pair(rng, k1, k2, touching, shallow=False):
    r2 = record(k2, rng, pos=rng.uniform(-20, 20, 2))
    r1 = record(k1, rng)
    R = extent(r1) + extent(r2)
    th = rng.uniform(0, 2 * math.pi)
    d = R * ((rng.uniform(0.6, 1.03) if shallow else rng.uniform(0.45, 1.0)) if touching else rng.uniform(1.05, 1.6))
    r1["pose"][1:] = r2["pose"][1:] + d * np.array([math.cos(th), math.sin(th)])
    return r1, r2


def special_pairs(rng):
    """The named cases of the issue: (name, r1, r2)."""
    S = []
    rect = lambda pos, dims, rot=0.0: dict(kind=RECT, pose=np.array([rot, pos[0], pos[1]]), prm=np.array(dims, float), scale=max(dims) * 1.5, grid=0)      # noqa: E731
    circ = lambda pos, rad: dict(kind=CIRCLE, pose=np.array([0.3, pos[0], pos[1]]), prm=np.array([rad, 0.0]), scale=rad * 2 * 1.3333, grid=0)      # noqa: E731
    bowl = lambda pos, r, d, rot=0.0: dict(kind=BOWL, pose=np.array([rot, pos[0], pos[1]]), prm=np.array([r, d]), scale=(r + d) * 2 * 1.3333, grid=0)      # noqa: E731
    grid = lambda pos, sc, g, rot=0.0: dict(kind=GRID, pose=np.array([rot, pos[0], pos[1]]), prm=np.zeros(2), scale=sc, grid=g)      # noqa: E731
    S.append(("aligned_rects", rect((0.0, 0.0), (4.0, 2.0)), rect((0.5, 3.0), (6.0, 4.0))))
    S.append(("corner_in_face", rect((0.0, 0.0), (3.0, 3.0), math.pi / 4), rect((0.0, 4.1), (8.0, 4.0))))
    S.append(("circle_in_bowl", circ((0.554, -0.022), 1.0), bowl((0.0, 0.0), 3.0, 0.4)))
    S.append(("circle_concentric_in_bowl", circ((0.013, 1.47), 2.55), bowl((0.0, 0.0), 3.0, 0.4)))
    S.append(("grid_disc_on_rect", grid((0.0, 0.0), 10.0, 0, 0.2), rect((0.3, 4.95), (12.0, 4.0))))
    S.append(("grid_disc_in_bowl", grid((0.013, 1.47), 8.5, 0, 0.1), bowl((0.0, 0.0), 3.0, 0.4)))
    S.append(("two_grid_discs", grid((0.0, 0.0), 10.0, 0, 0.4), grid((5.9, 0.3), 10.0, 0, 1.1)))
    return S


def contacts(grad=False):
    rng = np.random.default_rng(23 if grad else 17)
    recs, names = [], []
    seed = 1000
    if not grad:
        for name, r1, r2 in special_pairs(rng):
            rec, base = run_pair(r1, r2, seed), r1["pose"].copy()
            for _ in range(60):      # a condition on the inputs fails: move the scene a little, keep what it is a case of
                if rec is not None and (rec["count"] > 0):
                    break
                r1["pose"][1:] = base[1:] + rng.uniform(-0.02, 0.02, 2)
                rec = run_pair(r1, r2, seed)
            seed += 1
            assert rec is not None, name + ": a condition on the inputs fails, move the scene " + str(WHY[-3:])
            recs.append(rec); names.append(name)
            print("%-28s count %d of %d candidates, dim %d, edges %s" % (name, rec["count"], rec["ncand"], rec["dim"], rec["nedge"]))
    combos = [(a, b) for a in range(4) for b in range(a, 4)]
    quota = {True: 18, False: 0} if grad else {True: 22, False: 10}
    for k1, k2 in combos:
        for touching in (True, False):
            have = tries = 0
            while have < quota[touching]:
                tries += 1
                if grad and BOWL in (k1, k2) and tries > 60 and have == 0:
                    break      # (see run_pair: pairs with a bowl have no recorded autograd; they are checked by finite differences)
                assert tries < 20000, (k1, k2, touching)
                a, b = (k1, k2) if rng.uniform() < 0.5 else (k2, k1)
                r1, r2 = random_pair(rng, a, b, touching, shallow=grad)      # (few contacts: dimension <= 1)
                seed += 1
                rec = run_pair(r1, r2, seed, grad)
                if rec is None or (rec["count"] > 0) != touching:
                    continue
                recs.append(rec); names.append("%d%d" % (a, b)); have += 1
    d = pack({k: np.stack([r[k] for r in recs]) for k in recs[0]})
    d["eps"] = np.float64(EPS)
    d["names"] = np.array(names)
    if not grad:
        for i, g in enumerate(GRIDS):
            d["grid%d" % i] = g
    np.savez_compressed(os.path.join(GOLDEN, "sdf2d_contacts_grad.npz" if grad else "sdf2d_contacts.npz"), **d)
    print("%d pairs; counts %s; dims %s; max candidates %d" % (len(recs), np.bincount(d["count"]), np.bincount(d["dim"] + 1), d["ncand"].max()))


def query_and_surface():
    rng = np.random.default_rng(5)
    q, s = {}, {}
    bodies = [("circle", dict(kind=CIRCLE, pose=np.array([0.4, 1.0, -2.0]), prm=np.array([1.5, 0.0]), scale=1.5 * 2 * 1.3333, grid=0)),
              ("rect", dict(kind=RECT, pose=np.array([-0.7, 3.0, 1.0]), prm=np.array([4.0, 2.5]), scale=6.0, grid=0)),
              ("bowl", dict(kind=BOWL, pose=np.array([0.25, -1.0, 0.5]), prm=np.array([3.0, 0.4]), scale=3.4 * 2 * 1.3333, grid=0))]
    bodies += [("grid%d" % g, dict(kind=GRID, pose=np.array([0.3 * g - 0.2, 0.5, -0.5 + g]), prm=np.zeros(2), scale=6.0 + g, grid=g)) for g in range(3)]
    for name, rec in bodies:
        b, _ = make(rec)
        sc, k = float(b.scale), int(rec["kind"])
        loc = [rng.uniform(-0.6, 0.6, (120, 2)) * sc, np.zeros((1, 2))]
        edge = np.array([[0.5, 0.1], [-0.5, 0.2], [0.1, 0.5], [0.3, -0.5], [0.5, 0.5], [0.5 - 1e-9, 0.2], [0.5 + 1e-9, 0.2], [0.55, 0.0]]) * sc
        loc.append(edge)
        if k == RECT:
            h = rec["prm"] / 2
            loc.append(np.array([[h[0], 0.3], [h[0], h[1]], [-h[0], -h[1]], [0.0, h[1]], [h[0] + 0.2, h[1] + 0.1], [0.5, 0.5], [h[0] - 0.1, h[1] - 0.1], [0.0, 1e-3]]))
        if k == BOWL:
            r = rec["prm"][0]
            loc.append(np.stack([rng.uniform(-1.2, 1.2, 30) * r, np.full(30, r / 2)], 1))
            loc.append(np.stack([np.concatenate([np.full(15, r), np.full(15, -r)]), rng.uniform(-0.8, 1.2, 30) * r], 1))
        if k == GRID:
            n0, n1 = GRIDS[rec["grid"]].shape
            ii, jj = np.meshgrid(np.arange(0, n0, 4), np.arange(0, n1, 4), indexing="ij")
            loc.append(np.stack([(ii.ravel() / (n0 - 1) - 0.5) * sc, (jj.ravel() / (n1 - 1) - 0.5) * sc], 1))
        loc = np.concatenate(loc)
        if k == CIRCLE:
            loc = loc[np.abs(loc).sum(1) > 0]      # (the centre of a circle has no gradient: 0 / 0)
        c, sn = math.cos(rec["pose"][0]), math.sin(rec["pose"][0])
        pts = loc @ np.array([[c, -sn], [sn, c]]).T + rec["pose"][1:]
        with torch.no_grad():
            phi, g = b.query_sdfs(T(pts))
            verts, edges = b.get_surface()
        fin = np.isfinite(g.numpy()).all(1)
        for key in ("kind", "pose", "prm", "scale", "grid"):
            q["%s_%s" % (name, key)] = s["%s_%s" % (name, key)] = np.asarray(rec[key])
        q[name + "_pts"], q[name + "_sdf"], q[name + "_grad"] = pts[fin], phi.numpy()[fin], g.numpy()[fin]
        s[name + "_verts"], s[name + "_edges"], s[name + "_inertia"] = verts.numpy(), edges.numpy(), float(b.ang_inertia)
        if k == GRID:
            s[name + "_unit_verts"] = (b.verts / b.scale).numpy()
        print("%-8s %3d points (%d inside), %d vertices, %d edges, inertia %.6f" %
              (name, fin.sum(), (phi.numpy()[fin] < sc * 0.999).sum(), len(verts), len(edges), float(b.ang_inertia)))
    for i, g in enumerate(GRIDS):
        q["grid%d_samples" % i] = s["grid%d_samples" % i] = g
    # a saddle: cells with two crossings (classes 5 and 10 of the marching squares)
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, 6), np.linspace(-0.5, 0.5, 7), indexing="ij")
    saddle = (x + 0.03) * (y - 0.02) * np.where((np.abs(x) < 0.3) & (np.abs(y) < 0.3), 1.0, -1.0) + 0.001
    b = SDFGrid(T([0.0, 0.0, 0.0]), T(1.0), T(saddle))
    inner = saddle < 0
    cls = 8 * inner[:-1, :-1] + 4 * inner[:-1, 1:] + 2 * inner[1:, 1:] + inner[1:, :-1]
    s["saddle_samples"], s["saddle_unit_verts"], s["saddle_edges"] = saddle, (b.verts / b.scale).numpy(), b.edges.numpy()
    s["saddle_two_crossings"] = np.int64(((cls == 5) | (cls == 10)).sum())
    print("saddle: %d vertices, %d edges, %d cells with two crossings" % (len(b.verts), len(b.edges), s["saddle_two_crossings"]))
    np.savez_compressed(os.path.join(GOLDEN, "sdf2d_query.npz"), **q)
    np.savez_compressed(os.path.join(GOLDEN, "sdf2d_surface.npz"), **s)


def rollout(name, make_world, nsteps, **world_kw):
    torch.manual_seed(0)
    bodies, leaf, loss_of = make_world()
    w = World(bodies, [TotalConstraint(bodies[0])], dt=1.0 / 30, contact_callback=SDFContactHandler, **world_kw)
    pairs, traj = [], []
    for _ in range(nsteps):
        w.step()
        row = np.full((16, 2), -1, np.int64)
        for k, c in enumerate(w.contacts):
            row[k] = (c[1], c[2])
        pairs.append(row)
        traj.append(torch.cat([b.p for b in bodies]).detach().numpy())
    loss = loss_of(bodies)
    g = torch.autograd.grad(loss, [leaf])[0] if leaf is not None else float("nan")      # (None: a world recorded without grad)
    print("%-14s %d steps, %d sub-steps, loss %.6f, gradient %.6f, most contacts %d" %
          (name, nsteps, len(w.trajectory), float(loss), float(g), max((r[:, 0] >= 0).sum() for r in pairs)))
    return {name + "_pairs": np.stack(pairs), name + "_traj_p": np.stack(traj), name + "_loss": float(loss), name + "_grad": float(g),
            name + "_n_substeps": np.int64(len(w.trajectory))}


def rollouts():
    """Four worlds of the reference with these bodies.  The circle dropped off-centre into a pinned bowl is recorded WITHOUT
    grad (poses, contact pairs, sub-steps, loss): its contacts span two dimensions in every scene tried (bowl radius 100 to 300,
    ball radius 5 to 20, eps 0.01 to 0.1), and the reference's hull refuses tensors that require grad, which every state is
    after the first contact.  The build's d loss / d rad of that world is checked by finite differences of the build."""
    kw = dict(restitution=0.5, fric_coeff=0.9)

    def circle_on_rect():
        rad = T(20.0, True)
        floor, ball = SDFRect([500, 600], [1000, 50], **kw), SDFCircle([500, 480], rad, vel=[0, 30, 0], **kw)
        ball.add_force(Gravity(g=100))
        return [floor, ball], rad, lambda b: (b[1].pos ** 2).sum()

    def tilted_rect():
        wd = T(80.0, True)
        floor = SDFRect([500, 600], [1000, 50], **kw)
        box = SDFRect([0.3, 420, 520], torch.stack([wd, wd.new_tensor(50.0)]), **kw)
        box.add_force(Gravity(g=100))
        return [floor, box], wd, lambda b: (b[1].p ** 2).sum()

    def circle_in_bowl():      # (turned by pi: the bowl opens upwards, y points down)
        bowl, ball = SDFBowl([math.pi, 500, 500], 100.0, 10.0, **kw), SDFCircle([470, 505], 20.0, **kw)
        ball.add_force(Gravity(g=100))
        return [bowl, ball], None, lambda b: (b[1].pos ** 2).sum()

    def grid_disc():
        sc = T(100.0, True)
        floor = SDFRect([500, 600], [1000, 50], **kw)
        disc = SDFGrid([500, 520], sc, T(GRIDS[0]), vel=[2.0, 20, 0], **kw)
        disc.add_force(Gravity(g=100))
        return [floor, disc], sc, lambda b: (b[1].p ** 2).sum()

    d = {}
    for name, mk, n in (("circle_on_rect", circle_on_rect, 50), ("tilted_rect", tilted_rect, 40), ("circle_in_bowl", circle_in_bowl, 45),
                        ("grid_disc", grid_disc, 30)):
        d.update(rollout(name, mk, n))
    d["grid_disc_samples"] = GRIDS[0]
    np.savez_compressed(os.path.join(GOLDEN, "sdf2d_rollouts.npz"), **d)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    what = sys.argv[1:] or ["query", "contacts", "grad", "rollouts"]
    if "query" in what or "surface" in what:
        query_and_surface()
    if "contacts" in what:
        contacts()
    if "grad" in what:
        contacts(grad=True)
    if "rollouts" in what:
        rollouts()
