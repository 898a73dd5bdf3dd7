"""Golden gradients with respect to the samples of a 2-D grid body, recorded by running the reference itself (oracle.refshim)
-> tests/golden/sdf2d_grid_grad.npz (float64).  Run where the reference tree is present:  python tools/gen_sdf2d_grid_grad_golden.py

The reference differentiates a grid's QUERY with respect to its samples by plain autograd (`SDFGrid.query_sdfs` interpolates
`sdf` and the central differences of `sdf`).  It cannot differentiate a grid's OUTLINE (`marching_squares` ends in
`unique(dim=0)`, whose derivative torch does not implement), so everything recorded here keeps the outline of the grid whose
samples require grad out of the loss:
  (a) q<i>_*: `query_sdfs` of the 17 x 17 and the 21 x 33 grid at points in interior cells, in border cells (where one central
      difference is zero) and outside the box, with random cotangents on (phi, g): d (cot . (phi, g)) / d sdf, dense.
  (b) per pair: the reference's SDFContactHandler on a pair of the grid (samples require grad) and a circle, a rect or a second
      grid without grad.  The loss is sum gout . tuple over the kept contacts that lie on an edge of the OTHER body (the grid is
      the body queried); kept contacts on the grid's own edges get gout = 0 and stay out of the loss.  d loss / d sdf, dense.
The margin conditions of tools/gen_sdf2d_golden.py hold for every pair (a pair that misses one is drawn again), and the
reference's backward is run for every recorded pair: a pair whose backward raises is a defect of this generator."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_sdf2d_golden as base  # noqa: E402  (installs the reference through oracle.refshim)
from gen_sdf2d_golden import CIRCLE, GRID, RECT, SDFContactHandler, SDFGrid, T  # noqa: E402

PER_COMBO = 4
NMAX = 21 * 33


def query_set(gi, rng):
    sdf = T(base.GRIDS[gi], True)
    sc, pose = 5.0 + gi, np.array([0.3 * gi - 0.2, 0.5, -0.5 + gi])
    b = SDFGrid(T(pose), T(sc), sdf)
    n0, n1 = base.GRIDS[gi].shape
    cell = np.array([1.0 / (n0 - 1), 1.0 / (n1 - 1)])
    border = np.concatenate([np.stack([s * (0.5 - rng.uniform(0.05, 0.95, 6) * cell[0]), rng.uniform(-0.45, 0.45, 6)], 1) for s in (-1, 1)] +
                            [np.stack([rng.uniform(-0.45, 0.45, 6), s * (0.5 - rng.uniform(0.05, 0.95, 6) * cell[1])], 1) for s in (-1, 1)])
    loc = np.concatenate([rng.uniform(-0.5 + 1.5 * cell, 0.5 - 1.5 * cell, (40, 2)), border, rng.uniform(0.51, 0.6, (6, 2)) * rng.choice([-1, 1], (6, 2))]) * sc
    c, s = np.cos(pose[0]), np.sin(pose[0])
    pts = loc @ np.array([[c, -s], [s, c]]).T + pose[1:]
    phi, g = b.query_sdfs(T(pts))
    cot_phi, cot_g = rng.normal(size=len(pts)), rng.normal(size=(len(pts), 2))
    (gs,) = torch.autograd.grad((phi * T(cot_phi)).sum() + (g * T(cot_g)).sum(), [sdf])
    inside = phi.detach().numpy() < sc
    print("query set %d: %d points, %d inside, %d in border cells, |d sdf| max %.3f" % (gi, len(pts), inside.sum(), len(border), gs.abs().max()))
    assert inside.sum() >= 60 and (~inside).sum() >= 6 and np.isfinite(gs.numpy()).all()
    return {"q%d_grid" % gi: np.int32(gi), "q%d_pose" % gi: pose, "q%d_scale" % gi: np.float64(sc), "q%d_pts" % gi: pts,
            "q%d_phi" % gi: phi.detach().numpy(), "q%d_g" % gi: g.detach().numpy(), "q%d_cot_phi" % gi: cot_phi, "q%d_cot_g" % gi: cot_g,
            "q%d_g_sdf" % gi: gs.numpy()}


def run_pair(r1, r2, side, seed):
    """The handler on one pair; the grid on `side` has samples that require grad.  None: a condition fails, draw again."""
    torch.manual_seed(seed)
    recs, bodies, leaf = (r1, r2), [], None
    for s in range(2):
        if s == side:
            leaf = T(base.GRIDS[int(recs[s]["grid"])], True)
            bodies.append(SDFGrid(T(recs[s]["pose"]), T(recs[s]["scale"]), leaf))
        else:
            bodies.append(base.make(recs[s])[0])
    w = base.Stub(bodies)
    try:
        SDFContactHandler()([w], base.Geom(0), base.Geom(1))
    except RuntimeError as e:      # the hull of tensors that require grad: contacts that span two dimensions are not recorded
        if "requires grad" not in str(e):
            raise
        return None
    b1, b2 = bodies
    with torch.no_grad():
        v1, e1 = b1.get_surface()
        v2, e2 = b2.get_surface()
        ca, ta, pa, oka = base.trace(v1, e1, b2, 0, b1.pos, b2.pos)
        cb, tb, pb, okb = base.trace(v2, e2, b1, 1, b1.pos, b2.pos)
    cand, ctag, ct = np.concatenate([ca, cb]), np.concatenate([ta, tb]), np.concatenate([pa, pb])
    if not (oka and okb) or len(w.contacts) == 0 or len(w.contacts) > 8:
        return None
    if len(cand) > 1:
        p = cand[:, 2:4] - cand[:, 2:4].mean(0)
        sv = np.linalg.svd(p, compute_uv=False)
        if np.any((sv > 1e-6) & (sv < 1e-4)) or int((sv > 1e-5).sum()) > 1:
            return None
        if int((sv > 1e-5).sum()) == 1:
            proj = np.sort(p @ np.linalg.svd(p)[2][0])
            if proj[1] - proj[0] < 1e-7 * float(b1.scale) or proj[-1] - proj[-2] < 1e-7 * float(b1.scale):
                return None
    out = np.stack([base.flat(c[0]).detach().numpy() for c in w.contacts])
    which = [int(np.nonzero((cand == row).all(1))[0][0]) for row in out]
    tag, tpar = ctag[which].reshape(-1, 2), ct[which]
    # direction d walks the edges of body d: the grid is the body queried where d != side
    under_test = tag[:, 0] != side
    if not under_test.any():
        return None
    gout = np.random.default_rng(seed).normal(size=(len(out), 7)) * under_test[:, None]
    loss = sum((base.flat(c[0]) * T(gout[q])).sum() for q, c in enumerate(w.contacts) if under_test[q])
    (gs,) = torch.autograd.grad(loss, [leaf])      # (must not raise: no recorded loss touches the grid's outline)
    if not np.isfinite(gs.numpy()).all() or float(gs.abs().max()) == 0.0:
        return None
    pad = lambda a, n, dt=np.float64: np.concatenate([a, np.zeros((n - len(a),) + a.shape[1:], dt)]).astype(dt)      # noqa: E731
    return dict(kind=np.array([r1["kind"], r2["kind"]], np.int32), pose=np.stack([r1["pose"], r2["pose"]]), prm=np.stack([r1["prm"], r2["prm"]]),
                scale=np.array([r1["scale"], r2["scale"]]), grid=np.array([r1["grid"], r2["grid"]], np.int32), side=np.int32(side),
                count=np.int32(len(out)), out=pad(out, 8), tag=pad(tag, 8, np.int32), tpar=pad(tpar, 8), gout=pad(gout, 8),
                g_sdf=pad(gs.numpy().reshape(-1), NMAX))


def contact_set(rng):
    recs, names, seed = [], [], 5000
    for gi in (1, 2):
        for other in (CIRCLE, RECT, GRID):
            have = tries = 0
            while have < PER_COMBO:
                tries += 1
                assert tries < 20000, (gi, other)
                side = int(rng.integers(0, 2))
                kinds = (GRID, other) if side == 0 else (other, GRID)
                r1, r2 = base.random_pair(rng, kinds[0], kinds[1], True, shallow=True)
                (r1, r2)[side]["grid"] = gi
                if other == GRID:
                    (r1, r2)[1 - side]["grid"] = int(rng.integers(0, 3))
                seed += 1
                rec = run_pair(r1, r2, side, seed)
                if rec is None:
                    continue
                recs.append(rec); names.append("g%d_%d_side%d" % (gi, other, side)); have += 1
                print("%-14s count %d, under test %d, |d sdf| max %.3f, non-zero samples %d" %
                      (names[-1], rec["count"], int((np.abs(rec["gout"]).sum(1) > 0).sum()), np.abs(rec["g_sdf"]).max(), (rec["g_sdf"] != 0).sum()))
    d = {k: np.stack([r[k] for r in recs]) for k in recs[0]}
    d["names"] = np.array(names)
    return d


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    rng = np.random.default_rng(41)
    d = {"eps": np.float64(base.EPS)}
    for gi in (1, 2):
        d.update(query_set(gi, rng))
        d["grid%d" % gi] = base.GRIDS[gi]
    d["grid0"] = base.GRIDS[0]
    d.update(contact_set(rng))
    path = os.path.join(base.GOLDEN, "sdf2d_grid_grad.npz")
    np.savez_compressed(path, **d)
    print("%d pairs -> %s, %d bytes" % (len(d["count"]), path, os.path.getsize(path)))
