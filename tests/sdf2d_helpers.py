"""Shared by the 2-D SDF tests: the goldens of tools/gen_sdf2d_golden.py as kernel inputs, and the comparison of contact sets."""
import os
import types

import numpy as np
import torch

from diffsdfsim_amd.physics2d import sdf_bodies, sdf_contacts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Bounds ("2-D SDF contacts"): the analytic 2-D kernels are held to 1e-12 on tuples, scaled by the
# coordinate magnitude of the scene, and 1e-9 relative on gradients (tests/test_contacts2d_cpu.py); the same here.
TUPLE_TOL, GRAD_TOL = 1e-12, 1e-9
_cache = {}


def _unpack(d):
    """The ragged rows of a contact file (tools/gen_sdf2d_golden.py: pack) as arrays padded to the file's largest counts:
    cand [P, max ncand, 7], cand_tag, out [P, max count, 7], tag, tpar and, in the grad file, gout."""
    n, m, P = d["ncand"], d["count"], len(d["count"])
    c5 = d["cand_rows"]
    cand = np.zeros((P, max(int(n.max()), 1), 7))
    ctag = np.zeros((P, cand.shape[1], 2), np.int32)
    out, tag, tpar = np.zeros((P, max(int(m.max()), 1), 7)), np.zeros((P, max(int(m.max()), 1), 2), np.int32), np.zeros((P, max(int(m.max()), 1)))
    gout = np.zeros_like(out)
    co, ko = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)])
    for p in range(P):
        rows = c5[co[p]:co[p + 1]]
        cand[p, :n[p], 0:4], cand[p, :n[p], 6] = rows[:, 0:4], rows[:, 4]
        cand[p, :n[p], 4:6] = (rows[:, 2:4] + d["pose"][p, 0, 1:]) - d["pose"][p, 1, 1:]      # p2 = p1 + pos1 - pos2
        ctag[p, :n[p]] = d["cand_tag_rows"][co[p]:co[p + 1]]
        keep = d["keep_rows"][ko[p]:ko[p + 1]]
        out[p, :m[p]], tag[p, :m[p]], tpar[p, :m[p]] = cand[p, keep], ctag[p, keep], d["tpar_rows"][ko[p]:ko[p + 1]]
        if "gout_rows" in d:
            gout[p, :m[p]] = d["gout_rows"][ko[p]:ko[p + 1]]
    d.update(cand=cand, cand_tag=ctag, out=out, tag=tag, tpar=tpar)
    if "gout_rows" in d:
        d["gout"] = gout
    return d


def golden(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        _cache[name] = _unpack(d) if "cand_rows" in d else d
    return _cache[name]


def grid_sources(g):
    """The three sample arrays of the contact goldens as sources of a GridTable (samples, differences, outline)."""
    out = []
    for i in range(3):
        sdf = torch.tensor(g["grid%d" % i], dtype=torch.float64)
        verts, edges = sdf_bodies.marching_squares(sdf)
        out.append(types.SimpleNamespace(sdf=sdf, sdf_grads=sdf_bodies.central_differences(sdf), unit_verts=verts, edges=edges))
    return out


def table(device="cpu"):
    key = ("table", str(device))
    if key not in _cache:
        _cache[key] = sdf_contacts.GridTable(grid_sources(golden("sdf2d_contacts")), device)
    return _cache[key]


def inputs(g, idx, device="cpu", grad=False):
    """Pairs idx of a golden file as the arguments of sdf_contacts2d."""
    f = lambda a: torch.tensor(np.ascontiguousarray(np.moveaxis(a[idx], 0, 1)), dtype=torch.float64, device=device).requires_grad_(grad)   # noqa: E731
    i = lambda a: torch.tensor(np.ascontiguousarray(a[idx].T), dtype=torch.int32, device=device)      # noqa: E731
    return dict(pose=f(g["pose"]), prm=f(g["prm"]), scale=f(g["scale"]), kind=i(g["kind"]), grid_id=i(g["grid"]), grids=table(device))


def magnitude(g, p):
    """Coordinate magnitude of pair p: the largest position or extent in it."""
    return max(1.0, np.abs(g["pose"][p, :, 1:]).max() + g["scale"][p].max())


def by_tag(rows, tags, n):
    order = sorted(range(n), key=lambda q: (int(tags[q, 0]), int(tags[q, 1])))
    return rows[order], tags[order]


def compare_contacts(g, idx, out, count, tag, ncand=None, cand=None, cand_tag=None):
    """Counts equal, tuples equal as sets sorted by (direction, edge), the contacts before thinning equal in order.  Returns
    the largest tuple error over the coordinate magnitude."""
    out, count, tag = (x.detach().cpu().numpy() for x in (out, count, tag))
    worst = 0.0
    for k, p in enumerate(idx):
        assert count[k] == g["count"][p], (p, g["names"][p], count[k], g["count"][p])
        n = int(count[k])
        got, gt = by_tag(out[k], tag[k], n)
        want, wt = by_tag(g["out"][p], g["tag"][p], n)
        assert np.array_equal(gt, wt), (p, g["names"][p], gt.tolist(), wt.tolist())
        err = np.abs(got - want).max() / magnitude(g, p) if n else 0.0
        assert err <= TUPLE_TOL, (p, g["names"][p], err)
        worst = max(worst, err)
        assert np.all(out[k, n:] == 0.0)
        if ncand is not None:
            m = int(g["ncand"][p])
            assert int(ncand[k]) == m, (p, int(ncand[k]), m)
            assert np.array_equal(cand_tag[k, :m].cpu().numpy(), g["cand_tag"][p, :m]), p
            err = np.abs(cand[k, :m].cpu().numpy() - g["cand"][p, :m]).max() / magnitude(g, p) if m else 0.0
            assert err <= TUPLE_TOL, (p, err)
            worst = max(worst, err)
    return worst


def gout_in_kernel_order(g, idx, count, tag):
    """The recorded upstream gradient, row q of which belongs to the reference's q-th contact, in the kernel's contact order."""
    tg, cnt = tag.detach().cpu().numpy(), count.detach().cpu().numpy()
    gout = np.zeros((len(idx), tg.shape[1], 7))
    for k, p in enumerate(idx):
        for q in range(int(g["count"][p])):
            mine = [r for r in range(int(cnt[k])) if tuple(tg[k, r]) == tuple(g["tag"][p, q])]
            gout[k, mine[0]] = g["gout"][p, q]
    return gout


def compare_gradients(g, idx, a, nontrivial=True):
    """The gradients left on the leaves of `a` against the reference's autograd; every leaf non-trivial somewhere (unless the
    launch is too small to hold a pair of every kind)."""
    worst = 0.0
    for key, ref in (("pose", "g_pose"), ("prm", "g_prm"), ("scale", "g_scale")):
        got = np.moveaxis(a[key].grad.detach().cpu().numpy(), 0, 1)
        want = g[ref][idx]
        assert not nontrivial or np.abs(got).max() > 0.1, key
        for k in range(len(idx)):
            norm = max(1.0, np.abs(g["g_pose"][idx[k]]).max(), np.abs(g["g_prm"][idx[k]]).max(), np.abs(g["g_scale"][idx[k]]).max())
            err = np.abs(got[k] - want[k]).max() / norm
            assert err <= GRAD_TOL, (key, idx[k], g["names"][idx[k]], err, got[k], want[k])
            worst = max(worst, err)
    return worst
