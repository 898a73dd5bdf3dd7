"""The dense LCP (dss_lcp_dense_forward / _backward) at its dispatch seams, with mixed statuses in one launch and under every
stop rule: inputs, preconditions and assertions, stated once on numpy arrays.  test_emu_lcp_dense_seams.py runs them on the CPU
emulation of the kernels, test_lcp_dense_seams_gpu.py on the device.

The entry picks one of three code paths by size (csrc/lcp_dense.hip, csrc/lcp_dense_group.hip):
  group   nz, nineq, neq <= 8: eight systems per wavefront, everything in registers, Q and A Q^-1 A^T factored unpivoted
  wave    one wavefront per system; its workspace in LDS while lds_bytes + ws_bytes_per_system <= 30 KB
          ((12, 30, 6): 29 632 B, the last), in the caller's global workspace above ((12, 31, 6): 30 928 B, the first)
  refused staged vectors above 64 KB of LDS (nz = 682): DSS_E_UNSUPPORTED

A backend is anything with `lib` (the bound library), from_numpy, to_numpy, ptr and stream (diffsdfsim_amd.engine.TorchBackend,
tests/emu/emu.EmuBackend).  Every call goes through the raw C ABI with each output array one row too long and the whole of it
filled with a sentinel: a row that was not written, and a write past row B, both show.

References: oracle/lcp_oracle (pinned to the reference's goldens) and a numpy.longdouble evaluation of the LCP residuals from
the data.  Tolerances are the ones of tests/test_lcp_dense_gpu.py: z 1e-9, slack 1e-6, gradients 1e-7 relative to each array's
largest entry (from the oracle's primal and dual), status and iteration counts equal.  ONE deviation, in assert_grads: where
nz == neq the arrays dQ, dp, dG, dh and dF are zero in exact arithmetic and hold rounding noise in the oracle too; those five,
at those shapes only, are held to 1e-7 of the case's largest gradient instead of 1e-7 of their own noise.

Seeds (chosen on the CPU so that the stated preconditions hold and the oracle against the emulated kernels needs no tie excuse):
  A  random_lcp(SEAM_SEED + nz + nineq + neq, B, ...), SEAM_SEEDS[(64,64,6)]; (8,8,8) and (64,64,6) have systems whose first T
     takes a row exchange
  B  random_lcp(EMBED_SEED + nz + nineq + neq, 16, ...)
  D  random_lcp(MIXED_SEED[shape], ...)     E  random_lcp(STOP_SEED[shape], ...)
"""
import functools

import numpy as np

from helpers import random_lcp, rel
from oracle import lcp_oracle as O

FILL = -7.03125e77            # what every double output holds before a call (no kernel result equals it)
IFILL = 0x5A5A5A5A            # the same for iters / status
WS_FILL = 0xA5                # workspace bytes

E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3

SEAM_SEED, EMBED_SEED = 4100, 5200
SEAM_SEEDS = {(64, 64, 6): 4384}      # the default seed has no row exchange in its first T
MIXED_SEED = {(6, 4, 3): 7401, (12, 10, 6): 7403}
STOP_SEED = {(6, 8, 3): 8501, (12, 31, 6): 8503}


# ---- 1. the guarded calls --------------------------------------------------------------------------------------------------
def _filled(shape, dtype=np.float64):
    return np.full(shape, FILL if dtype == np.float64 else IFILL, dtype)


def _up(be, a):
    """-> (device handle or None, pointer or None); an empty array is a null pointer."""
    if a is None or a.size == 0:
        return None, None
    t = be.from_numpy(np.ascontiguousarray(a))
    return t, be.ptr(t)


def _dims(G, A):
    B, nineq, nz = G.shape
    return B, nz, nineq, (A.shape[1] if A is not None and A.size else 0)


class Result(dict):
    __getattr__ = dict.__getitem__


def _collect(be, rc, host, dev, B, ws):
    """Read every output back whole; on success split the B rows from the guard row and assert the guard."""
    full = {k: (be.to_numpy(dev[k]) if dev[k] is not None else host[k]) for k in host}
    r = Result(rc=rc, full=full)
    if ws is not None:
        w = be.to_numpy(ws[0])
        assert (w[ws[1]:] == WS_FILL).all(), "bytes written behind the workspace"
        r["ws_touched"] = bool((w[:ws[1]] != WS_FILL).any())
    for k, a in full.items():
        fill = FILL if a.dtype == np.float64 else IFILL
        if rc != 0:
            assert (a == fill).all(), "%s written although the call returned %d" % (k, rc)
        else:
            assert (a[B:] == fill).all(), "%s: written past row B = %d" % (k, B)
            r[k] = a[:B]
    return r


def _workspace(be, B, nz, nineq, neq, short=0):
    n = be.lib.dss_lcp_dense_workspace_bytes(B, nz, nineq, neq)
    t = be.from_numpy(np.full(n + 256, WS_FILL, np.uint8))
    return (t, n), be.ptr(t), n - short


def forward(be, ops, eps=1e-12, nil=3, max_iter=20, check_spd=True, dims=None, ws_short=0, null=()):
    """dss_lcp_dense_forward on guarded outputs.  dims = (B, nz, nineq, neq) to pass other sizes than the arrays have (the
    outputs are allocated for the larger of the two), ws_short: bytes taken off workspace_bytes, null: operands passed as NULL."""
    Q, p, G, h, A, b, F = ops
    aB, anz, anineq, aneq = _dims(G, A)
    B, nz, nineq, neq = dims or (aB, anz, anineq, aneq)
    rows = max(aB, B, 1) + 1
    host = dict(zhat=_filled((rows, max(anz, nz))), lam=_filled((rows, max(anineq, nineq, 1))), slack=_filled((rows, max(anineq, nineq, 1))),
                nu=_filled((rows, max(aneq, neq))), iters=_filled((rows,), np.int32), status=_filled((rows,), np.int32))
    ins = [None if n in null else _up(be, x) for n, x in zip("QpGhAbF", (Q, p, G, h, A, b, F))]
    dev, ptr = {}, {}
    for k, a in host.items():
        dev[k], ptr[k] = _up(be, a)
    ws, wptr, wbytes = _workspace(be, max(B, 1), max(nz, 1), max(nineq, 1), max(neq, 0), ws_short)
    rc = be.lib.dss_lcp_dense_forward(*[i[1] if i else None for i in ins], B, nz, nineq, neq, eps, nil, max_iter, int(check_spd),
                                      ptr["zhat"], ptr["lam"], ptr["slack"], ptr["nu"], ptr["iters"], ptr["status"], wptr, wbytes,
                                      be.stream())
    return _collect(be, rc, host, dev, B, ws)


def backward(be, Q, G, A, F, zhat, lam, slack, nu, dl, dims=None, ws_short=0, null=()):
    aB, anz, anineq, aneq = _dims(G, A)
    B, nz, nineq, neq = dims or (aB, anz, anineq, aneq)
    rows = max(aB, B, 1) + 1
    mz, mi, me = max(anz, nz), max(anineq, nineq, 1), max(aneq, neq)
    host = dict(dQ=_filled((rows, mz, mz)), dp=_filled((rows, mz)), dG=_filled((rows, mi, mz)), dh=_filled((rows, mi)),
                dA=_filled((rows, me, mz)), db=_filled((rows, me)), dF=_filled((rows, mi, mi)))
    ins = {n: (None if n in null else _up(be, x)) for n, x in
           zip(("Q", "G", "A", "F", "zhat", "lam", "slack", "nu", "dl"), (Q, G, A, F, zhat, lam, slack, nu, dl))}
    dev, ptr = {}, {}
    for k, a in host.items():
        dev[k], ptr[k] = _up(be, a)
    ws, wptr, wbytes = _workspace(be, max(B, 1), max(nz, 1), max(nineq, 1), max(neq, 0), ws_short)
    ip = lambda n: ins[n][1] if ins[n] else None
    rc = be.lib.dss_lcp_dense_backward(ip("Q"), ip("G"), ip("A"), ip("F"), B, nz, nineq, neq, ip("zhat"), ip("lam"), ip("slack"),
                                       ip("nu"), ip("dl"), ptr["dQ"], ptr["dp"], ptr["dG"], ptr["dh"], ptr["dA"], ptr["db"], ptr["dF"],
                                       wptr, wbytes, be.stream())
    return _collect(be, rc, host, dev, B, ws)


GRADS = ("dQ", "dp", "dG", "dh", "dA", "db", "dF")


# ---- 2. shared assertions --------------------------------------------------------------------------------------------------
def tie_at(hist, it_a, it_b, nil):
    """The oracle's residual history shows a tie where the two counts part: two successive residuals among those that decide
    the earlier stop differ by less than 1e-12 relative."""
    last = min(it_a, it_b)
    h = np.asarray(hist)[max(0, last - nil - 1): last + 1]
    return any(abs(a - b) < 1e-12 * max(abs(a), abs(b)) for a, b in zip(h[:-1], h[1:]))


def assert_counts(it, ito, ops, kw, what):
    """Iteration counts equal -- or ONE system of the case off by one at a residual tie, shown from the oracle's history.
    -> mask of the systems whose counts agree (the others' iterates are another iteration's)."""
    same = it == ito
    bad = np.nonzero(~same)[0]
    if bad.size:
        assert bad.size == 1 and abs(int(it[bad[0]]) - int(ito[bad[0]])) == 1, (what, it, ito)
        k = int(bad[0])
        hist = O.residual_history(*[x[k:k + 1] for x in ops], **kw)[0]
        print("%s: system %d stops at %d, the oracle at %d; the oracle's residuals %r" % (what, k, it[k], ito[k], list(hist)))
        assert tie_at(hist, int(it[k]), int(ito[k]), kw.get("not_improved_lim", 3)), (what, k, list(hist))
    return same


def check_forward(be, ops, what, **kw):
    """One launch against the oracle called with the same arguments -> (device result, oracle outputs)."""
    okw = dict(eps=kw.get("eps", 1e-12), not_improved_lim=kw.get("nil", 3), max_iter=kw.get("max_iter", 20),
               check_spd=kw.get("check_spd", True))
    r = forward(be, ops, **kw)
    assert r.rc == 0, (what, r.rc)
    ref = O.forward(*ops, **okw)
    zo, lo, so, nuo, ito, sto = ref
    assert (r.status == sto).all(), (what, r.status, sto)
    same = assert_counts(r.iters, ito, ops, okw, what)
    ez, es = rel(r.zhat[same], zo[same]), rel(r.slack[same], so[same])
    print("%s: z %.2e slack %.2e" % (what, ez, es))
    assert ez < 1e-9 and es < 1e-6, (what, ez, es)
    return r, ref


ZERO_WHEN_SQUARE = ("dQ", "dp", "dG", "dh", "dF")


def assert_grads(got, want, what, nz, neq):
    """Every gradient array within 1e-7 of the reference's, relative to the array's largest entry.  nz == neq only: x is fixed
    by A x = b, so dx = 0 and dlam = 0 exactly, only dA and db are non-zero, and ZERO_WHEN_SQUARE hold rounding noise on both
    sides, which has no digits to compare; those are held to 1e-7 of the largest gradient of the case (dA, db) instead."""
    gmax = max(np.abs(w).max() for w in want if w.size)
    for name, w in zip(GRADS, want):
        if not w.size:
            continue
        scale = gmax if (nz == neq and name in ZERO_WHEN_SQUARE) else np.abs(w).max()
        e = float(np.abs(got[name] - w).max() / max(scale, 1e-300))
        assert e < 1e-7, (what, name, e)


def check_backward(be, ops, ref, what, seed=7):
    Q, p, G, h, A, b, F = ops
    zo, lo, so, nuo = ref[:4]
    dl = np.random.default_rng(seed).standard_normal(zo.shape)
    want = O.backward(Q, G, A, F, zo, lo, so, nuo, dl)
    r = backward(be, Q, G, A, F, zo, lo, so, nuo, dl)
    assert r.rc == 0, (what, r.rc)
    assert_grads(r, want, what, Q.shape[1], A.shape[1])
    return r, want


# ---- 3. A: size seams ------------------------------------------------------------------------------------------------------
SEAMS = [(9, 8, 8, 8), (17, 8, 8, 8), (3, 8, 1, 0), (9, 1, 1, 0), (17, 1, 1, 0), (9, 9, 8, 3), (17, 9, 8, 3), (3, 8, 9, 3), (3, 10, 8, 9),
         (3, 12, 30, 6), (3, 12, 31, 6), (3, 63, 65, 0), (3, 64, 64, 6), (3, 65, 63, 1), (3, 16, 129, 4)]
PIVOTED = [(8, 8, 8), (64, 64, 6)]      # their first T must take a row exchange in some system


def seam_ops(B, nz, nineq, neq):
    return random_lcp(SEAM_SEEDS.get((nz, nineq, neq), SEAM_SEED + nz + nineq + neq), B, nz, nineq, neq)


def first_T(ops):
    """T = R + diag(s / z) of iteration 0, per system (batch.py:413-520): R in numpy, s and z the oracle's initial point
    (what a run of one iteration returns)."""
    Q, p, G, h, A, b, F = ops
    _, lam, slack, _, _, _ = O.forward(*ops, max_iter=1)
    out = []
    for k in range(len(Q)):
        Qi = np.linalg.inv(Q[k])
        R = G[k] @ Qi @ G[k].T + F[k]
        if A.shape[1]:
            GA = G[k] @ Qi @ A[k].T
            R = R - GA @ np.linalg.solve(A[k] @ Qi @ A[k].T, GA.T)
        out.append(R + np.diag(slack[k] / lam[k]))
    return out


def rows_exchanged(T):
    from scipy.linalg import lu
    P = lu(T)[0]
    return not np.array_equal(P, np.eye(len(T)))


def lds_need(nz, nineq, neq):
    """Staged vectors + workspace of one system in bytes, as csrc/lcp_dense.hip lays them out (lds_bytes + ws_bytes_per_system)."""
    lds = ((neq + nineq + 12 * nz + 4 * (neq + 1) + 8 + 1) & ~1) * 8
    dbl = nz * nz + 2 * nineq * nineq + neq * neq + 2 * neq * nineq + nz * nineq + nz * neq + 2 * nineq * neq + 10 * nineq + 8
    return lds + ((dbl * 8 + (nz + neq + nineq + 8) * 4 + 255) & ~255)


def expected_path(nz, nineq, neq):
    # the copy of the kernel's layout above is pinned to the two figures DESIGN.md section 5 states for the switch
    assert lds_need(12, 30, 6) == 29632 and lds_need(12, 31, 6) == 30928
    if nz <= 8 and nineq <= 8 and neq <= 8:
        return "group"
    return "lds" if lds_need(nz, nineq, neq) <= 30 * 1024 else "global"


def check_dispatch_sizes(fits):
    """fits(nz, nineq, neq): the size test of the dispatch itself (the emulator build exports it; the results cannot show which
    kernel ran, both are right).  Eight on every axis is the group kernel's, nine on any one axis is not."""
    for shape in [(8, 8, 8), (8, 1, 0), (1, 1, 0), (8, 8, 0), (1, 8, 8)] + [s for s in EMBED]:
        assert fits(*shape), shape
    for shape in [(9, 8, 8), (8, 9, 8), (8, 8, 9), (9, 8, 3), (8, 9, 3), (10, 8, 9), (9, 1, 0)] + [(nz + 1, ni, ne) for nz, ni, ne in EMBED if nz == 8]:
        assert not fits(*shape), shape


def check_seam(be, B, nz, nineq, neq):
    ops = seam_ops(B, nz, nineq, neq)
    what = "seam (%d,%d,%d) B=%d" % (nz, nineq, neq, B)
    if (nz, nineq, neq) in PIVOTED:
        n = sum(rows_exchanged(T) for T in first_T(ops))
        print("%s: %d systems whose first T takes a row exchange" % (what, n))
        assert n >= 1, what
    r, ref = check_forward(be, ops, what)
    # the global workspace is written exactly where the size is past the LDS budget: this pins the switch itself
    assert r.ws_touched == (expected_path(nz, nineq, neq) == "global"), (what, expected_path(nz, nineq, neq), r.ws_touched)
    check_backward(be, ops, ref, what)


# ---- 4. B: the group kernel against the wave kernel, by embedding ----------------------------------------------------------
EMBED = [(6, 4, 3), (8, 8, 5), (8, 8, 8)]


def embed(ops):
    """One decoupled unknown appended: Q' = diag(Q, 1), p' = (p, 0), a zero column in G and A.  It stays exactly 0 and
    every residual norm is unchanged, so both solves take the same iterations -- on different kernels (nz + 1 >= 9)."""
    Q, p, G, h, A, b, F = ops
    B, nz = p.shape
    Q2 = np.zeros((B, nz + 1, nz + 1)); Q2[:, :nz, :nz] = Q; Q2[:, nz, nz] = 1.0
    pad = lambda M: np.concatenate([M, np.zeros(M.shape[:-1] + (1,))], axis=-1)
    return Q2, pad(p), pad(G), h, pad(A), b, F


def check_embedding(be, nz, nineq, neq):
    ops = random_lcp(EMBED_SEED + nz + nineq + neq, 16, nz, nineq, neq)
    ops2 = embed(ops)
    what = "embed (%d,%d,%d)" % (nz, nineq, neq)
    g, w = forward(be, ops), forward(be, ops2)
    assert g.rc == 0 and w.rc == 0 and not g.ws_touched
    assert (g.status == w.status).all(), (g.status, w.status)
    okw = dict(eps=1e-12, not_improved_lim=3, max_iter=20, check_spd=True)
    same = assert_counts(w.iters, g.iters, ops, okw, what)
    assert (w.zhat[:, nz] == 0.0).all(), w.zhat[:, nz]
    ez, es = rel(w.zhat[same][:, :nz], g.zhat[same]), rel(w.slack[same], g.slack[same])
    print("%s: group vs wave z %.2e slack %.2e" % (what, ez, es))
    assert ez < 1e-9 and es < 1e-6, (what, ez, es)
    # backward from the oracle's primal and dual of the small system
    zo, lo, so, nuo, _, _ = O.forward(*ops)
    dl = np.random.default_rng(11).standard_normal((16, nz))
    pad = lambda M: np.concatenate([M, np.zeros(M.shape[:-1] + (1,))], axis=-1)
    bg = backward(be, ops[0], ops[2], ops[4], ops[6], zo, lo, so, nuo, dl)
    bw = backward(be, ops2[0], ops2[2], ops2[4], ops2[6], pad(zo), lo, so, nuo, pad(dl))
    assert bg.rc == 0 and bw.rc == 0
    lead = dict(dQ=np.s_[:, :nz, :nz], dG=np.s_[:, :, :nz], dA=np.s_[:, :, :nz], dp=np.s_[:, :nz], dh=np.s_[:], db=np.s_[:], dF=np.s_[:])
    assert_grads({name: bw[name][lead[name]] for name in GRADS}, [bg[name] for name in GRADS], what, nz, neq)


# ---- C: ill-scaled SPD Q on the group path ----------------------------------------------------------------------------------
ILL = [(6, 8, 3), (8, 8, 8)]
CONDS = [1e4, 1e8, 1e10]
ILL_SEED = 6340      # every system of both shapes has a solution at every condition number (oracle status 0)


def ill_scaled(seed, B, nz, nineq, neq, cond):
    """random_lcp with Q = D L L^T D + D^2, D diagonal and log-spaced from 1 to sqrt(cond): cond(Q) ~ cond."""
    Q, p, G, h, A, b, F = random_lcp(seed, B, nz, nineq, neq)
    L = np.random.default_rng(seed + 1).standard_normal((B, nz, nz))
    D = np.logspace(0.0, 0.5 * np.log10(cond), nz)
    Q = D[None, :, None] * (L @ L.transpose(0, 2, 1)) * D[None, None, :] + np.diag(D * D)[None]
    return Q, p, G, h, A, b, F


def residual_norms(ops, x, z, s, y):
    """-> norms [4][B]: |rx|, |rz|, |ry|, nineq mu of an iterate, evaluated from the data in numpy.longdouble (batch.py:117-131;
    their sum is the residual the solver minimises and stops on), and scale [B]: the operand scale, the largest magnitude among
    the terms those residuals sum (|Q||x|, |p|, |G^T||z|, |A^T||y|, |G||x|, |s|, |h|, |F||z|, |A||x|, |b|)."""
    LD = np.longdouble
    Q, p, G, h, A, b, F = (np.asarray(a, LD) for a in ops)
    x, z, s, y = (np.asarray(a, LD) for a in (x, z, s, y))
    mv = lambda M, v: np.einsum("bij,bj->bi", M, v)
    mtv = lambda M, v: np.einsum("bij,bi->bj", M, v)
    n2 = lambda v: np.sqrt((v * v).sum(1))
    rx = mv(Q, x) + p + mtv(G, z)
    rz = mv(G, x) + s - h - mv(F, z)
    terms = [mv(np.abs(Q), np.abs(x)), p, mtv(np.abs(G), np.abs(z)), mv(np.abs(G), np.abs(x)), s, h, mv(np.abs(F), np.abs(z))]
    ry = np.zeros((len(x), 0), LD)
    if A.shape[1]:
        rx = rx + mtv(A, y)
        ry = mv(A, x) - b
        terms += [mtv(np.abs(A), np.abs(y)), mv(np.abs(A), np.abs(x)), b]
    norms = np.stack([n2(rx), n2(rz), n2(ry), np.abs((s * z).sum(1))])
    return norms, np.max([np.abs(t).max(1) for t in terms], axis=0)


def check_ill_scaled(be, nz, nineq, neq, cond):
    """The group kernel (unpivoted LU of Q and A Q^-1 A^T, explicit inverses in the forward) against the oracle (pivoted LU
    solves) on ill-scaled Q: the residual of the returned iterate <= 4 x the oracle's + 1e-12 x the operand scale, per system.

    "The residual" is the sum of the four norms, the quantity the solver minimises, keeps its best iterate by and stops on.  The
    four are printed but not bounded one by one: once rounding in Q x (|Q||x| eps, 1e-11 .. 1e-7 here) is above eps = 1e-12 the
    run ends on the not-improved rule and the best iterate is picked by that noise; which of two iterates with the same sum it
    is moves nineq mu by 1e3 (the last steps shrink mu by 1 - 0.999 each) between two correct solvers.
    -> the worst device / oracle ratio of the sums, for the record in DESIGN.md section 5."""
    ops = ill_scaled(ILL_SEED, 8, nz, nineq, neq, cond)
    what = "ill-scaled (%d,%d,%d) cond %.0e" % (nz, nineq, neq, cond)
    c = np.linalg.cond(ops[0])
    assert (c > cond / 30).all() and (c < cond * 30).all(), (what, c)
    r = forward(be, ops)
    assert r.rc == 0 and not r.ws_touched
    zo, lo, so, nuo, ito, sto = O.forward(*ops)
    assert (sto == 0).all(), (what, sto)      # every system has a solution
    assert (r.status == sto).all(), (what, r.status, sto)
    nd, scale = residual_norms(ops, r.zhat, r.lam, r.slack, r.nu)
    no, _ = residual_norms(ops, zo, lo, so, nuo)
    td, to = nd.sum(0), no.sum(0)
    ratio = float((td / to).max())
    f = lambda v: "[" + " ".join("%.1e" % float(t) for t in v) + "]"
    print("%s: cond(Q) %.1e..%.1e, worst over the batch of |rx| |rz| |ry| nineq mu: device %s oracle %s; sums: device %s oracle %s; "
          "worst ratio of the sums %.3g; iterations device %s oracle %s; z vs oracle %.1e"
          % (what, c.min(), c.max(), f(nd.max(1)), f(no.max(1)), f(td), f(to), ratio, r.iters.tolist(), ito.tolist(), rel(r.zhat, zo)))
    assert (td <= 4 * to + np.longdouble(1e-12) * scale).all(), (what, ratio)
    return ratio


# ---- 5. D: mixed statuses in one launch ------------------------------------------------------------------------------------
MIXED = [(13, 6, 4, 3), (5, 12, 10, 6)]
SICK_Q, SICK_G = 1, 4        # "system 2" and "system 5" of the batch, counted from one


@functools.lru_cache(maxsize=None)
def mixed_batches(B, nz, nineq, neq):
    """-> healthy, not_spd (system SICK_Q: one negative eigenvalue; system SICK_G: contradictory inequalities g x <= -1 and
    -g x <= -1 with F = 0, as in the infeasible golden), singular (system SICK_Q: a zero row and column instead)."""
    healthy = random_lcp(MIXED_SEED[(nz, nineq, neq)], B, nz, nineq, neq)

    def sick(kind):
        Q, p, G, h, A, b, F = (a.copy() for a in healthy)
        m = nineq // 2
        G[SICK_G, m:2 * m] = -G[SICK_G, :m]; h[SICK_G] = -1.0; F[SICK_G] = 0.0
        if kind == "not_spd":
            w, V = np.linalg.eigh(Q[SICK_Q])
            Q[SICK_Q] -= (w[0] + 1.0) * np.outer(V[:, 0], V[:, 0])
            Q[SICK_Q] = 0.5 * (Q[SICK_Q] + Q[SICK_Q].T)
        else:
            Q[SICK_Q, 2, :] = 0.0; Q[SICK_Q, :, 2] = 0.0
        return Q, p, G, h, A, b, F
    return healthy, sick("not_spd"), sick("singular")


def check_mixed(be, B, nz, nineq, neq, kind):
    healthy, not_spd, singular = mixed_batches(B, nz, nineq, neq)
    ops, check_spd, want = (not_spd, True, 1) if kind == "not_spd" else (singular, False, 2)
    what = "mixed %s (%d,%d,%d) B=%d" % (kind, nz, nineq, neq, B)
    okw = dict(eps=1e-12, not_improved_lim=3, max_iter=20, check_spd=check_spd)
    # per-system oracle runs: the statuses are what the case says, and the healthy systems take >= 3 distinct counts
    one = [O.forward(*[x[k:k + 1] for x in ops], **okw) for k in range(B)]
    zo, lo, so, nuo = (np.concatenate([o[j] for o in one]) for j in range(4))
    ito, sto = (np.concatenate([o[j] for o in one]) for j in (4, 5))
    ok = np.ones(B, bool); ok[[SICK_Q, SICK_G]] = False
    assert sto[SICK_Q] == want and sto[SICK_G] == 4 and (sto[ok] == 0).all(), (what, sto)
    assert len(set(ito[ok])) >= 3, (what, ito)
    r = forward(be, ops, check_spd=check_spd)
    base = forward(be, healthy, check_spd=check_spd)
    assert r.rc == 0 and base.rc == 0
    print("%s: status %s iterations %s (oracle %s)" % (what, list(r.status), list(r.iters), list(ito)))
    assert (r.status == sto).all(), (what, r.status, sto)
    same = assert_counts(r.iters, ito, ops, okw, what)
    assert same[SICK_Q] and r.iters[SICK_Q] == 0 and (r.zhat[SICK_Q] == 0.0).all()
    # lam, slack, nu of a system whose Q is refused are not written (include/diffsdfsim_hip.h)
    for k in ("lam", "slack", "nu"):
        assert (r[k][SICK_Q] == FILL).all(), (what, k, r[k][SICK_Q])
    # a healthy system is the same, bit for bit, whoever its neighbours are
    for k in ("zhat", "lam", "slack", "nu", "iters", "status"):
        assert np.array_equal(r[k][ok], base[k][ok]), (what, k)
    live = ok & same
    assert rel(r.zhat[live], zo[live]) < 1e-9 and rel(r.slack[live], so[live]) < 1e-6 and rel(r.lam[live], lo[live]) < 1e-7
    if same[SICK_G]:      # the infeasible system: the same best iterate as the oracle's
        assert rel(r.zhat[SICK_G], zo[SICK_G]) < 1e-9


def mixed_for_function(kind):
    """Operands for LCPFunction with statuses {1, 4} ('not_spd'), {2, 4} ('singular': call with check_Q_spd=False) or {4}
    alone ('inaccurate') in one batch."""
    healthy, not_spd, singular = mixed_batches(13, 6, 4, 3)
    if kind == "inaccurate":
        ops = [a.copy() for a in not_spd]
        ops[0][SICK_Q] = healthy[0][SICK_Q]
        return tuple(ops)
    return not_spd if kind == "not_spd" else singular


# ---- 6. E: stop rules ------------------------------------------------------------------------------------------------------
STOPS = [(16, 6, 8, 3), (4, 12, 31, 6)]
RULES = [(1e-12, 3, 20), (1e-6, 3, 20), (1e-2, 3, 20), (1e-12, 1, 20), (1e-12, 3, 1), (1e-12, 3, 2), (1e-12, 3, 5)]      # eps, nil, max_iter


def stop_ops(B, nz, nineq, neq):
    return random_lcp(STOP_SEED[(nz, nineq, neq)], B, nz, nineq, neq)


def check_stop(be, B, nz, nineq, neq, eps, nil, max_iter):
    ops = stop_ops(B, nz, nineq, neq)
    what = "stop (%d,%d,%d) eps %g nil %d max_iter %d" % (nz, nineq, neq, eps, nil, max_iter)
    r, ref = check_forward(be, ops, what, eps=eps, nil=nil, max_iter=max_iter)
    ito = ref[4]
    hist = O.residual_history(*ops, eps=eps, not_improved_lim=nil, max_iter=max_iter)
    if eps == 1e-2:
        assert 2 * (ito < max_iter).sum() >= B, (what, ito)
    if nil == 1:
        # stopped by the not-improved rule: before max_iter, with the best residual still >= eps; the iteration that stops
        # is then not the best one, so the iterate returned is at least one iteration old
        old = [k for k in range(B) if ito[k] < max_iter and hist[k].min() >= eps and int(np.argmin(hist[k])) < ito[k]]
        print("%s: systems stopped by the not-improved rule %s" % (what, old))
        assert old, (what, ito)
    if max_iter == 5:
        cut = [k for k in range(B) if ito[k] == max_iter and int(np.argmin(hist[k])) < max_iter - 1]
        print("%s: systems cut by max_iter whose best iterate is not the last %s" % (what, cut))
        # the wave kernel stores on every improvement: its cut run must hold such a system (seed chosen so).  The group kernel's
        # batch has none at this seed; its "best, not last" is the nil = 1 run above, which asserts one.
        assert cut or (nz, nineq, neq) != (12, 31, 6), (what, ito)


def check_max_iter_zero(be, B, nz, nineq, neq):
    """No iterate is evaluated, so there is none to return: DSS_E_BADARG, nothing written (include/diffsdfsim_hip.h)."""
    r = forward(be, stop_ops(B, nz, nineq, neq), max_iter=0)
    assert r.rc == E_BADARG, r.rc


# ---- 7. F: argument errors and the largest size ----------------------------------------------------------------------------
def check_argument_errors(be):
    ops = random_lcp(3, 2, 6, 4, 3)
    fw = lambda **kw: forward(be, ops, **kw).rc
    zo, lo, so, nuo, _, _ = O.forward(*ops)
    dl = np.ones_like(zo)
    bw = lambda **kw: backward(be, ops[0], ops[2], ops[4], ops[6], zo, lo, so, nuo, dl, **kw).rc
    assert fw() == 0 and bw() == 0
    assert fw(ws_short=1) == E_WORKSPACE and bw(ws_short=1) == E_WORKSPACE
    assert fw(dims=(0, 6, 4, 3)) == E_BADARG and bw(dims=(0, 6, 4, 3)) == E_BADARG
    assert fw(dims=(2, 6, 0, 3)) == E_BADARG and bw(dims=(2, 6, 0, 3)) == E_BADARG
    assert fw(null=("A",)) == E_BADARG and bw(null=("A",)) == E_BADARG
    # the wave path too (the checks come before the dispatch, the workspace is what that path really uses)
    big = random_lcp(4, 2, 12, 31, 6)
    assert forward(be, big, ws_short=1).rc == E_WORKSPACE and forward(be, big, null=("A",)).rc == E_BADARG


def spd_system(seed, nz, nineq):
    """One well-conditioned system with no equalities: Q = I + L L^T / nz."""
    r = np.random.default_rng(seed)
    L = r.standard_normal((1, nz, nz))
    Q = np.eye(nz)[None] + L @ L.transpose(0, 2, 1) / nz
    return Q, r.standard_normal((1, nz)), r.standard_normal((1, nineq, nz)), r.random((1, nineq)), np.zeros((1, 0, nz)), np.zeros((1, 0)), \
        np.zeros((1, nineq, nineq))


def check_refused_size(be):
    """nz = 682: the staged vectors of a system need 65 584 B of LDS, more than the 64 KB a workgroup may ask for."""
    ops = spd_system(1, 682, 1)
    assert forward(be, ops).rc == E_UNSUPPORTED
    z = np.zeros((1, 682)); one = np.ones((1, 1))
    assert backward(be, ops[0], ops[2], ops[4], ops[6], z, one, one, np.zeros((1, 0)), z).rc == E_UNSUPPORTED


def check_largest_size(be, nz):
    ops = spd_system(2, nz, 2)
    check_forward(be, ops, "largest nz = %d" % nz, max_iter=3)
