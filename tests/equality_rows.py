"""Contact LCP problems with any block of unit equality rows (shared by test_emu_lcp_contact.py and test_lcp_contact_gpu.py).

`structured.random_problem` draws either no equality rows or the six that pin body 0.  The constraint classes of physics3d give
more: XConstraint / YConstraint / ZConstraint (one row), RotConstraint3D (three), TotalConstraint3D (six) on any body, several of
them in one world, or none.  Every one of their rows is a unit row of the body's six velocities (three angular, three linear)."""
import numpy as np

import structured as S


def with_unit_rows(P, joints, seed):
    """P with A, bvec and neq replaced: `joints` = [(body, rows)], rows indexing that body's six velocities, one unit row each in
    the order given.  bvec is small, seeded and non-zero, so that x_0 = rhs_y copied and A x = b solved differ by value."""
    P = dict(P)
    B, nz = P["Mblk"].shape[0], 6 * P["nb"]
    cols = [6 * b + r for b, rows in joints for r in rows]
    assert len(set(cols)) == len(cols) and all(0 <= b < P["nb"] and 0 <= r < 6 for b, rows in joints for r in rows)
    neq = len(cols)
    A = np.zeros((B, neq, nz))
    A[:, np.arange(neq), cols] = 1.0
    P["A"], P["neq"] = A, neq
    P["bvec"] = 0.05 * np.random.default_rng(seed).standard_normal((B, neq))
    return P


ALL6 = (0, 1, 2, 3, 4, 5)
# id: (random_problem options, joints).  n = 6 nb + neq picks the kernel's path: 18 and 54 factor in registers, and there only
# neq = 6 identity rows ON BODY 0 may take the pinned-body shortcut and the block-tridiagonal form; every other n <= 64 goes
# through the LDS elimination.  Seeds: the first for which the ORACLE ends at least half of the systems with status 0.
CASES = {
    "n18_no_rows": (dict(seed=50, B=2, nb=3, maxc=16, fd=8, nc_lo=6), []),
    "n18_no_rows_fd4": (dict(seed=151, B=3, nb=3, maxc=24, fd=4, nc_lo=6), []),
    "n54_no_rows": (dict(seed=52, B=2, nb=9, maxc=16, fd=8, nc_lo=6), []),
    "n18_body1_pinned": (dict(seed=153, B=3, nb=2, maxc=16, fd=8, nc_lo=4), [(1, ALL6)]),
    "n54_body5_pinned": (dict(seed=54, B=2, nb=8, maxc=24, fd=8, nc_lo=8), [(5, ALL6)]),
    "n54_body5_pinned_chain": (dict(seed=55, B=2, nb=8, maxc=24, fd=8, nc_lo=8, chain=True), [(5, ALL6)]),
    "n54_bodies0_3_pinned": (dict(seed=56, B=2, nb=7, maxc=24, fd=8, nc_lo=8), [(0, ALL6), (3, ALL6)]),
    "n54_bodies0_3_pinned_fd4": (dict(seed=57, B=2, nb=7, maxc=32, fd=4, nc_lo=8), [(0, ALL6), (3, ALL6)]),
    # (chain: with body 0's rows the identity and every contact between neighbours, only `neq == 6` keeps the shortcut away)
    "n54_bodies0_3_pinned_chain": (dict(seed=65, B=2, nb=7, maxc=24, fd=8, nc_lo=8, chain=True), [(0, ALL6), (3, ALL6)]),
    "n21_rot_body1": (dict(seed=58, B=4, nb=3, maxc=16, fd=8, nc_lo=4), [(1, (0, 1, 2))]),
    "n21_rot_body1_fd4": (dict(seed=59, B=2, nb=3, maxc=16, fd=4, nc_lo=4), [(1, (0, 1, 2))]),
    "n25_y_body2": (dict(seed=60, B=2, nb=4, maxc=16, fd=8, nc_lo=4), [(2, (4,))]),
    "n51_xyz_body2": (dict(seed=61, B=2, nb=8, maxc=24, fd=8, nc_lo=8), [(2, (3, 4, 5))]),
    "n64_mixed": (dict(seed=62, B=2, nb=10, maxc=32, fd=8, nc_lo=8), [(0, (4,)), (3, (0, 1)), (7, (5,))]),
    "n21_rot_body1_streamed": (dict(seed=63, B=2, nb=3, maxc=136, fd=8, nc_lo=100), [(1, (0, 1, 2))]),
    "n21_rot_body1_streamed_few": (dict(seed=64, B=2, nb=3, maxc=136, fd=8, nc_lo=6, nc_hi=16), [(1, (0, 1, 2))]),
}


# 100 or more random contacts on three bodies are never feasible: the oracle ends all 160 systems of seeds 63 .. 142 with status 4,
# with any iteration limit.  That case keeps every comparison (both sides stop on the same not-improving iterate); the same
# rows through the streamed state on a feasible contact set are "n21_rot_body1_streamed_few".
NEVER_FEASIBLE = ("n21_rot_body1_streamed",)


def problem(name):
    kw, joints = CASES[name]
    return with_unit_rows(S.random_problem(fixed_body0=False, **kw), joints, seed=1000 + kw["seed"])


def incoming(P):
    return np.random.default_rng(9).standard_normal((P["Mblk"].shape[0], 6 * P["nb"]))


def check_against_dense_oracle(P, fwd, bwd, max_iter=10, need_feasible=True):
    """The assertions and tolerances of the two files' dense-oracle tests, on host arrays: fwd = (x, lam, slack, nu, iters, status)
    of the kernel under test, bwd = (dM, dp, dcop, dA, db) of its backward for d loss / d x = incoming(P) at that forward state.
    At least half of the systems must end with status 0 IN THE ORACLE (random contact sets are often infeasible: status 4, where
    the iterates are still compared, but a case must not turn into a comparison of diverged iterates only; need_feasible=False
    for NEVER_FEASIBLE alone).  Returns the worst error per quantity."""
    from helpers import rel
    from oracle import lcp_oracle as O
    x, lam, slack, nu, it, st = fwd
    dM, dp, dcop, dA, db = bwd
    dl = incoming(P)
    B, fd = P["Mblk"].shape[0], P["fd"]
    worst, ok = {}, 0

    def hold(name, got, want, tol):
        e = rel(got, want)
        worst[name] = max(worst.get(name, 0.0), e)
        assert e < tol, (name, s, e)
    for s in range(B):
        nc = int(P["nc"][s])
        Q, p, G, h, A, b, F = S.expand_dense(P, s)
        zo, lo, so, nuo, ito, sto = O.forward(Q[None], p[None], G[None], h[None], A[None], b[None], F[None], max_iter=max_iter)
        ok += int(sto[0] == 0)
        assert abs(int(ito[0]) - int(it[s])) <= 1, (s, ito, it)      # the eps = 1e-12 stop test can flip on the last bit
        hold("x", x[s], zo[0], 1e-9)
        hold("slack", S.struct_vec(slack[s], nc, fd), so[0], 1e-6)
        hold("lam", S.struct_vec(lam[s], nc, fd), lo[0], 1e-5)
        hold("nu", nu[s], nuo[0], 1e-8)
        # backward as a pure function of the same forward state
        ls, ss = S.struct_vec(lam[s], nc, fd), S.struct_vec(slack[s], nc, fd)
        dQ, dpo, dG, dh, dAo, dbo, dF = O.backward(Q[None], G[None], A[None], F[None], x[s][None], ls[None], ss[None], nu[s][None], dl[s][None])
        wM, wp, wcop = S.contract_dense_grads(P, s, dQ[0], dpo[0], dG[0], dh[0], dF[0])
        for name, got, want in (("dM", dM[s], wM), ("dp", dp[s], wp), ("dcop", dcop[s], wcop), ("dA", dA[s], dAo[0]), ("db", db[s], dbo[0])):
            hold(name, got, want, 1e-6)
    assert 2 * ok >= B or not need_feasible, ("fewer than half of the systems are feasible in the oracle", ok, B)
    return worst
