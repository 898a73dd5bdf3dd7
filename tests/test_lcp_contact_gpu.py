"""GPU: contact-structured LCP kernel (csrc/lcp_contact.hip) through the C ABI.

Checked against (a) the dense C oracle on the expanded operands (fresh seeds), (b) the dense HIP
kernel on the same expansion (two independent device paths), (c) size-independent properties at
config-3 batch size: residuals of the LCP conditions and run-to-run bit reproducibility.
Tolerance on velocities: 1e-9 relative (north_star: 1e-5).
"""
import numpy as np
import pytest
import torch

import equality_rows as EQ
import structured as S
from helpers import rel

pytestmark = pytest.mark.gpu


def dev(P):
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    return dict(Mblk=t(P["Mblk"]), pvec=t(P["pvec"]), A=t(P["A"]), bvec=t(P["bvec"]), cop=t(P["cop"]),
                cbody=t(P["cbody"], torch.int32), nc=t(P["nc"], torch.int32))


def run(P, max_iter=10):
    from diffsdfsim_amd.lcp.contact import lcp_contact_forward
    d = dev(P)
    out = lcp_contact_forward(d["Mblk"], d["pvec"], d["A"], d["bvec"], d["cop"], d["cbody"], d["nc"], P["fd"], max_iter=max_iter)
    torch.cuda.synchronize()
    return d, out


def test_block_tridiagonal_elimination_and_its_fallback_agree_with_the_dense_oracle():
    """Eight bodies, body 0 pinned, every contact between neighbours in the body order or with body 0 (a stack): the kernel
    eliminates H_oo as a block-tridiagonal matrix (kkt_reg.h: regk_factor_lead_tri).  One contact that skips a body (1 <-> 3) must
    send the scene through the general elimination instead.  Both against the dense oracle at 1e-9, with 70-100 contacts (two
    contacts per lane) and with 10-30."""
    from oracle import lcp_oracle as O
    for seed, maxc, lo in ((31, 128, 70), (32, 32, 10)):
        P = S.random_problem(seed=seed, B=6, nb=8, maxc=maxc, fd=8, nc_lo=lo, chain=True)
        cb = P["cbody"]
        for s in range(6):
            k = int(P["nc"][s])
            assert all(a == 0 or b == 0 or abs(int(a) - int(b)) == 1 for a, b in cb[s][:, :k].T)
        cb[4, :, 0] = (1, 3)          # scenes 4 and 5: no longer a chain
        cb[5, :, 1] = (6, 2)
        d, (x, lam, slack, nu, it, st) = run(P)
        x, it = x.cpu().numpy(), it.cpu().numpy()
        for s in range(6):
            Q, p, G, h, A, b, F = S.expand_dense(P, s)
            zo, lo_, so, nuo, ito, sto = O.forward(Q[None], p[None], G[None], h[None], A[None], b[None], F[None], max_iter=10)
            assert abs(int(ito[0]) - int(it[s])) <= 1
            assert rel(x[s], zo[0]) < 1e-9, (seed, s, rel(x[s], zo[0]))


# (nb, fd, random_problem options) as in tests/test_emu_lcp_contact.py: n = 12, 24, 30 through the LDS LU, n = 54 with contacts that do
# not form a chain (both forms: the natural register factorisation)
STATE_FORMS = [(2, 8, dict(fixed_body0=False)), (3, 8, {}), (4, 8, {}), (2, 4, dict(fixed_body0=False)), (3, 4, {}),
               (4, 4, {}), (8, 8, {}),
               # n = 18 without equality rows, and n = 54 as 7 bodies with bodies 0 and 3 pinned (neq = 12: the general elimination)
               (3, 8, dict(fixed_body0=False)), (7, 8, dict(fixed_body0=False, joints=[(0, EQ.ALL6), (3, EQ.ALL6)]))]


@pytest.mark.parametrize("nb,fd,kw", STATE_FORMS)
def test_register_and_streamed_state_agree(nb, fd, kw):
    """The forward kernel with the per-contact IPM state in registers (maxc = 128) and streamed through the workspace (the same problem
    padded to maxc = 136).  The emulator has them bitwise equal; on the device a value that goes through memory may meet an FMA that
    the register form does not, so: the same iteration counts and status, results within 1e-12."""
    kw = dict(kw)
    joints = kw.pop("joints", None)
    P = S.random_problem(seed=40 + nb + fd, B=2, nb=nb, maxc=128, fd=fd, nc_lo=40, **kw)
    if joints:
        P = EQ.with_unit_rows(P, joints, seed=40)
    a = [t.cpu().numpy() for t in run(P, max_iter=20)[1]]
    b = [t.cpu().numpy() for t in run(S.pad_contacts(P, 136), max_iter=20)[1]]
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    assert rel(b[0], a[0]) <= 1e-12 and rel(b[3], a[3]) <= 1e-12
    for s, nc in enumerate(P["nc"]):
        assert rel(b[1][s, :, :nc], a[1][s, :, :nc]) <= 1e-12 and rel(b[2][s, :, :nc], a[2][s, :, :nc]) <= 1e-12


@pytest.mark.parametrize("cfg", [dict(seed=11, B=6, nb=2, maxc=8, fd=8), dict(seed=12, B=4, nb=8, maxc=32, fd=8),
                                 dict(seed=13, B=3, nb=3, maxc=8, fd=4), dict(seed=14, B=2, nb=4, maxc=96, fd=8, nc_lo=70),
                                 dict(seed=15, B=5, nb=2, maxc=8, fd=8), dict(seed=16, B=3, nb=8, maxc=24, fd=8, nc_lo=10),
                                 dict(seed=17, B=2, nb=3, maxc=136, fd=8, nc_lo=100),   # > 128: the streaming kernel
                                 dict(seed=18, B=2, nb=8, maxc=24, fd=8, nc_lo=10, rot_A=True), dict(seed=19, B=2, nb=2, maxc=8, fd=8, rot_A=True)])   # equality rows that are not the identity: the unreduced KKT system
def test_forward_backward_vs_dense_oracle(cfg):
    from diffsdfsim_amd.lcp.contact import lcp_contact_backward
    from oracle import lcp_oracle as O
    cfg = dict(cfg)
    rot_A = cfg.pop("rot_A", False)
    P = S.random_problem(**cfg)
    if rot_A:   # body 0 still pinned, but by a rotated set of rows: the pinned-body shortcut must not trigger
        Qr, _ = np.linalg.qr(np.random.default_rng(77).standard_normal((6, 6)))
        P["A"][:, :, :6] = Qr
    d, (x, lam, slack, nu, it, st) = run(P)
    dl = torch.tensor(np.random.default_rng(9).standard_normal(tuple(x.shape)), device="cuda")
    dM, dp, dcop, dA, db = lcp_contact_backward(d["Mblk"], d["A"], d["cop"], d["cbody"], d["nc"], P["fd"], x, lam, slack, nu, dl, want_dA=True)
    x, lam, slack, nu, it, dl, dM, dp, dcop, dA, db = (v.cpu().numpy() for v in (x, lam, slack, nu, it, dl, dM, dp, dcop, dA, db))
    for s in range(P["Mblk"].shape[0]):
        nc, fd = int(P["nc"][s]), P["fd"]
        Q, p, G, h, A, b, F = S.expand_dense(P, s)
        zo, lo, so, nuo, ito, sto = O.forward(Q[None], p[None], G[None], h[None], A[None], b[None], F[None], max_iter=10)
        assert abs(int(ito[0]) - int(it[s])) <= 1  # the eps = 1e-12 stop test can flip on the last bit
        assert rel(x[s], zo[0]) < 1e-9
        assert rel(S.struct_vec(slack[s], nc, fd), so[0]) < 1e-6
        ls, ss = S.struct_vec(lam[s], nc, fd), S.struct_vec(slack[s], nc, fd)
        dQ, dpo, dG, dh, dAo, dbo, dF = O.backward(Q[None], G[None], A[None], F[None], x[s][None], ls[None], ss[None], nu[s][None], dl[s][None])
        wM, wp, wcop = S.contract_dense_grads(P, s, dQ[0], dpo[0], dG[0], dh[0], dF[0])
        assert rel(dM[s], wM) < 1e-6 and rel(dp[s], wp) < 1e-6 and rel(dcop[s], wcop) < 1e-6
        assert rel(dA[s], dAo[0]) < 1e-6 and rel(db[s], dbo[0]) < 1e-6


@pytest.mark.parametrize("name", list(EQ.CASES))
def test_any_block_of_unit_equality_rows_vs_dense_oracle(name):
    """No rows, partial rows (RotConstraint3D, X/Y/ZConstraint), a pinned body that is not body 0, two pinned bodies: every
    dispatch of n = 6 nb + neq (equality_rows.CASES), forward and backward, with dA and db.  Worst errors measured on the
    MI355X: DESIGN.md section 2."""
    from diffsdfsim_amd.lcp.contact import lcp_contact_backward
    P = EQ.problem(name)
    d, fwd = run(P)
    x, lam, slack, nu = fwd[:4]
    dl = torch.tensor(EQ.incoming(P), device="cuda")
    bwd = lcp_contact_backward(d["Mblk"], d["A"], d["cop"], d["cbody"], d["nc"], P["fd"], x, lam, slack, nu, dl, want_dA=True)
    torch.cuda.synchronize()
    B, nz = P["Mblk"].shape[0], 6 * P["nb"]
    bwd = [v.cpu().numpy() if v is not None else np.zeros(s) for v, s in zip(bwd, (0, 0, 0, (B, 0, nz), (B, 0)))]      # no rows: no dA, db
    worst = EQ.check_against_dense_oracle(P, [v.cpu().numpy() for v in fwd], bwd,
                                          need_feasible=name not in EQ.NEVER_FEASIBLE)
    print("%s: %s" % (name, ", ".join("%s %.1e" % kv for kv in worst.items())))


def test_more_than_64_unknowns_is_refused_by_both_entries():
    """(nb, neq) = (10, 5): n = 65.  DSS_E_UNSUPPORTED (-3) from the forward and the backward entry, before any launch."""
    from diffsdfsim_amd._lib import HipLibraryError
    from diffsdfsim_amd.lcp.contact import lcp_contact_backward
    P = EQ.with_unit_rows(S.random_problem(seed=1, B=1, nb=10, maxc=8, fixed_body0=False), [(0, (0, 1, 2, 3, 4))], seed=1)
    d = dev(P)
    with pytest.raises(HipLibraryError, match="dss_lcp_contact_forward failed with code -3$"):
        run(P)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    with pytest.raises(HipLibraryError, match="dss_lcp_contact_backward failed with code -3$"):
        lcp_contact_backward(d["Mblk"], d["A"], d["cop"], d["cbody"], d["nc"], 8, z(1, 60), z(1, 10, 8), z(1, 10, 8), z(1, 5), z(1, 60), want_dA=True)


def test_against_dense_hip_kernel():
    """Two independent device implementations of the same LCP must agree."""
    from diffsdfsim_amd.lcp.lcp import lcp_dense_forward
    P = S.random_problem(seed=21, B=8, nb=3, maxc=6, fd=8, ragged=False)
    d, (x, lam, slack, nu, it, st) = run(P)
    ops = [np.stack(o) for o in zip(*[S.expand_dense(P, s) for s in range(8)])]
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    zd, *_ = lcp_dense_forward(*(T(o) for o in ops), 1e-12, 3, 10, True)
    assert rel(x.cpu().numpy(), zd.cpu().numpy()) < 1e-9


def test_full_batch_properties_config3_size():
    """B=1024 scenes x 8 bodies, ragged contact counts: bit-reproducible; wherever the solver reports
    convergence the LCP conditions hold (random contact sets are often infeasible: those report
    DSS_LCP_INACCURATE exactly like the reference's INACC_ERR condition, batch.py:165-167)."""
    P = S.random_problem(seed=31, B=1024, nb=8, maxc=128, fd=8, nc_lo=4, nc_hi=40)
    d, (x, lam, slack, nu, it, st) = run(P)
    d2, (x2, lam2, slack2, *_r) = run(P)
    assert torch.equal(x, x2) and torch.equal(lam, lam2) and torch.equal(slack, slack2)
    st = st.cpu().numpy()
    assert set(np.unique(st)) <= {0, 4}
    x, lam, slack, nu = (v.cpu().numpy() for v in (x, lam, slack, nu))
    worst, checked = 0.0, 0
    for s in range(0, 1024, 7):
        if st[s] != 0:
            continue
        nc, fd = int(P["nc"][s]), P["fd"]
        Q, p, G, h, A, b, F = S.expand_dense(P, s)
        z, sl = S.struct_vec(lam[s], nc, fd), S.struct_vec(slack[s], nc, fd)
        assert (z > 0).all() and (sl > 0).all()
        rx = Q @ x[s] + G.T @ z + A.T @ nu[s] + p
        rz = G @ x[s] + sl - h - F @ z
        worst = max(worst, np.abs(rx).max(), np.abs(rz).max(), np.abs(A @ x[s] - b).max())
        checked += 1
    print("worst residual over", checked, "converged systems:", worst)
    # random contact sets: after the engine's 10 iterations the primal residual of the converged ones is at the 1e-3 level
    # (measured 1.9e-3 over 142 systems); the physical operands of the benchmark scenes are held tighter below
    assert checked > 100 and worst < 5e-3, (checked, worst)


def test_lcp_conditions_hold_on_the_benchmark_scenes():
    """The LCPs of BASELINE configs[2] as the stepper assembles them (1024 different box stacks, 80-110 contacts each, the
    operands of the last attempt): every scene converges (status 0), and the solution satisfies the conditions the
    reference's solver iterates on (batch.py:117-131) -- stationarity and the equality rows to round-off (every Newton step
    solves them exactly once a full step was taken), primal feasibility and complementarity to the interior point method's
    accuracy after its 10 iterations (engines.py:25)."""
    from diffsdfsim_amd import scenes
    from diffsdfsim_amd.engine import BatchEngine
    E = BatchEngine(scenes.box_stack(1024, nbox=7, seed=4242), maxc=128, max_cand=1024, max_pc=48, max_sub=0, strict_no_pen=False)
    for _ in range(2):
        E.step()
    st, nc = E.get("lcp_status"), E.get("nc")
    assert (st == 0).all(), np.unique(st)
    P = dict(Mblk=E.get("Mblk"), pvec=E.get("pvec"), A=E.get("Je"), bvec=np.zeros((E.B, E.neq)), cop=E.get("cop"),
             cbody=E.get("cop_body"), nc=E.get("lcp_iters") * 0 + E.get("nc"), nb=E.nb, neq=E.neq, maxc=E.maxc, fd=E.fd)
    x, lam, slack, nu = E.get("x"), E.get("lam"), E.get("slack"), E.get("nu")
    # the operands in the engine's arrays are those of the LAST attempt, whose contact count is the one before the
    # detection that followed it: read it off the multipliers (rows beyond it are untouched zeros)
    worst = dict(rx=0.0, ry=0.0, rz=0.0, comp=0.0)
    ncs = []
    for s in range(0, 1024, 37):
        n_used = int((np.abs(lam[s][0]) > 0).sum())
        P["nc"][s] = n_used
        ncs.append(n_used)
        fd = P["fd"]
        Q, p, G, h, A, b, F = S.expand_dense(P, s)
        z, sl = S.struct_vec(lam[s], n_used, fd), S.struct_vec(slack[s], n_used, fd)
        assert (z > 0).all() and (sl > 0).all()
        scale = max(1.0, np.abs(p).max())
        worst["rx"] = max(worst["rx"], np.abs(Q @ x[s] + G.T @ z + A.T @ nu[s] + p).max() / scale)
        worst["ry"] = max(worst["ry"], np.abs(A @ x[s] - b).max())
        worst["rz"] = max(worst["rz"], np.abs(G @ x[s] + sl - h - F @ z).max())
        worst["comp"] = max(worst["comp"], float(sl @ z) / len(z))
    assert min(ncs) >= 60 and max(ncs) <= 128, (min(ncs), max(ncs))
    assert worst["rx"] < 1e-9 and worst["ry"] < 1e-10 and worst["rz"] < 1e-6 and worst["comp"] < 1e-6, worst
