"""CPU (the emulation build of the kernels): the dense LCP at its dispatch seams, with mixed statuses in one launch and under
every stop rule.  Inputs, preconditions and assertions are in lcp_dense_cases.py; test_lcp_dense_seams_gpu.py is the device twin.
This proves the kernels' logic, not the GPU build.
"""
import numpy as np
import pytest

import lcp_dense_cases as C
from emu import emu

BE = emu.EmuBackend


@pytest.mark.parametrize("B,nz,nineq,neq", C.SEAMS)
def test_size_seams_forward_and_backward_match_the_oracle(B, nz, nineq, neq):
    C.check_seam(BE(), B, nz, nineq, neq)


@pytest.mark.parametrize("nz,nineq,neq", C.EMBED)
def test_group_kernel_matches_wave_kernel_on_the_embedded_system(nz, nineq, neq):
    C.check_embedding(BE(), nz, nineq, neq)


def test_dispatch_takes_the_group_kernel_up_to_eight_on_every_axis_and_not_at_nine():
    C.check_dispatch_sizes(lambda *s: bool(emu.lib().dss_emu_lcp_dense_group_fits(*s)))


@pytest.mark.parametrize("nz,nineq,neq", C.EMBED)
def test_entry_runs_the_group_kernel_where_it_fits_not_the_wave_kernel(nz, nineq, neq):
    """What the entry returns for a small system is not what the wave kernel returns for it (the test hook): the eliminations
    differ, so some system differs in its last bits, while both agree to 1e-9."""
    ops = C.random_lcp(C.EMBED_SEED + nz + nineq + neq, 16, nz, nineq, neq)
    g, w = emu.lcp_dense_forward(*ops), emu.lcp_dense_forward(*ops, wave=True)
    assert (g[5] == w[5]).all() and C.rel(w[0], g[0]) < 1e-9
    assert not np.array_equal(g[0], w[0])


def test_wave_hook_refuses_max_iter_zero_like_the_entry():
    ops = [np.ascontiguousarray(a) for a in C.random_lcp(3, 2, 6, 4, 3)]
    L = emu.lib()
    out = [np.zeros((2, 6)), np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros(2, np.int32)]
    n = L.dss_lcp_dense_workspace_bytes(2, 6, 4, 3)
    ws = np.zeros(n, np.uint8)
    rc = L.dss_emu_lcp_dense_wave_forward(*[a.ctypes.data for a in ops], 2, 6, 4, 3, 1e-12, 3, 0, 1, *[a.ctypes.data for a in out],
                                          ws.ctypes.data, n, None)
    assert rc == C.E_BADARG and not any(a.any() for a in out)


@pytest.mark.parametrize("cond", C.CONDS)
@pytest.mark.parametrize("nz,nineq,neq", C.ILL)
def test_ill_scaled_q_on_the_group_path_residual_within_four_times_the_oracles(nz, nineq, neq, cond):
    C.check_ill_scaled(BE(), nz, nineq, neq, cond)


@pytest.mark.parametrize("kind", ["not_spd", "singular"])
@pytest.mark.parametrize("B,nz,nineq,neq", C.MIXED)
def test_mixed_statuses_in_one_launch(B, nz, nineq, neq, kind):
    C.check_mixed(BE(), B, nz, nineq, neq, kind)


@pytest.mark.parametrize("eps,nil,max_iter", C.RULES)
@pytest.mark.parametrize("B,nz,nineq,neq", C.STOPS)
def test_stop_rules_match_the_oracle(B, nz, nineq, neq, eps, nil, max_iter):
    C.check_stop(BE(), B, nz, nineq, neq, eps, nil, max_iter)


@pytest.mark.parametrize("B,nz,nineq,neq", C.STOPS)
def test_max_iter_zero_is_an_argument_error(B, nz, nineq, neq):
    C.check_max_iter_zero(BE(), B, nz, nineq, neq)


def test_argument_errors_leave_the_outputs_alone():
    C.check_argument_errors(BE())


def test_nz_682_is_refused():
    C.check_refused_size(BE())


@pytest.mark.parametrize("kind,check_spd,error", [("not_spd", True, "Q is not SPD"), ("singular", False, "Cannot perform LU factorization on Q"),
                                                  ("inaccurate", True, None)])
def test_lcpfunction_raises_for_any_failed_system_of_the_batch(kind, check_spd, error, monkeypatch, capsys):
    """LCPFunction's reading of the status words (diffsdfsim_amd/lcp/lcp.py), with the emulated kernel standing in for the
    device call: statuses {1, 4} and {2, 4} in one batch raise like the reference (lcp.py:109-113, batch.py:417-424), which
    checks every sample; {4} alone prints INACC_ERR once and returns."""
    import torch
    from diffsdfsim_amd.lcp import lcp as M

    def emulated(Q, p, G, h, A, b, F, eps, nil, max_iter, check):
        out = emu.lcp_dense_forward(*(t.numpy() for t in (Q, p, G, h, A, b, F)), eps, nil, max_iter, check)
        return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
    monkeypatch.setattr(M, "lcp_dense_forward", emulated)
    ops = [torch.from_numpy(a) for a in C.mixed_for_function(kind)]
    fn = M.LCPFunction(check_Q_spd=check_spd)
    if error:
        with pytest.raises(RuntimeError, match=error):
            fn(*ops)
    else:
        z = fn(*ops)
        assert capsys.readouterr().out.count(M.INACC_ERR.strip()) == 1
        assert z.shape == (13, 6) and torch.isfinite(z).all()
