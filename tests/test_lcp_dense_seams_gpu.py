"""GPU: the dense LCP at its dispatch seams, with mixed statuses in one launch and under every stop rule, on the device through
the raw C ABI.  Inputs, preconditions and assertions are in lcp_dense_cases.py; test_emu_lcp_dense_seams.py is the emulator twin.
An overrun lands in the guard row behind an output and is reported as an assertion; no case relies on a fault.
"""
import pytest

import lcp_dense_cases as C

pytestmark = pytest.mark.gpu


def BE():
    from diffsdfsim_amd.engine import TorchBackend
    return TorchBackend("cuda:0")


@pytest.mark.parametrize("B,nz,nineq,neq", C.SEAMS)
def test_size_seams_forward_and_backward_match_the_oracle(B, nz, nineq, neq):
    C.check_seam(BE(), B, nz, nineq, neq)


@pytest.mark.parametrize("nz,nineq,neq", C.EMBED)
def test_group_kernel_matches_wave_kernel_on_the_embedded_system(nz, nineq, neq):
    C.check_embedding(BE(), nz, nineq, neq)


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


def test_largest_accepted_size_matches_the_oracle():
    """SLOW for this suite: nz = 681, nineq = 2, neq = 0, one system, three iterations -- the largest nz the entry accepts
    (65 488 B of staged vectors), against the oracle at 1e-9.  Measured once on the MI355X: 0.7 s, the oracle's solve included."""
    C.check_largest_size(BE(), 681)


@pytest.mark.parametrize("kind,check_spd,error", [("not_spd", True, "Q is not SPD"), ("singular", False, "Cannot perform LU factorization on Q"),
                                                  ("inaccurate", True, None)])
def test_lcpfunction_raises_for_any_failed_system_of_the_batch(kind, check_spd, error, capsys):
    """Statuses {1, 4} and {2, 4} in one batch raise like the reference, which checks every sample (lcp.py:109-113,
    batch.py:417-424); {4} alone prints INACC_ERR once and returns."""
    import torch
    from diffsdfsim_amd.lcp import lcp as M
    ops = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in C.mixed_for_function(kind)]
    fn = M.LCPFunction(check_Q_spd=check_spd)
    if error:
        with pytest.raises(RuntimeError, match=error):
            fn(*ops)
    else:
        z = fn(*ops)
        assert capsys.readouterr().out.count(M.INACC_ERR.strip()) == 1
        assert z.shape == (13, 6) and bool(torch.isfinite(z).all())
