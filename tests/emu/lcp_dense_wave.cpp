// TEST-ONLY: the wavefront-per-system dense LCP forward on systems the product hands to the eight-lanes-per-system kernel
// (nz, nineq, neq <= 8), so that tests/test_emu_lcp_dense.py can compare the two kernels on the same small systems.
// Same arguments and the same argument errors as dss_lcp_dense_forward.  And the size test of the dispatch itself
// (dss_emu_lcp_dense_group_fits): which kernel the entry picks cannot be seen from its results, both are right.
#include "dss_device.h"

#include "../../include/diffsdfsim_hip.h"

namespace dss {
bool lcp_dense_group_fits(int nz, int nineq, int neq);
int launch_lcp_dense_wave_forward(const double *Q, const double *p, const double *G, const double *h, const double *A, const double *b,
                                  const double *F, int B, int nz, int nineq, int neq, double eps, int not_improved_lim, int max_iter,
                                  int check_spd, double *zhat, double *lam, double *slack, double *nu, int *iters, int *status,
                                  void *workspace, hipStream_t stream);
}

extern "C" int dss_emu_lcp_dense_group_fits(int nz, int nineq, int neq) { return dss::lcp_dense_group_fits(nz, nineq, neq) ? 1 : 0; }

extern "C" int dss_emu_lcp_dense_wave_forward(const double *Q, const double *p, const double *G, const double *h, const double *A,
                                              const double *b, const double *F, int B, int nz, int nineq, int neq, double eps,
                                              int not_improved_lim, int max_iter, int check_spd, double *zhat, double *lam,
                                              double *slack, double *nu, int *iters, int *status, void *workspace,
                                              size_t workspace_bytes, void *stream)
{
    if (B <= 0 || nz <= 0 || nineq <= 0 || neq < 0 || max_iter < 1) return DSS_E_BADARG;
    if (workspace_bytes < dss_lcp_dense_workspace_bytes(B, nz, nineq, neq)) return DSS_E_WORKSPACE;
    return dss::launch_lcp_dense_wave_forward(Q, p, G, h, A, b, F, B, nz, nineq, neq, eps, not_improved_lim, max_iter, check_spd, zhat,
                                              lam, slack, nu, iters, status, workspace, (hipStream_t)stream);
}
