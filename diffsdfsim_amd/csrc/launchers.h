// launchers.h -- the host functions that cross translation units inside csrc/, declared once: included by the file that
// defines each and by the files that call it.  None of them is part of the C ABI (include/diffsdfsim_hip.h).
#pragma once
#include "dss_device.h"

#include "../../include/diffsdfsim_hip.h"

namespace dss {
// narrowphase.hip: contact detection at the current pose (the lean compilation hands over to the full one, narrowphase_all.hip,
// when DssWorld.shape_rare is set, and to the box-only one, narrowphase_box.hip, when DssWorld.shape_box is);
// narrowphase_igr.hip: the query rounds of the pairs with a neural SDF body
int launch_find_contacts(const DssWorld &W, int *nc_out, int *body_out, int *face_out, double *abc_out,
                         double *geom_out, hipStream_t stream);
int launch_find_contacts_all(const DssWorld &W, int *nc_out, int *body_out, int *face_out, double *abc_out,
                             double *geom_out, hipStream_t stream);
int launch_find_contacts_box(const DssWorld &W, int *nc_out, int *body_out, int *face_out, double *abc_out,
                             double *geom_out, hipStream_t stream);
int launch_igr_rounds(const DssWorld &W, hipStream_t stream);
// igr_mlp.hip: the latent size of the network that DssIgrNet.width / .latent name (0, 0 = the 128 / 2 network), -1 = no kernel is
// built for the shape; one evaluation round over a device-side point list / over the value list and the gradient list of a query round
int igr_net_latent(const DssIgrNet &N);
int launch_igr_list(const DssIgrNet &N, const double *pts, const int *lat_idx, const double *latents, int lat_stride,
                    const int *n_dev, int n_cap, int mode, double *sdf, double *grad, hipStream_t stream, int est);
int launch_igr_pair(const DssIgrNet &N, const double *pts_v, const int *lat_v, const int *n_v, double *sdf_v, const double *pts_g,
                    const int *lat_g, const int *n_g, double *sdf_g, double *grad_g, const double *latents, int lat_stride, int n_cap,
                    hipStream_t stream, int est_v, int est_g);
// step_bwd_all.hip: first stage of the reverse sweep, full variant (bwd_pre_kernel over step_bwd_pre.h); lcp_contact.hip: dss_lcp_contact_backward for
// the rows of G that carry gradient (1 normal | 2 friction), multipliers optionally read from tape slot slot[s]
void launch_bwd_pre_all(const DssWorld &W, const DssAdjoint &A, hipStream_t stream);
int lcp_contact_backward_rows(const double *Mblk, const double *A, const double *cop, const int *cbody, const int *nc,
                              const int *active, int B, int nb, int neq, int maxc, int fric_dirs, const double *x,
                              const double *lam, const double *slack, const double *nu, const double *dl_dx, double *dMblk,
                              double *dpvec, double *dcop, double *dA, double *db, int rows, const int *slot, void *stream);
// lcp_dense_group.hip: eight lanes per system, for nz, nineq, neq <= 8
bool lcp_dense_group_fits(int nz, int nineq, int neq);
int launch_lcp_dense_group_forward(const double *Q, const double *p, const double *G, const double *h, const double *A, const double *b,
                                   const double *F, int B, int nz, int nineq, int neq, double eps, int not_improved_lim, int max_iter,
                                   int check_spd, double *zhat, double *lam, double *slack, double *nu, int *iters, int *status,
                                   hipStream_t stream);
int launch_lcp_dense_group_backward(const double *Q, const double *G, const double *A, const double *F, int B, int nz, int nineq, int neq,
                                    const double *zhat, const double *lam, const double *slack, const double *nu, const double *dl_dz,
                                    double *dQ, double *dp, double *dG, double *dh, double *dA, double *db, double *dF, hipStream_t stream);
}  // namespace dss
