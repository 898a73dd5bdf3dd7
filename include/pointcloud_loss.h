// pointcloud_loss.h -- C ABI of the point-cloud loss (csrc/pointcloud_loss.hip), exported by libdiffsdfsim_hip.so beside the
// functions of diffsdfsim_hip.h, whose conventions it shares (device pointers into caller-owned memory, double =
// binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).  Part of the checked ABI: bound by
// world_abi.PROTOTYPES, which tests/test_abi.py holds to these declarations.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Point-cloud loss: replaces match_pointcloud (experiments/trajectory_fitting/optim_pointcloud.py:166-201) for nseg
 * (scene, observed frame) segments in one call, value and Jacobian together.  Segment s has its own pose [7] (quaternion
 * wxyz + position), shape_type and prm [4] (three shape parameters + the corner radius, a constant of the body) and owns the
 * world-frame points pts[seg_off[s] : seg_off[s + 1]] (seg_off [nseg + 1] on the device; at most max_seg_len points of a
 * segment are read).  With p = R(q)^T (x - pos), R normalised by 2 / (q.q) like Body3D.M, and phi = the body's SDF at p:
 *   out[s] = sum over the points with all(|p| <= scale) of  phi^2, 1, d phi^2 / d pose[7], d phi^2 / d prm[3]      [12]
 * (points outside the query cube add nothing, as `sdf_values[overlap_mask == False] = 0` there; the derivative w.r.t. the raw
 * quaternion components holds for a non-unit q).  No atomics: two calls on the same input return the same bits.
 * Analytic primitives only: a segment of DSS_SHAPE_IGR / DSS_SHAPE_GRID gives DSS_E_UNSUPPORTED and leaves `out` untouched.
 * The status depends on shape_type, so this call (unlike the others) copies those nseg ints to the host and waits for the
 * stream before it enqueues its two kernels. */
size_t dss_pointcloud_loss_workspace_bytes(int nseg, int max_seg_len);
int dss_pointcloud_loss(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose,
                        const int *shape_type, const double *prm, double *out, void *workspace, size_t workspace_bytes,
                        void *stream);

/* dss_pointcloud_loss with voxel-grid segments.  grid_id [nseg] (-1: none) points into the pooled table of DssWorld's
 * convention: grid_off [ngrid] (offset of a grid's samples in grid_data, in doubles), grid_dims [ngrid][3] (>= 2 per axis, x
 * slowest), grid_data.  Segments of types 0-5 are computed by the same code as in dss_pointcloud_loss (grid_id is not read for
 * them).  A segment of DSS_SHAPE_GRID with grid_id >= 0 has phi = scale * trilinear(samples) (scale = prm[3]; geom.h's
 * SHAPE_GRID value) and, as the derivative of phi w.r.t. the body-frame point, DiffGridSDF's rule: the interpolated
 * central-difference field of the samples, normalised once -- NOT the derivative of the trilinear value.  The chain to position
 * and raw quaternion is the one of the analytic segments; the three prm outputs of a grid segment are exactly 0.
 * DSS_SHAPE_IGR, and DSS_SHAPE_GRID with grid_id < 0, give DSS_E_UNSUPPORTED and leave `out` untouched; a grid_id >= ngrid or a
 * dim < 2 gives DSS_E_BADARG.  Same workspace (dss_pointcloud_loss_workspace_bytes), same two kernels' structure, same 12
 * outputs, no atomics.  The host reads shape_type, grid_id and grid_dims (and waits for the stream) before it enqueues. */
int dss_pointcloud_loss_grids(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose,
                              const int *shape_type, const double *prm, const int *grid_id, int ngrid, const int *grid_off,
                              const int *grid_dims, const double *grid_data, double *out, void *workspace,
                              size_t workspace_bytes, void *stream);

/* The adjoint of dss_pointcloud_loss_grids with respect to the samples (csrc/pointcloud_loss_grid_adj.hip).  The same segments,
 * points, poses and table; g_sum [nseg] are the upstream weights of the nseg sums.  For every DSS_SHAPE_GRID segment s with
 * g_sum[s] != 0 and every point of it inside the query cube, with phi = scale * sum_c w_c sample_c over the 8 corners of the
 * point's (clamped) cell:
 *   g_data[grid_off[grid_id[s]] + c] += 2 g_sum[s] phi scale w_c
 * -- the derivative of the trilinear value itself (the value is linear in the samples); the reference has none.  g_data is
 * pooled like grid_data and ADDED INTO: the caller zeroes it.  Analytic segments add nothing.  The adds are fp64 global atomics:
 * the order within one sample is the order of arrival, so two calls agree to the rounding of that sample's sum, not in bits.
 * The scale's gradient is not computed.  Arguments are checked as by dss_pointcloud_loss_grids, with the same statuses
 * (DSS_E_BADARG: a null pointer, nseg <= 0, ngrid < 0, a grid_id >= ngrid, a dim < 2; DSS_E_UNSUPPORTED: DSS_SHAPE_IGR, or
 * DSS_SHAPE_GRID with grid_id < 0); a refused call leaves g_data untouched.  The host reads shape_type, grid_id and grid_dims (and
 * waits for the stream) before it enqueues its one kernel. */
int dss_pointcloud_loss_grids_adjoint(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose,
                                      const int *shape_type, const double *prm, const int *grid_id, int ngrid, const int *grid_off,
                                      const int *grid_dims, const double *grid_data, const double *g_sum, double *g_data,
                                      void *stream);

#ifdef __cplusplus
}
#endif
