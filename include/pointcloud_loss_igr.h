// pointcloud_loss_igr.h -- C ABI of the point-cloud loss of neural (decode_igr) bodies (csrc/pointcloud_loss_igr.hip), exported by
// libdiffsdfsim_hip.so beside the functions of diffsdfsim_hip.h, whose conventions it shares (device pointers into
// caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).  Part of
// the checked ABI: bound by world_abi.PROTOTYPES, which tests/test_abi.py holds to these declarations.
#pragma once
#include <stddef.h>

#include "diffsdfsim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSS_PC_IGR_OUT 13 /* sum (scale phi)^2, count, d / d quat (4), d / d pos (3), d / d latent (DSS_IGR_LATENT_MAX) */

/* match_pointcloud (experiments/trajectory_fitting/optim_pointcloud.py:166-201) over SDF3D.query_sdfs with decode_igr
 * (bodies.py:721-760, return_grads=False) for nseg (scene, observed frame) segments of neural bodies that share one network.
 * Segment s has a pose [7] (quaternion wxyz + position), a scale (shape_aux, a constant of the body) and the latent code
 * latents[lat_idx[s] * lat_stride : + L] (L = the network's latent size), and owns the world-frame points
 * pts[seg_off[s] : seg_off[s + 1]] (seg_off [nseg + 1] ascending, on the device; at most max_seg_len points of a segment are read).
 * With p = R(q)^T (x - pos), R normalised by 2 / (q.q), u = p / scale and phi = net(u, z):
 *   out[s] = sum over the points with all(|p| <= scale) of
 *            (scale phi)^2, 1, d / d q [4] (raw components: holds for a non-unit q), d / d pos [3], d / d z [4]        [13]
 * where the derivative goes through the network itself (the gradient of phi is not normalised: g = 2 scale phi d phi / d u,
 * latent term k = 2 scale^2 phi d phi / d z_k); latent slots >= L are exactly 0.  Points outside the query cube add nothing.
 *
 * n_pts is the number of rows of pts the segments may name (>= seg_off[nseg]); it is the capacity of the compacted query
 * list, and a point that would not fit is dropped.  Four stages on `stream`: per (segment, chunk of 2048
 * points) count the points inside the cube; scan the counts; compact (u, lat_idx, source row) in index order; evaluate the
 * network over the list with DSS_IGR_XYZ and DSS_IGR_LATENT (the host reads the list's length, one int: THE CALL BLOCKS until the stream
 * has drained and cannot be captured into a graph; in return the network's launch shape follows the list, not the capacity,
 * and an empty list launches nothing); per chunk form the 13 terms of its entries
 * (wavefront butterfly, fixed tree over the four wavefronts) and add a segment's chunk partials in index order.  No atomics: two
 * calls on the same input return the same bits, and a segment's row does not depend on the other segments of the call.
 *
 * DSS_E_BADARG: nseg < 1, a negative length, a null net (or one of its six pointers), seg_off, pose, scale, lat_idx, latents or
 * out, a null pts with max_seg_len > 0 and n_pts > 0, lat_stride < L.  DSS_E_WORKSPACE: the workspace is null or smaller than
 * dss_pointcloud_loss_igr_workspace_bytes (where that is not 0).  DSS_E_UNSUPPORTED: a network shape no kernel is built for, or
 * nseg * chunks * 13 or 12 * n_pts past an int.  Nothing is launched and nothing written on any of these argument errors.  A failure of
 * the runtime after the first launch (the read of the list's length: DSS_E_BADARG; a launch: DSS_E_UNSUPPORTED) leaves the
 * workspace written and `out` unwritten.
 * lat_idx is not checked against the table: its size is not an argument (the sibling dss_igr_query_list takes none either), a
 * row outside `latents` is the caller's error. */
size_t dss_pointcloud_loss_igr_workspace_bytes(int nseg, int max_seg_len, int n_pts);
int dss_pointcloud_loss_igr(const DssIgrNet *net, int nseg, int max_seg_len, const int *seg_off, const double *pts,
                            const double *pose /*[nseg][7] quat wxyz + pos*/, const double *scale /*[nseg]*/,
                            const int *lat_idx /*[nseg]*/, const double *latents, int lat_stride, int n_pts,
                            double *out /*[nseg][13]*/, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
