// cloud_select.h -- C ABI of the selection of a labelled body's points from recorded organised clouds and of the per-segment
// statistics of the selected points (csrc/cloud_select.hip), exported by libdiffsdfsim_hip.so beside the functions of
// diffsdfsim_hip.h, whose conventions it shares (device pointers into caller-owned memory, double = binary64
// row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).  Part of the checked ABI: bound by
// world_abi.PROTOTYPES, which tests/test_abi.py holds to these declarations.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The points of label `label` in nframe recorded frames: `pointcloud[segmentation_mask == 4]` of match_pointcloud
 * (experiments/trajectory_fitting/optim_pointcloud_real.py:151-155) for every frame of a recording in one call.
 *   pcs  [nframe][H][W][3]   the organised cloud: the world-frame point seen by each pixel
 *   segs [nframe][H][W]      the label image
 * A pixel is selected if segs == label and its three coordinates are finite.  (The reference keeps a point with a NaN or an
 * infinite coordinate; in its loss such a point fails |p| < scale and adds nothing, so dropping it leaves the loss as it is
 * and keeps the statistics below finite.)  There is no erosion: the recorded script has none.  Points come in row-major
 * pixel order per frame, frames one after the other.
 *   dss_cloud_select_count   rows [nframe * H]: the selected pixels of each image row
 *   dss_cloud_select_emit    row_off [nframe * H]: the exclusive prefix sum of rows, made by the caller; pts [N][3], N its
 *                            total (pts may be NULL where N = 0).  Frame f owns pts[row_off[f * H] : row_off[(f + 1) * H]]
 *                            (N for the last frame).
 * A wavefront per image row, 64 columns at a time, ballot and prefix popcount; no atomics, the same bits in every call.
 * A null pointer (but pts, see above) or nframe, H or W below 1 gives DSS_E_BADARG; nframe * H * W of 2^31 or more gives
 * DSS_E_UNSUPPORTED, the code of every size outside the compiled limits.  Nothing is launched in either case. */
int dss_cloud_select_count(int nframe, int H, int W, int label, const double *pcs, const int *segs, int *rows, void *stream);
int dss_cloud_select_emit(int nframe, int H, int W, int label, const double *pcs, const int *segs, const int *row_off,
                          double *pts, void *stream);

/* Statistics of nseg segments of points: segment s owns pts[seg_off[s] : seg_off[s + 1]] (seg_off [nseg + 1] on the device;
 * at most max_seg_len points of a segment are read).
 *   out [nseg][10]   count, sum x, sum y, sum z, min x, min y, min z, max x, max y, max z
 * An empty segment gives count 0, sums 0, min +inf, max -inf.  The launch shape of dss_pointcloud_loss: a 256-thread
 * workgroup per (segment, chunk of 2 048 points), a wavefront butterfly, a fixed tree over the four wavefronts, one partial
 * [10] per workgroup in the workspace; a second kernel combines a segment's partials in index order.  No atomics: the order of
 * every sum is a function of the launch shape alone, two calls return the same bits.  min and max ignore a NaN coordinate
 * (fmin / fmax); the points of dss_cloud_select_emit have none.
 * DSS_E_BADARG: nseg < 1, max_seg_len < 0, a null seg_off or out, a null pts with max_seg_len > 0 (max_seg_len = 0, only
 * empty segments, is valid and needs no workspace).  DSS_E_WORKSPACE: the workspace is null or smaller than
 * dss_cloud_stats_workspace_bytes.  DSS_E_UNSUPPORTED: nseg * max(1, chunks) * 10 does not fit an int.  Nothing is launched then. */
size_t dss_cloud_stats_workspace_bytes(int nseg, int max_seg_len);
int dss_cloud_stats(int nseg, int max_seg_len, const int *seg_off, const double *pts, double *out, void *workspace,
                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
