// chamfer.h -- C ABI of the segmented nearest-neighbour search behind the chamfer distance of level-set meshes
// (csrc/chamfer.hip), exported by libdiffsdfsim_hip.so beside the functions of diffsdfsim_hip.h, whose conventions it
// shares (device pointers into caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*,
// DSS_E_* return codes).  Part of the checked ABI: bound by world_abi.PROTOTYPES, which tests/test_abi.py holds to these
// declarations.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The launch shape, for callers and tests that pick their sizes from it (diffsdfsim_amd/chamfer.py mirrors the four numbers;
 * tests/test_emu_chamfer.py compares the two):
 *   DSS_CHAMFER_TILE        reference points per LDS tile
 *   DSS_CHAMFER_QUERIES     query points per workgroup (256 threads, DSS_CHAMFER_QUERIES / 256 queries in each thread's registers)
 *   DSS_CHAMFER_SPLIT_TILES the fewest tiles a split of the reference range is given
 *   DSS_CHAMFER_TARGET_WG   workgroups the launcher aims at before it stops splitting (8 per compute unit of an MI355X) */
#define DSS_CHAMFER_TILE 512
#define DSS_CHAMFER_QUERIES 512
#define DSS_CHAMFER_SPLIT_TILES 2
#define DSS_CHAMFER_TARGET_WG 2048

/* Segmented nearest neighbour: nseg segments, segment s owns the query points q[q_off[s] : q_off[s + 1]] and the reference
 * points r[r_off[s] : r_off[s + 1]] (q_off, r_off [nseg + 1] ascending, on the device; at most max_q_len / max_r_len points of a
 * segment are read).  For every query i of segment s
 *   d2[i]  = min_j |q_i - r_j|^2 over the segment's reference points, evaluated as (qx-rx)^2 + (qy-ry)^2 + (qz-rz)^2 (the
 *            compiler may contract it into fused multiply-adds; no |q|^2 + |r|^2 - 2 q.r form is used anywhere)
 *   idx[i] = the row of that j in r (global, not relative to the segment); of equal computed distances the lowest j
 * A query whose segment has no reference point gets d2 = +inf, idx = -1; an empty query segment writes nothing.  The inputs
 * are finite: a precondition, not checked (a NaN distance never replaces the held minimum).
 * Launch: a 256-thread workgroup per (segment, block of DSS_CHAMFER_QUERIES queries, split of the reference range), reference
 * points streamed through LDS in tiles.  splits = min(ceil(tiles / DSS_CHAMFER_SPLIT_TILES), ceil(DSS_CHAMFER_TARGET_WG /
 * (nseg * query blocks))) with tiles = ceil(max_r_len / DSS_CHAMFER_TILE) and query blocks = ceil(max_q_len /
 * DSS_CHAMFER_QUERIES): with one split the results are written at once and no workspace is needed; with more, every split
 * writes its (d2, idx) to the workspace and a second kernel merges a query's partials in split order, a strictly smaller
 * distance replacing the held one.  No atomics: two calls return the same bits.
 * DSS_E_BADARG: nseg < 1, a negative length, a null q_off, r_off, d2 or idx, a null q with max_q_len > 0, a null r with
 * max_r_len > 0.  DSS_E_WORKSPACE: the workspace is null or smaller than dss_chamfer_nn_workspace_bytes (where that is not 0).
 * DSS_E_UNSUPPORTED: nseg * max_q_len or nseg * max_r_len (the bounds of Nq and Nr), a grid (nseg * query blocks * splits, nseg *
 * query blocks * DSS_CHAMFER_QUERIES / 256), the partials nseg * splits * max_q_len or the end of the last split (splits * its
 * whole tiles * DSS_CHAMFER_TILE) do not fit an int.  Nothing is launched and nothing written on any error. */
size_t dss_chamfer_nn_workspace_bytes(int nseg, int max_q_len, int max_r_len);
int dss_chamfer_nn(int nseg, int max_q_len, int max_r_len, const int *q_off, const double *q, const int *r_off, const double *r,
                   double *d2, int *idx, void *workspace, size_t workspace_bytes, void *stream);

/* out[s] = sum of v[off[s] : off[s + 1]] / (off[s + 1] - off[s]): the mean of a segment's values (NaN for an empty segment: 0 / 0).
 * A 256-thread workgroup per segment: strided partial sums, a wavefront butterfly, a fixed tree over the four wavefronts; the
 * order is a function of the segment's length alone, two calls return the same bits.
 * DSS_E_BADARG: nseg < 1, a null off or out, a null v.  Nothing is launched then. */
int dss_chamfer_segment_mean(int nseg, const int *off, const double *v, double *out, void *stream);

#ifdef __cplusplus
}
#endif
