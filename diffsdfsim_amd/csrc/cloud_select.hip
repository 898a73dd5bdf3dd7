// cloud_select.hip -- the front of the recorded point-cloud fit (experiments/trajectory_fitting/optim_pointcloud_real.py): from
// label images and organised clouds to the flat pts / seg_off segments dss_pointcloud_loss reads, and the per-frame statistics
// the script initialises from (bounding-box diameter and centroid of the labelled points, :326-331, :499).  ABI and
// conventions: cloud_select.h.
//
//   dss_cloud_select_count   the row compaction of chunk_grid.h (a wavefront per image row) over cs_selected
//   dss_cloud_select_emit    the same walk; copies the selected pixels' points
//   dss_cloud_stats          the chunk grid of chunk_grid.h; each lane keeps sum / min / max of x, y, z in registers; block_sum for
//                            the sums, the same butterflies and tree with fmin / fmax for the rest, one partial [10] per
//                            workgroup; a second kernel combines a segment's partials in index order
//
// Memory-bound (4 B read per pixel and 24 B more per labelled pixel, 24 B per point); no atomics, so every output is a
// function of the input alone.
#include "../../include/diffsdfsim_hip.h"
#include "../../include/cloud_select.h"
#include "chunk_grid.h"

namespace {
using namespace dss;

constexpr int CS_OUT = 10;

__device__ __forceinline__ bool cs_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for a NaN)

// is pixel (row r, column c) of the frame at pixel index `base` a point of `label`
__device__ __forceinline__ bool cs_selected(const double *__restrict__ pcs, const int *__restrict__ segs, size_t base, int W, int r, int c,
                                            int label)
{
    if (c >= W) return false;
    const size_t i = base + (size_t)r * W + c;
    if (segs[i] != label) return false;
    return cs_finite(pcs[3 * i]) && cs_finite(pcs[3 * i + 1]) && cs_finite(pcs[3 * i + 2]);
}

__global__ void __launch_bounds__(CG_THREADS) cloud_select_count_kernel(int nrow, int H, int W, int label, const double *__restrict__ pcs,
                                                                       const int *__restrict__ segs, int *__restrict__ rows)
{
    int g;
    if (!row_of_wave(nrow, g)) return;
    const int frame = g / H, r = g - frame * H;
    const size_t base = (size_t)frame * H * W;
    const int n = row_count(W, [&](int c) { return cs_selected(pcs, segs, base, W, r, c, label); });
    if (lane_id() == 0) rows[g] = n;
}

__global__ void __launch_bounds__(CG_THREADS) cloud_select_emit_kernel(int nrow, int H, int W, int label, const double *__restrict__ pcs,
                                                                      const int *__restrict__ segs, const int *__restrict__ row_off,
                                                                      double *__restrict__ pts)
{
    int g;
    if (!row_of_wave(nrow, g)) return;
    const int frame = g / H, r = g - frame * H;
    const size_t base = (size_t)frame * H * W;
    row_emit(W, row_off[g], [&](int c) { return cs_selected(pcs, segs, base, W, r, c, label); }, [&](int slot, int c) {
        const double *in = pcs + 3 * (base + (size_t)r * W + c);
        double *out = pts + 3 * (size_t)slot;
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = in[i];
    });
}

__global__ void __launch_bounds__(CG_THREADS) cloud_stats_kernel(int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                const double *__restrict__ pts, double *__restrict__ partial)
{
    __shared__ double red_sum[CG_WAVES][3], red[CG_WAVES][6];      // red: min x, y, z, max x, y, z
    const int tid = threadIdx.x;
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    const double inf = __builtin_huge_val();
    double sum[3] = {0.0, 0.0, 0.0}, mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    const double *P = pts + 3 * (size_t)first;
    for (int i = lo + tid; i < hi; i += CG_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = P[3 * (size_t)i + k];
            sum[k] += v;
            mn[k] = fmin(mn[k], v);
            mx[k] = fmax(mx[k], v);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double b = wave_min(mn[k]), c = wave_max(mx[k]);
        if (lane_id() == 0) { red[tid / WAVE][k] = b; red[tid / WAVE][3 + k] = c; }
    }
    double *out = partial + (size_t)blockIdx.x * CS_OUT;
    block_sum<3>(sum, red_sum, out + 1);      // (its barrier is the one min and max wait for)
    if (tid == 0) out[0] = (double)(hi - lo);
    if (tid < 3) out[4 + tid] = fmin(fmin(red[0][tid], red[1][tid]), fmin(red[2][tid], red[3][tid]));
    else if (tid < 6) out[4 + tid] = fmax(fmax(red[0][tid], red[1][tid]), fmax(red[2][tid], red[3][tid]));
}

// out[s][k] = the segment's partials combined in index order (count 0, sums 0, min +inf, max -inf for an empty segment)
__global__ void __launch_bounds__(CG_THREADS) cloud_stats_combine_kernel(int nseg, int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                        const double *__restrict__ partial, double *__restrict__ out)
{
    const int t = blockIdx.x * CG_THREADS + threadIdx.x;
    if (t >= nseg * CS_OUT) return;
    const int s = t / CS_OUT, k = t - s * CS_OUT;
    int len = seg_off[s + 1] - seg_off[s];
    if (len > max_seg_len) len = max_seg_len;
    const int nch = len > 0 ? (len + CG_CHUNK - 1) / CG_CHUNK : 0;
    const double inf = __builtin_huge_val();
    double acc = k < 4 ? 0.0 : (k < 7 ? inf : -inf);
    for (int c = 0; c < nch; ++c) {
        const double v = partial[((size_t)s * chunks + c) * CS_OUT + k];
        acc = k < 4 ? acc + v : (k < 7 ? fmin(acc, v) : fmax(acc, v));
    }
    out[t] = acc;
}

bool cs_images_ok(int nframe, int H, int W) { return (long long)nframe * H * W <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int dss_cloud_select_count(int nframe, int H, int W, int label, const double *pcs, const int *segs, int *rows, void *stream)
{
    if (nframe <= 0 || H <= 0 || W <= 0 || !pcs || !segs || !rows) return DSS_E_BADARG;
    if (!cs_images_ok(nframe, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nframe * H;
    hipLaunchKernelGGL(cloud_select_count_kernel, dim3(row_blocks(nrow)), dim3(CG_THREADS), 0, (hipStream_t)stream, nrow, H, W, label,
                       pcs, segs, rows);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_cloud_select_emit(int nframe, int H, int W, int label, const double *pcs, const int *segs, const int *row_off, double *pts,
                          void *stream)
{
    // (pts may be NULL: no pixel selected, nothing is written)
    if (nframe <= 0 || H <= 0 || W <= 0 || !pcs || !segs || !row_off) return DSS_E_BADARG;
    if (!cs_images_ok(nframe, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nframe * H;
    hipLaunchKernelGGL(cloud_select_emit_kernel, dim3(row_blocks(nrow)), dim3(CG_THREADS), 0, (hipStream_t)stream, nrow, H, W, label,
                       pcs, segs, row_off, pts);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

size_t dss_cloud_stats_workspace_bytes(int nseg, int max_seg_len)
{
    if (nseg <= 0 || max_seg_len <= 0) return 0;
    return (size_t)nseg * pc_chunks(max_seg_len) * CS_OUT * sizeof(double);
}

int dss_cloud_stats(int nseg, int max_seg_len, const int *seg_off, const double *pts, double *out, void *workspace, size_t workspace_bytes,
                    void *stream)
{
    if (nseg <= 0 || max_seg_len < 0 || !seg_off || !out || (max_seg_len > 0 && !pts)) return DSS_E_BADARG;
    if ((long long)nseg * (pc_chunks(max_seg_len) > 0 ? pc_chunks(max_seg_len) : 1) > 0x7fffffffLL / CS_OUT)
        return DSS_E_UNSUPPORTED;      // grid.x and the int indices nseg * chunks * CS_OUT, nseg * CS_OUT
    const size_t need = dss_cloud_stats_workspace_bytes(nseg, max_seg_len);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DSS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = pc_chunks(max_seg_len);
    if (chunks > 0)
        hipLaunchKernelGGL(cloud_stats_kernel, dim3(chunks * nseg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, seg_off, pts,
                           (double *)workspace);
    hipLaunchKernelGGL(cloud_stats_combine_kernel, dim3((nseg * CS_OUT + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, st, nseg,
                       max_seg_len, chunks, seg_off, (const double *)workspace, out);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
