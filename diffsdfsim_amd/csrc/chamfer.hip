// chamfer.hip -- the nearest-neighbour search behind the chamfer distance of two vertex clouds
// (pytorch3d.loss.chamfer_distance(obj.verts, obj_target.verts), logged by every experiment of the reference in every
// iteration), for a batch of scenes in one call.  ABI, semantics and the launcher's rule: chamfer.h.
//
//   chamfer_nn_kernel      256-thread workgroups, one per (segment, block of CH_QUERIES queries, split of the reference range),
//                          flat grid, the split fastest.  A thread keeps CH_QPT queries and their running (minimum, index) in
//                          registers; the workgroup copies CH_TILE reference points at a time into LDS as three arrays x[], y[],
//                          z[], and every lane walks the tile reading the same address (a broadcast: no bank conflict).  Per
//                          pair: 3 subtractions, 1 multiply, 2 fused multiply-adds, 1 compare, selects of the distance and the
//                          index.  j ascends and only a strictly smaller distance replaces the held one, so of equal distances
//                          the lowest j stays.
//   chamfer_merge_kernel   a thread per query: its partials in split order, again strictly smaller replaces.
//   chamfer_mean_kernel    a workgroup per segment: the mean of its values in a fixed order.
//
// All fp64 VALU work, O(Nq Nr) per segment; no atomics, so every output is a function of the input alone.
#include "../../include/diffsdfsim_hip.h"
#include "../../include/chamfer.h"
#include "wave_utils.h"

namespace {
using namespace dss;

constexpr int CH_THREADS = 256, CH_TILE = DSS_CHAMFER_TILE, CH_QUERIES = DSS_CHAMFER_QUERIES, CH_QPT = CH_QUERIES / CH_THREADS;
static_assert(CH_QPT >= 1 && CH_QPT * CH_THREADS == CH_QUERIES, "queries per workgroup: a multiple of the workgroup");

__device__ __forceinline__ int ch_len(const int *__restrict__ off, int s, int max_len)
{
    const int len = off[s + 1] - off[s];
    return len < max_len ? len : max_len;      // (the grid and the workspace were sized for max_len)
}

// pd2 / pidx: null with one split (d2 / idx are written), else the partials [nseg][splits][max_q_len]
__global__ void __launch_bounds__(CH_THREADS) chamfer_nn_kernel(int qblocks, int splits, int split_len, int max_q_len, int max_r_len,
                                                               const int *__restrict__ q_off, const double *__restrict__ q,
                                                               const int *__restrict__ r_off, const double *__restrict__ r,
                                                               double *__restrict__ d2, int *__restrict__ idx, double *__restrict__ pd2,
                                                               int *__restrict__ pidx)
{
    __shared__ double tx[CH_TILE], ty[CH_TILE], tz[CH_TILE];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int k = b % splits;
    b /= splits;
    const int qb = b % qblocks, s = b / qblocks;
    const int qlen = ch_len(q_off, s, max_q_len), q0 = q_off[s], qlo = qb * CH_QUERIES;
    if (qlo >= qlen) return;      // (the whole workgroup: this segment has no query in the block)
    const int rlen = ch_len(r_off, s, max_r_len), r0 = r_off[s];
    const int lo = k * split_len < rlen ? k * split_len : rlen, hi = lo + split_len < rlen ? lo + split_len : rlen;

    double qx[CH_QPT], qy[CH_QPT], qz[CH_QPT], best[CH_QPT];
    int at[CH_QPT];
#pragma unroll
    for (int u = 0; u < CH_QPT; ++u) {
        const int i = qlo + tid + u * CH_THREADS;
        const double *p = q + 3 * (size_t)(q0 + (i < qlen ? i : qlen - 1));      // (a lane past the end searches for the last query)
        qx[u] = p[0]; qy[u] = p[1]; qz[u] = p[2];
        best[u] = __builtin_huge_val();
        at[u] = -1;
    }
    for (int t = lo; t < hi; t += CH_TILE) {
        const int n = hi - t < CH_TILE ? hi - t : CH_TILE;
        __syncthreads();      // (the previous tile has been read by every wavefront)
        for (int j = tid; j < n; j += CH_THREADS) {
            const double *p = r + 3 * (size_t)(r0 + t + j);
            tx[j] = p[0]; ty[j] = p[1]; tz[j] = p[2];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const double rx = tx[j], ry = ty[j], rz = tz[j];
#pragma unroll
            for (int u = 0; u < CH_QPT; ++u) {
                const double dx = qx[u] - rx, dy = qy[u] - ry, dz = qz[u] - rz;
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < best[u]) { best[u] = d; at[u] = t + j; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CH_QPT; ++u) {
        const int i = qlo + tid + u * CH_THREADS;
        if (i >= qlen) continue;
        const int row = at[u] < 0 ? -1 : r0 + at[u];
        if (pd2) {
            const size_t o = ((size_t)s * splits + k) * max_q_len + i;
            pd2[o] = best[u]; pidx[o] = row;
        } else {
            d2[q0 + i] = best[u]; idx[q0 + i] = row;
        }
    }
}

// a thread per (segment, query slot): the query's partials in split order
__global__ void __launch_bounds__(CH_THREADS) chamfer_merge_kernel(int qblocks, int splits, int max_q_len, const int *__restrict__ q_off,
                                                                  const double *__restrict__ pd2, const int *__restrict__ pidx,
                                                                  double *__restrict__ d2, int *__restrict__ idx)
{
    const int per = CH_QUERIES / CH_THREADS;      // workgroups per query block
    const int s = blockIdx.x / (qblocks * per), i = (blockIdx.x - s * qblocks * per) * CH_THREADS + threadIdx.x;
    if (i >= ch_len(q_off, s, max_q_len)) return;
    double best = __builtin_huge_val();
    int at = -1;
    for (int k = 0; k < splits; ++k) {
        const size_t o = ((size_t)s * splits + k) * max_q_len + i;
        const double d = pd2[o];
        if (d < best) { best = d; at = pidx[o]; }
    }
    d2[q_off[s] + i] = best; idx[q_off[s] + i] = at;
}

__global__ void __launch_bounds__(CH_THREADS) chamfer_mean_kernel(const int *__restrict__ off, const double *__restrict__ v,
                                                                 double *__restrict__ out)
{
    __shared__ double red[CH_THREADS / WAVE];
    const int s = blockIdx.x, tid = threadIdx.x, lo = off[s], hi = off[s + 1];
    double acc = 0.0;
    for (int i = lo + tid; i < hi; i += CH_THREADS) acc += v[i];
    acc = wave_sum(acc);
    if (lane_id() == 0) red[tid / WAVE] = acc;
    __syncthreads();
    if (tid == 0) out[s] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)(hi - lo);
}

struct ChShape { long long qblocks, tiles, splits, split_len; };

ChShape ch_shape(int nseg, int max_q_len, int max_r_len)
{
    ChShape c;
    c.qblocks = ((long long)max_q_len + CH_QUERIES - 1) / CH_QUERIES;
    c.tiles = ((long long)max_r_len + CH_TILE - 1) / CH_TILE;
    const long long base = (long long)nseg * (c.qblocks > 0 ? c.qblocks : 1);
    const long long by_tiles = (c.tiles + DSS_CHAMFER_SPLIT_TILES - 1) / DSS_CHAMFER_SPLIT_TILES, by_grid = (DSS_CHAMFER_TARGET_WG + base - 1) / base;
    c.splits = by_tiles < by_grid ? by_tiles : by_grid;
    if (c.splits < 1) c.splits = 1;
    c.split_len = (c.tiles + c.splits - 1) / c.splits * CH_TILE;      // whole tiles per split
    if (c.split_len < CH_TILE) c.split_len = CH_TILE;
    return c;
}

}  // namespace

extern "C" {

size_t dss_chamfer_nn_workspace_bytes(int nseg, int max_q_len, int max_r_len)
{
    if (nseg <= 0 || max_q_len <= 0 || max_r_len <= 0) return 0;
    const ChShape c = ch_shape(nseg, max_q_len, max_r_len);
    if (c.splits <= 1) return 0;
    return (size_t)nseg * (size_t)c.splits * (size_t)max_q_len * (sizeof(double) + sizeof(int));
}

int dss_chamfer_nn(int nseg, int max_q_len, int max_r_len, const int *q_off, const double *q, const int *r_off, const double *r,
                   double *d2, int *idx, void *workspace, size_t workspace_bytes, void *stream)
{
    if (nseg <= 0 || max_q_len < 0 || max_r_len < 0 || !q_off || !r_off || !d2 || !idx || (max_q_len > 0 && !q) || (max_r_len > 0 && !r))
        return DSS_E_BADARG;
    const ChShape c = ch_shape(nseg, max_q_len, max_r_len);
    const long long lim = 0x7fffffffLL;
    // the row counts nseg * max_len bound Nq and Nr; grid.x of the two kernels; the partials' count; the end of the last split
    if ((long long)nseg * max_q_len > lim || (long long)nseg * max_r_len > lim || (long long)nseg * c.qblocks * c.splits > lim ||
        (long long)nseg * c.qblocks * CH_QPT > lim || (long long)nseg * c.splits * max_q_len > lim || c.splits * c.split_len > lim)
        return DSS_E_UNSUPPORTED;
    const size_t need = dss_chamfer_nn_workspace_bytes(nseg, max_q_len, max_r_len);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DSS_E_WORKSPACE;
    if (max_q_len == 0) return DSS_OK;      // only empty query segments: nothing to write
    hipStream_t st = (hipStream_t)stream;
    double *pd2 = need > 0 ? (double *)workspace : nullptr;
    int *pidx = need > 0 ? (int *)(pd2 + (size_t)nseg * c.splits * max_q_len) : nullptr;
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((unsigned)(nseg * c.qblocks * c.splits)), dim3(CH_THREADS), 0, st, (int)c.qblocks, (int)c.splits,
                       (int)c.split_len, max_q_len, max_r_len, q_off, q, r_off, r, d2, idx, pd2, pidx);
    if (need > 0)
        hipLaunchKernelGGL(chamfer_merge_kernel, dim3((unsigned)(nseg * c.qblocks * (CH_QUERIES / CH_THREADS))), dim3(CH_THREADS), 0, st,
                           (int)c.qblocks, (int)c.splits, max_q_len, q_off, (const double *)pd2, (const int *)pidx, d2, idx);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_chamfer_segment_mean(int nseg, const int *off, const double *v, double *out, void *stream)
{
    if (nseg <= 0 || !off || !v || !out) return DSS_E_BADARG;
    hipLaunchKernelGGL(chamfer_mean_kernel, dim3((unsigned)nseg), dim3(CH_THREADS), 0, (hipStream_t)stream, off, v, out);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
