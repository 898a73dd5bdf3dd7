// chunk_grid.h -- the device idioms the observation kernels share, stated once: the chunk grid (256-thread workgroups, one per
// CG_CHUNK consecutive items), stream compaction over it and over image rows, and the workgroup / segment sums.
//
//   pc_chunk             the chunk of workgroup blockIdx.x in a flat grid of nseg * chunks, segment-major
//   chunk_count          ballot + popcount of the chunk's live items -> one count per chunk
//   chunk_scan_kernel    one workgroup: exclusive prefix of the chunk counts (wavefront shuffles, the four wavefront totals in LDS,
//                        a running carry over tiles of 256 chunks) and the total, clamped to a capacity
//   chunk_emit           the walk of chunk_count again: a live item's slot is its chunk's offset + the live items before it in index
//                        order (the (iteration, wavefront) cells before its own from LDS, the lanes below it from the ballot)
//   row_count, row_emit  the same for image rows: a wavefront per row, 64 columns at a time
//   block_sum            N sums over the workgroup: wavefront butterflies, then a fixed tree over the four wavefronts in LDS
//   segment_sum_kernel   out[s][k] = the segment's chunk partials added in index order
//
// Users: pointcloud_loss.hip, pointcloud_loss_grid_adj.hip, pointcloud_loss_igr.hip, igr_grid_adjoint.hip, cloud_select.hip,
// depth_camera.hip.  No atomics: slots and summation orders are functions of the launch shape alone.  The predicates and writers
// are lambdas; every trip count is wavefront-uniform, so each ballot sees its whole wavefront.
#pragma once
#include "wave_utils.h"

namespace dss {

constexpr int CG_THREADS = 256, CG_CHUNK = 2048, CG_ITERS = CG_CHUNK / CG_THREADS, CG_WAVES = CG_THREADS / WAVE;

inline int pc_chunks(int max_seg_len) { return (max_seg_len + CG_CHUNK - 1) / CG_CHUNK; }

// the chunk of workgroup blockIdx.x: -> false if it holds nothing of its segment
__device__ __forceinline__ bool pc_chunk(int max_seg_len, int chunks, const int *__restrict__ seg_off, int &s, int &first, int &lo, int &hi)
{
    s = blockIdx.x / chunks;
    const int chunk = blockIdx.x - s * chunks;
    first = seg_off[s];
    int len = seg_off[s + 1] - first;
    if (len > max_seg_len) len = max_seg_len;      // the workspace was sized for max_seg_len
    lo = chunk * CG_CHUNK;
    if (lo >= len) return false;                    // (the whole workgroup: nothing of this segment in the chunk)
    hi = lo + CG_CHUNK < len ? lo + CG_CHUNK : len;
    return true;
}

// the lanes of a ballot below this one
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// the fixed tree over the four wavefronts' values
template <class T> __device__ __forceinline__ T wave_tree(const T *x) { return (x[0] + x[1]) + (x[2] + x[3]); }

// -> the items i of [lo, lo + CG_CHUNK) with live(i), in thread 0 (the whole workgroup calls)
template <class LIVE> __device__ __forceinline__ int chunk_count(int lo, LIVE live)
{
    __shared__ int wcount[CG_WAVES];
    int n = 0;
#pragma unroll
    for (int it = 0; it < CG_ITERS; ++it) n += __popcll(__ballot(live(lo + it * CG_THREADS + (int)threadIdx.x)));
    if (lane_id() == 0) wcount[threadIdx.x / WAVE] = n;
    __syncthreads();
    return wave_tree(wcount);
}

// offs[i] = counts[0] + ... + counts[i - 1], total[0] = min(their sum, cap).  (A template, launched as chunk_scan_kernel<>, so that
// only the files that launch it compile it; static, so that each of them has its own.)
template <class = void>
static __global__ void __launch_bounds__(CG_THREADS) chunk_scan_kernel(int nwg, int cap, const int *__restrict__ counts, int *__restrict__ offs,
                                                                      int *__restrict__ total)
{
    __shared__ int wsum[CG_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = tid / WAVE;
    int carry = 0;
    for (int base = 0; base < nwg; base += CG_THREADS) {
        const int i = base + tid, c = i < nwg ? counts[i] : 0;
        int inc = c;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(inc, o, WAVE);
            if (lane >= o) inc += v;
        }
        if (lane == WAVE - 1) wsum[wv] = inc;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wsum[w];
        if (i < nwg) offs[i] = carry + before + inc - c;
        carry += wave_tree(wsum);
        __syncthreads();      // the next tile overwrites wsum
    }
    if (tid == 0) total[0] = carry < cap ? carry : cap;
}

// write(slot, i) for every live item i of [lo, lo + CG_CHUNK) whose slot is below cap; offs: chunk_scan_kernel's (the whole
// workgroup calls)
template <class LIVE, class WRITE> __device__ __forceinline__ void chunk_emit(int lo, LIVE live, const int *__restrict__ offs, int cap, WRITE write)
{
    __shared__ int cell[CG_ITERS][CG_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = tid / WAVE;
    unsigned long long mask[CG_ITERS];
#pragma unroll
    for (int it = 0; it < CG_ITERS; ++it) {
        mask[it] = __ballot(live(lo + it * CG_THREADS + tid));
        if (lane == 0) cell[it][wv] = __popcll(mask[it]);
    }
    __syncthreads();
    int at = offs[blockIdx.x];
#pragma unroll
    for (int it = 0; it < CG_ITERS; ++it) {
        int mine = at;
        for (int w = 0; w < wv; ++w) mine += cell[it][w];
        if ((mask[it] >> lane) & 1ull) {
            const int slot = mine + lanes_below(mask[it], lane);
            if (slot < cap) write(slot, lo + it * CG_THREADS + tid);
        }
        at += wave_tree(cell[it]);
    }
}

// Image rows, a wavefront each (workgroups of CG_THREADS: CG_WAVES rows): g = the wavefront's row of nrow, false beyond them.
__device__ __forceinline__ bool row_of_wave(int nrow, int &g)
{
    g = blockIdx.x * CG_WAVES + threadIdx.x / WAVE;
    return g < nrow;      // (the whole wavefront)
}
inline int row_blocks(int nrow) { return (nrow + CG_WAVES - 1) / CG_WAVES; }

// -> the columns c of [0, W) with selected(c), in every lane
template <class SEL> __device__ __forceinline__ int row_count(int W, SEL selected)
{
    const int lane = lane_id();
    int n = 0;
    for (int c0 = 0; c0 < W; c0 += WAVE) n += __popcll(__ballot(selected(c0 + lane)));
    return n;
}

// write(slot, c) for every selected column c of [0, W): slot = at + the selected columns before c
template <class SEL, class WRITE> __device__ __forceinline__ void row_emit(int W, int at, SEL selected, WRITE write)
{
    const int lane = lane_id();
    for (int c0 = 0; c0 < W; c0 += WAVE) {
        const int c = c0 + lane;
        const bool sel = selected(c);
        const unsigned long long mask = __ballot(sel);
        if (sel) write(at + lanes_below(mask, lane), c);
        at += __popcll(mask);
    }
}

// row[k] = acc[k] added over the workgroup, k < N: wavefront butterflies, then the fixed tree (red: LDS; a barrier inside)
template <int N> __device__ __forceinline__ void block_sum(const double *acc, double (*red)[N], double *__restrict__ row)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double w = wave_sum(acc[k]);
        if (lane_id() == 0) red[tid / WAVE][k] = w;
    }
    __syncthreads();
    if (tid < N) row[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// out[s][k] = the partials [N] of the segment's chunks added in index order (zero for an empty segment)
template <int N>
__global__ void __launch_bounds__(CG_THREADS) segment_sum_kernel(int nseg, int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                const double *__restrict__ partial, double *__restrict__ out)
{
    const int t = blockIdx.x * CG_THREADS + threadIdx.x;
    if (t >= nseg * N) return;
    const int s = t / N, k = t - s * N;
    int len = seg_off[s + 1] - seg_off[s];
    if (len > max_seg_len) len = max_seg_len;
    const int nch = len > 0 ? (len + CG_CHUNK - 1) / CG_CHUNK : 0;
    double sum = 0.0;
    for (int c = 0; c < nch; ++c) sum += partial[((size_t)s * chunks + c) * N + k];
    out[t] = sum;
}

}  // namespace dss
