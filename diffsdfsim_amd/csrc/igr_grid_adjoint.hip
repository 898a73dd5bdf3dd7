// igr_grid_adjoint.hip -- the chain from a neural body's value grid to its latent code: g_latent[l] = sum_i g_grid[i] d f(x_i; z) / d z_l
// over the lattice nodes x_i of the grid.  ABI and conventions: igr_grid_adjoint.h.
//
// The adjoint of a value grid is sparse (a depth image touches the corners of the cells its hits fell into: tens of thousands of
// the two million nodes of a 128^3 grid) and the network is the expensive part (0.9 MFLOP per point and pass on the 128-wide
// network, 3.6 on the 256-wide one), so the non-zero nodes are compacted first and the MFMA kernel of igr_mlp.hip
// (dss::launch_igr_list, unchanged) walks the compacted list alone -- the count / scan / emit idiom of pointcloud_loss_igr.hip,
// restated here so that file keeps its bits:
//
//   iga_count_kernel    256 threads, one workgroup per (neural grid, 2048 consecutive samples), grid-major: ballot + popcount of
//                       the samples with !(g == 0) -> one count per chunk
//   iga_scan_kernel     one workgroup: exclusive prefix of the chunk counts (wavefront shuffles, the four wavefront totals in LDS,
//                       a running carry over tiles of 256 chunks) and the total, unclamped, in n_nodes
//   (host)              reads the total: longer than the list's capacity -> DSS_E_WORKSPACE before anything else is written
//   iga_emit_kernel     the same walk, over the chunks whose count is not zero: a node's slot is its chunk's offset + the non-zero
//                       nodes before it in index order; writes the lattice point u, the grid's latent row and the weight g
//   launch_igr_list     DSS_IGR_LATENT for exactly the list's length, or not at all for an empty list
//   iga_reduce_kernel   the chunk grid again: each lane takes its chunk's entries in strided order; wavefront butterfly, fixed tree
//                       over the four wavefronts, one partial [DSS_IGR_LATENT_MAX] per chunk
//   iga_sum_kernel      g_latent[r][l] = the chunk partials of the grids that name row r, added in grid-major order
//
// A workgroup finds its (grid, chunk) by walking the dims table (wavefront-uniform loads, a handful of grids), so no table of
// chunk offsets has to be built and uploaded.  No atomics anywhere.
#include "../../include/diffsdfsim_hip.h"
#include "launchers.h"
#include "igr_grid_adjoint.h"
#include "wave_utils.h"

#include <vector>

namespace {
using namespace dss;

constexpr int IGA_THREADS = 256, IGA_CHUNK = 2048, IGA_ITERS = IGA_CHUNK / IGA_THREADS, IGA_WAVES = IGA_THREADS / WAVE;
constexpr int IGA_LMAX = DSS_IGR_LATENT_MAX;

// samples of grid g (a dim >= 2 each and at most 2^31 - 1 - 2048 together: the host checked) and its chunks; 0 chunks for a grid that
// is not a neural one
__device__ __host__ inline int iga_chunks_of(int size) { return (int)(((long long)size + IGA_CHUNK - 1) / IGA_CHUNK); }

struct IgaChunk {
    int g, n[3], lo, hi;      // the grid, its dims, the chunk's samples [lo, hi) of the grid
};

// the chunk of workgroup blockIdx.x in the grid-major order of the neural grids: -> false if there is none (never, for the launch
// shapes of the host below)
__device__ __forceinline__ bool iga_chunk(int ngrid, const int *__restrict__ grid_dims, const int *__restrict__ lat_idx, IgaChunk &C)
{
    int w = blockIdx.x;
    for (int g = 0; g < ngrid; ++g) {
        if (lat_idx[g] < 0) continue;
        const int n0 = grid_dims[3 * g], n1 = grid_dims[3 * g + 1], n2 = grid_dims[3 * g + 2], size = n0 * n1 * n2, ch = iga_chunks_of(size);
        if (w < ch) {
            C.g = g; C.n[0] = n0; C.n[1] = n1; C.n[2] = n2;
            C.lo = w * IGA_CHUNK;
            C.hi = size - C.lo < IGA_CHUNK ? size : C.lo + IGA_CHUNK;
            return true;
        }
        w -= ch;
    }
    return false;
}

// does sample i (of the grid's adjoint G, i < hi) carry weight: anything but a zero, a NaN included
__device__ __forceinline__ bool iga_live(const double *__restrict__ G, int i, int hi)
{
    if (i >= hi) return false;
    return !(G[i] == 0.0);
}

__global__ void __launch_bounds__(IGA_THREADS) iga_count_kernel(int ngrid, const int *__restrict__ grid_off, const int *__restrict__ grid_dims,
                                                               const int *__restrict__ lat_idx, const double *__restrict__ g_grid,
                                                               int *__restrict__ counts)
{
    __shared__ int wcount[IGA_WAVES];
    IgaChunk C;
    if (!iga_chunk(ngrid, grid_dims, lat_idx, C)) {
        if (threadIdx.x == 0) counts[blockIdx.x] = 0;
        return;
    }
    const double *G = g_grid + (size_t)grid_off[C.g];
    int n = 0;
#pragma unroll
    for (int it = 0; it < IGA_ITERS; ++it) n += __popcll(__ballot(iga_live(G, C.lo + it * IGA_THREADS + (int)threadIdx.x, C.hi)));
    if (lane_id() == 0) wcount[threadIdx.x / WAVE] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wcount[0] + wcount[1]) + (wcount[2] + wcount[3]);
}

// (a list of more than 2^31 - 1 nodes cannot arise: the table's offsets are ints)
__global__ void __launch_bounds__(IGA_THREADS) iga_scan_kernel(int nwg, const int *__restrict__ counts, int *__restrict__ offs, int *__restrict__ total)
{
    __shared__ int wsum[IGA_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = tid / WAVE;
    int carry = 0;
    for (int base = 0; base < nwg; base += IGA_THREADS) {
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
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();      // the next tile overwrites wsum
    }
    if (tid == 0) total[0] = carry;
}

__global__ void __launch_bounds__(IGA_THREADS) iga_emit_kernel(int ngrid, int cap, const int *__restrict__ grid_off, const int *__restrict__ grid_dims,
                                                              const int *__restrict__ lat_idx, const double *__restrict__ g_grid,
                                                              const int *__restrict__ counts, const int *__restrict__ offs,
                                                              double *__restrict__ qpts, int *__restrict__ qlat, double *__restrict__ qw)
{
    __shared__ int cell[IGA_ITERS][IGA_WAVES];
    if (counts[blockIdx.x] == 0) return;      // (the whole workgroup: only the chunks that carry weight read g_grid a second time)
    IgaChunk C;
    if (!iga_chunk(ngrid, grid_dims, lat_idx, C)) return;
    const double *G = g_grid + (size_t)grid_off[C.g];
    const int tid = threadIdx.x, lane = lane_id(), wv = tid / WAVE;
    unsigned long long mask[IGA_ITERS];
#pragma unroll
    for (int it = 0; it < IGA_ITERS; ++it) {
        mask[it] = __ballot(iga_live(G, C.lo + it * IGA_THREADS + tid, C.hi));
        if (lane == 0) cell[it][wv] = __popcll(mask[it]);
    }
    __syncthreads();
    const int row = lat_idx[C.g], plane = C.n[1] * C.n[2];
    const double step[3] = {2.0 / (double)(C.n[0] - 1), 2.0 / (double)(C.n[1] - 1), 2.0 / (double)(C.n[2] - 1)};
    int at = offs[blockIdx.x];
#pragma unroll
    for (int it = 0; it < IGA_ITERS; ++it) {
        int mine = at;
        for (int w = 0; w < wv; ++w) mine += cell[it][w];
        if ((mask[it] >> lane) & 1ull) {
            const int slot = mine + __popcll(mask[it] & ((1ull << lane) - 1ull)), i = C.lo + it * IGA_THREADS + tid;
            if (slot < cap) {      // (the host launches this kernel only for a list that fits)
                const int i0 = i / plane, r = i - i0 * plane, i1 = r / C.n[2], i2 = r - i1 * C.n[2];
                qpts[3 * (size_t)slot] = __builtin_fma((double)i0, step[0], -1.0);
                qpts[3 * (size_t)slot + 1] = __builtin_fma((double)i1, step[1], -1.0);
                qpts[3 * (size_t)slot + 2] = __builtin_fma((double)i2, step[2], -1.0);
                qlat[slot] = row;
                qw[slot] = G[i];
            }
        }
        at += (cell[it][0] + cell[it][1]) + (cell[it][2] + cell[it][3]);
    }
}

// GS: doubles per row of glat (launch_igr_list's DSS_IGR_LATENT: 3 for L <= 3, L beyond); L: the network's latent size
__global__ void __launch_bounds__(IGA_THREADS) iga_reduce_kernel(int L, int GS, const int *__restrict__ counts, const int *__restrict__ offs,
                                                                const double *__restrict__ qw, const double *__restrict__ glat,
                                                                double *__restrict__ partial)
{
    __shared__ double red[IGA_WAVES][IGA_LMAX];
    const int tid = threadIdx.x;
    const int e0 = offs[blockIdx.x], e1 = e0 + counts[blockIdx.x];
    double acc[IGA_LMAX];
#pragma unroll
    for (int k = 0; k < IGA_LMAX; ++k) acc[k] = 0.0;
    for (int e = e0 + tid; e < e1; e += IGA_THREADS) {
        const double w = qw[e];
#pragma unroll
        for (int k = 0; k < IGA_LMAX; ++k)
            if (k < L) acc[k] += w * glat[(size_t)GS * e + k];
    }
#pragma unroll
    for (int k = 0; k < IGA_LMAX; ++k) {
        const double w = wave_sum(acc[k]);
        if (lane_id() == 0) red[tid / WAVE][k] = w;
    }
    __syncthreads();
    if (tid < IGA_LMAX) partial[(size_t)blockIdx.x * IGA_LMAX + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// g_latent[r][k] = the partials of the chunks of the grids that name row r, in grid-major order (zero for a row nobody names)
__global__ void __launch_bounds__(IGA_THREADS) iga_sum_kernel(int ngrid, int nlat, const int *__restrict__ grid_dims, const int *__restrict__ lat_idx,
                                                             const double *__restrict__ partial, double *__restrict__ g_latent)
{
    const int t = blockIdx.x * IGA_THREADS + threadIdx.x;
    if (t >= nlat * IGA_LMAX) return;
    const int r = t / IGA_LMAX, k = t - r * IGA_LMAX;
    double sum = 0.0;
    size_t c = 0;
    for (int g = 0; g < ngrid; ++g) {
        if (lat_idx[g] < 0) continue;
        const int ch = iga_chunks_of(grid_dims[3 * g] * grid_dims[3 * g + 1] * grid_dims[3 * g + 2]);
        if (lat_idx[g] == r)
            for (int j = 0; j < ch; ++j) sum += partial[(c + j) * IGA_LMAX + k];
        c += ch;
    }
    g_latent[t] = sum;
}

// the network's latent size, as igr_mlp.hip reads DssIgrNet (0, 0 = the 128 / 2 network); -1 = no kernel is built for the shape
int iga_latent(const DssIgrNet &N)
{
    const int w = N.width ? N.width : 128, l = N.latent ? N.latent : 2;
    return ((w == 128 && l == 2) || (w == 256 && l == 4)) ? l : -1;
}

// the workspace: doubles first, then ints
struct IgaWorkspace {
    double *partial, *qpts, *qw, *sdf, *glat;
    int *counts, *offs, *qlat;
    size_t bytes;
};
// base == NULL: only .bytes is set
IgaWorkspace iga_layout(void *base, size_t nwg, int cap)
{
    const size_t n = (size_t)cap;
    const size_t nd = nwg * IGA_LMAX + (3 + 1 + 1 + IGA_LMAX) * n, ni = 2 * nwg + n;
    IgaWorkspace W = {};
    W.bytes = nd * sizeof(double) + ((ni * sizeof(int) + 7) & ~(size_t)7);
    if (!base) return W;
    double *d = (double *)base;
    W.partial = d; d += nwg * IGA_LMAX;
    W.qpts = d; d += 3 * n;
    W.qw = d; d += n;
    W.sdf = d; d += n;
    W.glat = d; d += IGA_LMAX * n;
    int *i = (int *)d;
    W.counts = i; i += nwg;
    W.offs = i; i += nwg;
    W.qlat = i;
    return W;
}

}  // namespace

extern "C" {

size_t dss_igr_grid_adjoint_workspace_bytes(int nsamples, int cap, int nlat)
{
    if (nsamples <= 0 || cap <= 0 || nlat <= 0 || cap > 0x7fffffff / IGA_LMAX) return 0;
    // sum_g ceil(size_g / 2048) <= nsamples / 2048 + ngrid, and a grid has at least 8 samples
    return iga_layout(nullptr, (size_t)nsamples / IGA_CHUNK + (size_t)nsamples / 8 + 1, cap).bytes;
}

int dss_igr_grid_adjoint(const DssIgrNet *net, int ngrid, const int *grid_off, const int *grid_dims, const int *lat_idx, const double *latents,
                         int lat_stride, int nlat, const double *g_grid, int cap, double *g_latent, int *n_nodes, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    if (!net || !net->W0 || !net->b0 || !net->Wp || !net->bh || !net->W8 || !net->b8) return DSS_E_BADARG;
    if (ngrid < 1 || nlat < 1 || cap < 1 || !grid_off || !grid_dims || !lat_idx || !latents || !g_grid || !g_latent || !n_nodes || !workspace)
        return DSS_E_BADARG;
    const int L = iga_latent(*net);
    if (L < 0) return DSS_E_UNSUPPORTED;
    if (lat_stride < L) return DSS_E_BADARG;
    if (cap > 0x7fffffff / IGA_LMAX || nlat > 0x7fffffff / IGA_LMAX) return DSS_E_UNSUPPORTED;      // the int indices 4 cap (igr_mlp.hip), 4 nlat
    hipStream_t st = (hipStream_t)stream;
    // dims and latent rows decide the status and the launch shapes: the host reads them first
#if defined(DSS_EMU)
    const int *dims = grid_dims, *rows = lat_idx;      // (the emulator's device memory is the host's)
#else
    std::vector<int> host_dims(3 * (size_t)ngrid), host_rows(ngrid);
    if (hipMemcpyAsync(host_dims.data(), grid_dims, sizeof(int) * 3 * (size_t)ngrid, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(host_rows.data(), lat_idx, sizeof(int) * (size_t)ngrid, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return DSS_E_BADARG;      // (the runtime refused a pointer)
    const int *dims = host_dims.data(), *rows = host_rows.data();
#endif
    long long nwg_ll = 0;
    for (int g = 0; g < ngrid; ++g) {
        if (dims[3 * g] < 2 || dims[3 * g + 1] < 2 || dims[3 * g + 2] < 2 || rows[g] >= nlat) return DSS_E_BADARG;
        const long long size = (long long)dims[3 * g] * dims[3 * g + 1] * dims[3 * g + 2];
        if (size > 0x7fffffffLL - IGA_CHUNK) return DSS_E_UNSUPPORTED;      // (a sample index of the last chunk, lo + 2047, stays an int)
        if (rows[g] >= 0) nwg_ll += iga_chunks_of((int)size);
    }
    if (nwg_ll > 0x7fffffffLL) return DSS_E_UNSUPPORTED;      // grid.x
    const int nwg = (int)nwg_ll;
    if (workspace_bytes < iga_layout(nullptr, (size_t)nwg, cap).bytes) return DSS_E_WORKSPACE;
    const IgaWorkspace W = iga_layout(workspace, (size_t)nwg, cap);
    if (nwg > 0)
        hipLaunchKernelGGL(iga_count_kernel, dim3(nwg), dim3(IGA_THREADS), 0, st, ngrid, grid_off, grid_dims, lat_idx, g_grid, W.counts);
    hipLaunchKernelGGL(iga_scan_kernel, dim3(1), dim3(IGA_THREADS), 0, st, nwg, (const int *)W.counts, W.offs, n_nodes);
    // The list's length decides whether it fits, and the network's grid and workgroup shape: the host reads it (one int) and
    // launches for exactly that many nodes.
    int total = 0;
#if defined(DSS_EMU)
    total = n_nodes[0];
#else
    if (hipMemcpyAsync(&total, n_nodes, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return DSS_E_BADARG;
#endif
    if (total > cap) return DSS_E_WORKSPACE;
    if (total > 0) {
        hipLaunchKernelGGL(iga_emit_kernel, dim3(nwg), dim3(IGA_THREADS), 0, st, ngrid, cap, grid_off, grid_dims, lat_idx, g_grid,
                           (const int *)W.counts, (const int *)W.offs, W.qpts, W.qlat, W.qw);
        const int rc = dss::launch_igr_list(*net, W.qpts, W.qlat, latents, lat_stride, nullptr, total, DSS_IGR_LATENT, W.sdf, W.glat, st, -1);
        if (rc != DSS_OK) return rc;
    }
    if (nwg > 0)
        hipLaunchKernelGGL(iga_reduce_kernel, dim3(nwg), dim3(IGA_THREADS), 0, st, L, L > 3 ? L : 3, (const int *)W.counts, (const int *)W.offs,
                           (const double *)W.qw, (const double *)W.glat, W.partial);
    hipLaunchKernelGGL(iga_sum_kernel, dim3((nlat * IGA_LMAX + IGA_THREADS - 1) / IGA_THREADS), dim3(IGA_THREADS), 0, st, ngrid, nlat, grid_dims,
                       lat_idx, (const double *)W.partial, g_latent);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
