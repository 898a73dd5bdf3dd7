// igr_grid_adjoint.hip -- the chain from a neural body's value grid to its latent code: g_latent[l] = sum_i g_grid[i] d f(x_i; z) / d z_l
// over the lattice nodes x_i of the grid.  ABI and conventions: igr_grid_adjoint.h.
//
// The adjoint of a value grid is sparse (a depth image touches the corners of the cells its hits fell into: tens of thousands of
// the two million nodes of a 128^3 grid) and the network is the expensive part (0.9 MFLOP per point and pass on the 128-wide
// network, 3.6 on the 256-wide one), so the non-zero nodes are compacted first and the MFMA kernel of igr_mlp.hip
// (dss::launch_igr_list, unchanged) walks the compacted list alone, by the count / scan / emit idiom of chunk_grid.h:
//
//   iga_count_kernel    chunk_count, one workgroup per (neural grid, 2048 consecutive samples), grid-major: the samples with !(g == 0)
//   chunk_scan_kernel   the chunks' offsets and the total, unclamped, in n_nodes
//   (host)              reads the total: longer than the list's capacity -> DSS_E_WORKSPACE before anything else is written
//   iga_emit_kernel     chunk_emit over the chunks whose count is not zero: writes the lattice point u, the grid's latent row and
//                       the weight g
//   launch_igr_list     DSS_IGR_LATENT for exactly the list's length, or not at all for an empty list
//   iga_reduce_kernel   the chunk grid again: each lane takes its chunk's entries in strided order; block_sum, one partial
//                       [DSS_IGR_LATENT_MAX] per chunk
//   iga_sum_kernel      g_latent[r][l] = the chunk partials of the grids that name row r, added in grid-major order
//
// A workgroup finds its (grid, chunk) by walking the dims table (wavefront-uniform loads, a handful of grids), so no table of
// chunk offsets has to be built and uploaded.  No atomics anywhere.
#include "../../include/diffsdfsim_hip.h"
#include "launchers.h"
#include "igr_grid_adjoint.h"
#include "chunk_grid.h"

namespace {
using namespace dss;

constexpr int IGA_LMAX = DSS_IGR_LATENT_MAX;

// samples of grid g (a dim >= 2 each and at most 2^31 - 1 - 2048 together: the host checked) and its chunks; 0 chunks for a grid that
// is not a neural one
__device__ __host__ inline int iga_chunks_of(int size) { return (int)(((long long)size + CG_CHUNK - 1) / CG_CHUNK); }

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
            C.lo = w * CG_CHUNK;
            C.hi = size - C.lo < CG_CHUNK ? size : C.lo + CG_CHUNK;
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

__global__ void __launch_bounds__(CG_THREADS) iga_count_kernel(int ngrid, const int *__restrict__ grid_off, const int *__restrict__ grid_dims,
                                                              const int *__restrict__ lat_idx, const double *__restrict__ g_grid,
                                                              int *__restrict__ counts)
{
    IgaChunk C;
    if (!iga_chunk(ngrid, grid_dims, lat_idx, C)) {
        if (threadIdx.x == 0) counts[blockIdx.x] = 0;
        return;
    }
    const double *G = g_grid + (size_t)grid_off[C.g];
    const int n = chunk_count(C.lo, [&](int i) { return iga_live(G, i, C.hi); });
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ void __launch_bounds__(CG_THREADS) iga_emit_kernel(int ngrid, int cap, const int *__restrict__ grid_off, const int *__restrict__ grid_dims,
                                                             const int *__restrict__ lat_idx, const double *__restrict__ g_grid,
                                                             const int *__restrict__ counts, const int *__restrict__ offs,
                                                             double *__restrict__ qpts, int *__restrict__ qlat, double *__restrict__ qw)
{
    if (counts[blockIdx.x] == 0) return;      // (the whole workgroup: only the chunks that carry weight read g_grid a second time)
    IgaChunk C;
    if (!iga_chunk(ngrid, grid_dims, lat_idx, C)) return;
    const double *G = g_grid + (size_t)grid_off[C.g];
    const int row = lat_idx[C.g], plane = C.n[1] * C.n[2];
    const double step[3] = {2.0 / (double)(C.n[0] - 1), 2.0 / (double)(C.n[1] - 1), 2.0 / (double)(C.n[2] - 1)};
    // (cap: the host launches this kernel only for a list that fits)
    chunk_emit(C.lo, [&](int i) { return iga_live(G, i, C.hi); }, offs, cap, [&](int slot, int i) {
        const int i0 = i / plane, r = i - i0 * plane, i1 = r / C.n[2], i2 = r - i1 * C.n[2];
        qpts[3 * (size_t)slot] = __builtin_fma((double)i0, step[0], -1.0);
        qpts[3 * (size_t)slot + 1] = __builtin_fma((double)i1, step[1], -1.0);
        qpts[3 * (size_t)slot + 2] = __builtin_fma((double)i2, step[2], -1.0);
        qlat[slot] = row;
        qw[slot] = G[i];
    });
}

// GS: doubles per row of glat (launch_igr_list's DSS_IGR_LATENT: 3 for L <= 3, L beyond); L: the network's latent size
__global__ void __launch_bounds__(CG_THREADS) iga_reduce_kernel(int L, int GS, const int *__restrict__ counts, const int *__restrict__ offs,
                                                                const double *__restrict__ qw, const double *__restrict__ glat,
                                                                double *__restrict__ partial)
{
    __shared__ double red[CG_WAVES][IGA_LMAX];
    const int tid = threadIdx.x;
    const int e0 = offs[blockIdx.x], e1 = e0 + counts[blockIdx.x];
    double acc[IGA_LMAX];
#pragma unroll
    for (int k = 0; k < IGA_LMAX; ++k) acc[k] = 0.0;
    for (int e = e0 + tid; e < e1; e += CG_THREADS) {
        const double w = qw[e];
#pragma unroll
        for (int k = 0; k < IGA_LMAX; ++k)
            if (k < L) acc[k] += w * glat[(size_t)GS * e + k];
    }
    block_sum<IGA_LMAX>(acc, red, partial + (size_t)blockIdx.x * IGA_LMAX);
}

// g_latent[r][k] = the partials of the chunks of the grids that name row r, in grid-major order (zero for a row nobody names)
__global__ void __launch_bounds__(CG_THREADS) iga_sum_kernel(int ngrid, int nlat, const int *__restrict__ grid_dims, const int *__restrict__ lat_idx,
                                                             const double *__restrict__ partial, double *__restrict__ g_latent)
{
    const int t = blockIdx.x * CG_THREADS + threadIdx.x;
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
    return iga_layout(nullptr, (size_t)nsamples / CG_CHUNK + (size_t)nsamples / 8 + 1, cap).bytes;
}

int dss_igr_grid_adjoint(const DssIgrNet *net, int ngrid, const int *grid_off, const int *grid_dims, const int *lat_idx, const double *latents,
                         int lat_stride, int nlat, const double *g_grid, int cap, double *g_latent, int *n_nodes, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    if (!net || !net->W0 || !net->b0 || !net->Wp || !net->bh || !net->W8 || !net->b8) return DSS_E_BADARG;
    if (ngrid < 1 || nlat < 1 || cap < 1 || !grid_off || !grid_dims || !lat_idx || !latents || !g_grid || !g_latent || !n_nodes || !workspace)
        return DSS_E_BADARG;
    const int L = igr_net_latent(*net);
    if (L < 0) return DSS_E_UNSUPPORTED;
    if (lat_stride < L) return DSS_E_BADARG;
    if (cap > 0x7fffffff / IGA_LMAX || nlat > 0x7fffffff / IGA_LMAX) return DSS_E_UNSUPPORTED;      // the int indices 4 cap (igr_mlp.hip), 4 nlat
    hipStream_t st = (hipStream_t)stream;
    // dims and latent rows decide the status and the launch shapes: the host reads them first
    HostInts host_dims, host_rows;
    if (!host_dims.copy(grid_dims, 3 * (size_t)ngrid, st) || !host_rows.copy(lat_idx, ngrid, st) || !host_sync(st)) return DSS_E_BADARG;
    const int *dims = host_dims.p, *rows = host_rows.p;
    long long nwg_ll = 0;
    for (int g = 0; g < ngrid; ++g) {
        if (dims[3 * g] < 2 || dims[3 * g + 1] < 2 || dims[3 * g + 2] < 2 || rows[g] >= nlat) return DSS_E_BADARG;
        const long long size = (long long)dims[3 * g] * dims[3 * g + 1] * dims[3 * g + 2];
        if (size > 0x7fffffffLL - CG_CHUNK) return DSS_E_UNSUPPORTED;      // (a sample index of the last chunk, lo + 2047, stays an int)
        if (rows[g] >= 0) nwg_ll += iga_chunks_of((int)size);
    }
    if (nwg_ll > 0x7fffffffLL) return DSS_E_UNSUPPORTED;      // grid.x
    const int nwg = (int)nwg_ll;
    if (workspace_bytes < iga_layout(nullptr, (size_t)nwg, cap).bytes) return DSS_E_WORKSPACE;
    const IgaWorkspace W = iga_layout(workspace, (size_t)nwg, cap);
    if (nwg > 0)
        hipLaunchKernelGGL(iga_count_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, ngrid, grid_off, grid_dims, lat_idx, g_grid, W.counts);
    // (no clamp: the table's offsets are ints, so a list of more than 2^31 - 1 nodes cannot arise)
    hipLaunchKernelGGL(chunk_scan_kernel<>, dim3(1), dim3(CG_THREADS), 0, st, nwg, 0x7fffffff, (const int *)W.counts, W.offs, n_nodes);
    // The list's length decides whether it fits, and the network's grid and workgroup shape: the host reads it (one int) and
    // launches for exactly that many nodes.
    HostInts host_total;
    if (!host_total.copy(n_nodes, 1, st) || !host_sync(st)) return DSS_E_BADARG;
    const int total = host_total.p[0];
    if (total > cap) return DSS_E_WORKSPACE;
    if (total > 0) {
        hipLaunchKernelGGL(iga_emit_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, ngrid, cap, grid_off, grid_dims, lat_idx, g_grid,
                           (const int *)W.counts, (const int *)W.offs, W.qpts, W.qlat, W.qw);
        const int rc = dss::launch_igr_list(*net, W.qpts, W.qlat, latents, lat_stride, nullptr, total, DSS_IGR_LATENT, W.sdf, W.glat, st, -1);
        if (rc != DSS_OK) return rc;
    }
    if (nwg > 0)
        hipLaunchKernelGGL(iga_reduce_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, L, L > 3 ? L : 3, (const int *)W.counts, (const int *)W.offs,
                           (const double *)W.qw, (const double *)W.glat, W.partial);
    hipLaunchKernelGGL(iga_sum_kernel, dim3((nlat * IGA_LMAX + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, st, ngrid, nlat, grid_dims,
                       lat_idx, (const double *)W.partial, g_latent);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
