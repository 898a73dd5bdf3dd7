// pointcloud_loss_igr.hip -- the point-cloud loss of experiments/trajectory_fitting/optim_pointcloud.py (`match_pointcloud`,
// :166-201) for neural (decode_igr) bodies: value, pose Jacobian and latent Jacobian of a batch of (scene, observed frame)
// segments.  ABI and conventions: pointcloud_loss_igr.h.
//
// The network is the expensive part (0.9 MFLOP per point and pass on the 128-wide network, 3.6 on the 256-wide one) and an
// observed cloud lies partly outside the estimate's query cube, so the points inside are compacted first and the MFMA kernel of
// igr_mlp.hip (dss::launch_igr_list, unchanged) walks the compacted list alone:
//
//   pci_count_kernel    chunk_count over the chunk grid (chunk_grid.h), segment-major: the points inside the cube
//   chunk_scan_kernel   the chunks' offsets and the total, clamped to the list's capacity, in device memory
//   pci_emit_kernel     chunk_emit: writes u = p / scale, the segment's latent row and the source row
//   launch_igr_list     DSS_IGR_XYZ, then DSS_IGR_LATENT (two passes of its own for L = 4).  A device-side length of 0 would be
//                       safe there (tiles_for gives at least one workgroup and the persistent tile loop `for (base = bid * PTS;
//                       base < n; ...)` does not run), but the grid and the workgroup shape would be picked for the capacity
//                       n_pts, not for the list: the host reads the total (one int, the call's only wait, as dss_pointcloud_loss
//                       reads its shape types) and launches for exactly that length, or not at all for an empty list
//   pci_reduce_kernel   the chunk grid again: each lane takes its chunk's entries in strided order and forms the 13 terms, the
//                       pose chain of pointcloud_point.h written out for plain doubles; block_sum, one partial [13] per chunk
//   segment_sum_kernel  out[s][k] = the segment's chunk partials added in index order
//
// The body-frame point is formed with explicit fused multiply-adds (pci_body_point), so that the three kernels that decide
// "inside" decide it on the same bits whatever the compiler contracts elsewhere.  No atomics: a segment's row is a function of
// its own points, pose, scale and latent row alone.
#include "../../include/diffsdfsim_hip.h"
#include "geom.h"
#include "launchers.h"
#include "../../include/pointcloud_loss_igr.h"
#include "chunk_grid.h"

namespace {
using namespace dss;

constexpr int PCI_OUT = DSS_PC_IGR_OUT, PCI_LMAX = DSS_IGR_LATENT_MAX;

struct PciSegment {
    double q[4], pos[3], R[9], scale;
};

__device__ __forceinline__ void pci_segment(PciSegment &S, const double *__restrict__ pose, double scale)
{
    for (int i = 0; i < 4; ++i) S.q[i] = pose[i];
    for (int i = 0; i < 3; ++i) S.pos[i] = pose[4 + i];
    quat_to_mat(S.q, S.R);
    S.scale = scale;
}

// d = x - pos, p = R^T d; -> all(|p| <= scale)
__device__ __forceinline__ bool pci_body_point(const PciSegment &S, const double *__restrict__ x, double *d, double *p)
{
    for (int i = 0; i < 3; ++i) d[i] = x[i] - S.pos[i];
    for (int i = 0; i < 3; ++i) p[i] = __builtin_fma(S.R[6 + i], d[2], __builtin_fma(S.R[3 + i], d[1], S.R[i] * d[0]));
    return fabs(p[0]) <= S.scale && fabs(p[1]) <= S.scale && fabs(p[2]) <= S.scale;
}

// is point i (of the segment's points P, i < hi) inside the segment's cube
__device__ __forceinline__ bool pci_inside(const PciSegment &S, const double *__restrict__ P, int i, int hi)
{
    if (i >= hi) return false;
    const double x[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
    double d[3], p[3];
    return pci_body_point(S, x, d, p);
}

__global__ void __launch_bounds__(CG_THREADS) pci_count_kernel(int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                              const double *__restrict__ pts, const double *__restrict__ pose,
                                                              const double *__restrict__ scale, int *__restrict__ counts)
{
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) {
        if (threadIdx.x == 0) counts[blockIdx.x] = 0;
        return;
    }
    PciSegment S;
    pci_segment(S, pose + 7 * (size_t)s, scale[s]);
    const double *P = pts + 3 * (size_t)first;
    const int n = chunk_count(lo, [&](int i) { return pci_inside(S, P, i, hi); });
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ void __launch_bounds__(CG_THREADS) pci_emit_kernel(int max_seg_len, int chunks, int cap, const int *__restrict__ seg_off,
                                                             const double *__restrict__ pts, const double *__restrict__ pose,
                                                             const double *__restrict__ scale, const int *__restrict__ lat_idx,
                                                             const int *__restrict__ offs, double *__restrict__ qpts,
                                                             int *__restrict__ qlat, int *__restrict__ qsrc)
{
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    PciSegment S;
    pci_segment(S, pose + 7 * (size_t)s, scale[s]);
    const double *P = pts + 3 * (size_t)first;
    const int row = lat_idx[s];
    chunk_emit(lo, [&](int i) { return pci_inside(S, P, i, hi); }, offs, cap, [&](int slot, int i) {
        const double x[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
        double d[3], p[3];
        pci_body_point(S, x, d, p);
        for (int k = 0; k < 3; ++k) qpts[3 * (size_t)slot + k] = p[k] / S.scale;      // (a division, as query_sdfs writes it)
        qlat[slot] = row;
        qsrc[slot] = first + i;
    });
}

// GS: doubles per row of glat (launch_igr_list's DSS_IGR_LATENT: 3 for L <= 3, L beyond); L: the network's latent size
__global__ void __launch_bounds__(CG_THREADS) pci_reduce_kernel(int max_seg_len, int chunks, int cap, int L, int GS,
                                                                const int *__restrict__ seg_off, const double *__restrict__ pts,
                                                                const double *__restrict__ pose, const double *__restrict__ scale,
                                                                const int *__restrict__ counts, const int *__restrict__ offs,
                                                                const int *__restrict__ qsrc, const double *__restrict__ sdf,
                                                                const double *__restrict__ gxyz, const double *__restrict__ glat,
                                                                double *__restrict__ partial)
{
    __shared__ double red[CG_WAVES][PCI_OUT];
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    PciSegment S;
    pci_segment(S, pose + 7 * (size_t)s, scale[s]);
    const double two_s = 2.0 / (S.q[0] * S.q[0] + S.q[1] * S.q[1] + S.q[2] * S.q[2] + S.q[3] * S.q[3]);
    const double r = S.q[0], qi = S.q[1], qj = S.q[2], qk = S.q[3], sc = S.scale;
    const double *R = S.R;
    const int tid = threadIdx.x;
    const int e0 = offs[blockIdx.x];
    int e1 = e0 + counts[blockIdx.x];
    if (e1 > cap) e1 = cap;
    double acc[PCI_OUT];
#pragma unroll
    for (int k = 0; k < PCI_OUT; ++k) acc[k] = 0.0;
    for (int e = e0 + tid; e < e1; e += CG_THREADS) {
        // the quaternion chain needs d = x - pos beside p, and u = p / scale does not give it back exactly: the entry names its
        // source row and the point is formed again, on the bits the mask was decided on
        const size_t src = (size_t)qsrc[e];
        const double x[3] = {pts[3 * src], pts[3 * src + 1], pts[3 * src + 2]};
        double d[3], p[3];
        pci_body_point(S, x, d, p);
        const double phi = sdf[e], v = sc * phi, k2 = 2.0 * sc * phi;
        const double g[3] = {k2 * gxyz[3 * (size_t)e], k2 * gxyz[3 * (size_t)e + 1], k2 * gxyz[3 * (size_t)e + 2]};      // d (scale phi)^2 / d p
        acc[0] += v * v;
        acc[1] += 1.0;
        // a[j][i] = d_j g_i contracted with d N / d q_k (N = (R - 1) / two_s): the chain of pointcloud_point.h
        const double a00 = d[0] * g[0], a01 = d[0] * g[1], a02 = d[0] * g[2];
        const double a10 = d[1] * g[0], a11 = d[1] * g[1], a12 = d[1] * g[2];
        const double a20 = d[2] * g[0], a21 = d[2] * g[1], a22 = d[2] * g[2];
        const double sr = qk * (a10 - a01) + qj * (a02 - a20) + qi * (a21 - a12);
        const double si = qj * (a01 + a10) + qk * (a02 + a20) + r * (a21 - a12) - 2.0 * qi * (a11 + a22);
        const double sj = qi * (a01 + a10) + qk * (a12 + a21) + r * (a02 - a20) - 2.0 * qj * (a00 + a22);
        const double sk = qi * (a02 + a20) + qj * (a12 + a21) + r * (a10 - a01) - 2.0 * qk * (a00 + a11);
        const double gn = g[0] * (p[0] - d[0]) + g[1] * (p[1] - d[1]) + g[2] * (p[2] - d[2]);
        acc[2] += two_s * (sr - r * gn);
        acc[3] += two_s * (si - qi * gn);
        acc[4] += two_s * (sj - qj * gn);
        acc[5] += two_s * (sk - qk * gn);
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[6 + i] += -(R[3 * i] * g[0] + R[3 * i + 1] * g[1] + R[3 * i + 2] * g[2]);
        const double kz = k2 * sc;
#pragma unroll
        for (int k = 0; k < PCI_LMAX; ++k)
            if (k < L) acc[9 + k] += kz * glat[(size_t)GS * e + k];
    }
    block_sum<PCI_OUT>(acc, red, partial + (size_t)blockIdx.x * PCI_OUT);
}

// the workspace: doubles first, then ints
struct PciWorkspace {
    double *partial, *qpts, *sdf, *gxyz, *glat;
    int *counts, *offs, *total, *qlat, *qsrc;
    size_t bytes;
};
// base == NULL: only .bytes is set
PciWorkspace pci_layout(void *base, int nseg, int max_seg_len, int n_pts)
{
    const size_t nwg = (size_t)nseg * pc_chunks(max_seg_len), n = (size_t)n_pts;
    const size_t nd = nwg * PCI_OUT + (3 + 1 + 3 + PCI_LMAX) * n, ni = 2 * nwg + 2 + 2 * n;
    PciWorkspace W = {};
    W.bytes = nd * sizeof(double) + ((ni * sizeof(int) + 7) & ~(size_t)7);
    if (!base) return W;
    double *d = (double *)base;
    W.partial = d; d += nwg * PCI_OUT;
    W.qpts = d; d += 3 * n;
    W.sdf = d; d += n;
    W.gxyz = d; d += 3 * n;
    W.glat = d; d += PCI_LMAX * n;
    int *i = (int *)d;
    W.counts = i; i += nwg;
    W.offs = i; i += nwg;
    W.total = i; i += 2;
    W.qlat = i; i += n;
    W.qsrc = i;
    return W;
}

}  // namespace

extern "C" {

size_t dss_pointcloud_loss_igr_workspace_bytes(int nseg, int max_seg_len, int n_pts)
{
    if (nseg <= 0 || max_seg_len <= 0 || n_pts <= 0) return 0;
    return pci_layout(nullptr, nseg, max_seg_len, n_pts).bytes;
}

int dss_pointcloud_loss_igr(const DssIgrNet *net, int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose,
                            const double *scale, const int *lat_idx, const double *latents, int lat_stride, int n_pts, double *out,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    if (!net || !net->W0 || !net->b0 || !net->Wp || !net->bh || !net->W8 || !net->b8) return DSS_E_BADARG;
    if (nseg <= 0 || max_seg_len < 0 || n_pts < 0 || !seg_off || !pose || !scale || !lat_idx || !latents || !out) return DSS_E_BADARG;
    if (max_seg_len > 0 && n_pts > 0 && !pts) return DSS_E_BADARG;
    const int L = igr_net_latent(*net);
    if (L < 0) return DSS_E_UNSUPPORTED;
    if (lat_stride < L) return DSS_E_BADARG;
    if (n_pts == 0) max_seg_len = 0;      // (no row of pts may be named: every segment is empty)
    if ((long long)nseg * (pc_chunks(max_seg_len) > 0 ? pc_chunks(max_seg_len) : 1) > 0x7fffffffLL / PCI_OUT || n_pts > 0x7fffffff / 12)
        return DSS_E_UNSUPPORTED;      // grid.x and the int indices nseg * chunks * 13, 3 n_pts, 4 n_pts
    const size_t need = dss_pointcloud_loss_igr_workspace_bytes(nseg, max_seg_len, n_pts);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DSS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = pc_chunks(max_seg_len), nwg = chunks * nseg;
    const PciWorkspace W = pci_layout(workspace, nseg, max_seg_len, n_pts);
    if (chunks > 0) {
        hipLaunchKernelGGL(pci_count_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, seg_off, pts, pose, scale, W.counts);
        hipLaunchKernelGGL(chunk_scan_kernel<>, dim3(1), dim3(CG_THREADS), 0, st, nwg, n_pts, (const int *)W.counts, W.offs, W.total);
        hipLaunchKernelGGL(pci_emit_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, n_pts, seg_off, pts, pose, scale, lat_idx,
                           (const int *)W.offs, W.qpts, W.qlat, W.qsrc);
        // The list's length decides the network's grid and workgroup shape, and it is usually far below n_pts (the part of the
        // clouds inside the cubes): the host reads it -- one int, the call's only wait -- and launches for exactly that many points.
        HostInts host_total;
        if (!host_total.copy(W.total, 1, st) || !host_sync(st)) return DSS_E_BADARG;      // (as dss_pointcloud_loss reports its read)
        const int total = host_total.p[0];
        if (total > 0) {
            int rc = dss::launch_igr_list(*net, W.qpts, W.qlat, latents, lat_stride, nullptr, total, DSS_IGR_XYZ, W.sdf, W.gxyz, st, -1);
            if (rc == DSS_OK)
                rc = dss::launch_igr_list(*net, W.qpts, W.qlat, latents, lat_stride, nullptr, total, DSS_IGR_LATENT, W.sdf, W.glat, st, -1);      // (writes the same values again)
            if (rc != DSS_OK) return rc;
        }
        hipLaunchKernelGGL(pci_reduce_kernel, dim3(nwg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, n_pts, L, L > 3 ? L : 3, seg_off, pts,
                           pose, scale, (const int *)W.counts, (const int *)W.offs, (const int *)W.qsrc, (const double *)W.sdf,
                           (const double *)W.gxyz, (const double *)W.glat, W.partial);
    }
    hipLaunchKernelGGL(segment_sum_kernel<PCI_OUT>, dim3((nseg * PCI_OUT + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, st, nseg, max_seg_len,
                       chunks, seg_off, (const double *)W.partial, out);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
