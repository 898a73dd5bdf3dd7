// pointcloud_loss_grid_adj.hip -- the point-cloud loss of voxel-grid segments, differentiated with respect to the samples.
//
//   dss_pointcloud_loss_grids_adjoint   g_data[sample c of grid g] += sum over the segments s with grid_id[s] == g and their points
//                                       inside the query cube of  2 g_sum[s] phi scale w_c        (pointcloud_point.h: pc_grid_point)
//
// phi = scale * the trilinear value is linear in the eight samples of the point's cell, so this is the derivative of the value
// dss_pointcloud_loss_grids sums -- not DiffGridSDF's rule, which concerns the query point and stays what the pose Jacobian uses.
// The reference has no such derivative (DiffGridSDF.forward marks the samples non-differentiable).
//
// The forward's launch shape (chunk_grid.h): one lane per point, a workgroup per (segment, chunk of 2048 points).  A lane
// recomputes its point's cell, weights and phi and adds its eight terms with the hardware's fp64 global atomic add
// (-munsafe-fp-atomics: no compare-and-swap loop), as g_verts in step_bwd_all.hip and the 2-D grid adjoint do.  The order of the
// adds into one sample is the order of arrival: two calls agree to the rounding of an n-term sum, not in their bits.  Nothing is
// merged before the adds.
#include "../../include/diffsdfsim_hip.h"
#include "shape_args.h"
#include "chunk_grid.h"
#include "../../include/pointcloud_loss.h"
#include "pointcloud_point.h"

namespace {
using namespace dss;

__global__ void __launch_bounds__(CG_THREADS) pointcloud_grid_adjoint_kernel(int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                            const double *__restrict__ pts, const double *__restrict__ pose,
                                                                            const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                            const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                                                            const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                            const double *__restrict__ g_sum, double *__restrict__ g_data)
{
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    if (shape_type[s] != SHAPE_GRID) return;
    const int g = grid_id[s];      // (< ngrid: the launcher has checked)
    const double gs = g_sum[s];
    if (g < 0 || gs == 0.0) return;
    const double *P = pts + 3 * (size_t)first;
    PcSegment S;
    pc_segment(S, pose + 7 * (size_t)s, SHAPE_GRID, prm + 4 * (size_t)s);
    S.shape.grid = grid_data + grid_off[g];
    for (int i = 0; i < 3; ++i) S.shape.gn[i] = grid_dims[3 * g + i];
    double *G = g_data + grid_off[g];
    const int n1 = S.shape.gn[1], n2 = S.shape.gn[2];
    const double k0 = 2.0 * gs * val(S.shape.scale);
    for (int i = lo + (int)threadIdx.x; i < hi; i += CG_THREADS) {
        const double x[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
        int i0[3];
        double w[3], phi;
        if (!pc_grid_point(S, x, i0, w, phi)) continue;
        const double k = k0 * phi;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
                    atomicAdd(G + ((size_t)(i0[0] + dx) * n1 + i0[1] + dy) * n2 + i0[2] + dz, k * grid_corner_weight(w, dx, dy, dz));
    }
}

}  // namespace

extern "C" int dss_pointcloud_loss_grids_adjoint(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose,
                                                 const int *shape_type, const double *prm, const int *grid_id, int ngrid, const int *grid_off,
                                                 const int *grid_dims, const double *grid_data, const double *g_sum, double *g_data, void *stream)
{
    if (nseg <= 0 || max_seg_len < 0 || !seg_off || !pose || !shape_type || !prm || !g_sum || (max_seg_len > 0 && !pts) || !grid_id || ngrid < 0)
        return DSS_E_BADARG;
    if (ngrid > 0 && (!grid_off || !grid_dims || !grid_data || !g_data)) return DSS_E_BADARG;
    if ((long long)nseg * pc_chunks(max_seg_len) > 0x7fffffffLL / PC_OUT) return DSS_E_UNSUPPORTED;      // the forward's limit (grid.x, its partials)
    // shape types, grid ids and the grids' dims decide the status, as in dss_pointcloud_loss_grids: the host reads them first
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    if (const int rc = judge_shapes(nseg, shape_type, SHAPES_ANALYTIC, SHAPES_GRID, grid_id, ngrid, grid_dims, st, &any)) return rc;
    const int chunks = pc_chunks(max_seg_len);
    if (!any || chunks == 0) return DSS_OK;      // no grid segment, or no point: nothing to add
    hipLaunchKernelGGL(pointcloud_grid_adjoint_kernel, dim3(chunks * nseg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, seg_off, pts, pose,
                       shape_type, prm, grid_id, grid_off, grid_dims, grid_data, g_sum, g_data);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}
