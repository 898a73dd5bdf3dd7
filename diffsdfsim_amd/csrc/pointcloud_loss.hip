// pointcloud_loss.hip -- the point-cloud loss of experiments/trajectory_fitting/optim_pointcloud.py (`match_pointcloud`,
// :166-201) for a batch of (scene, observed frame) segments, value and Jacobian in one pass.
//
//   dss_pointcloud_loss   per segment s: out[s] = sum over its points inside the body's query cube of
//                         (phi^2, 1, d phi^2 / d pose[7], d phi^2 / d prm[3])   (pointcloud_point.h)
//   dss_pointcloud_loss_grids   the same with voxel-grid segments (SHAPE_GRID) from a pooled grid table: a kernel of its own,
//                         the analytic loops shared
//
// One lane per point in a strided loop over the chunk grid of chunk_grid.h (a workgroup per (segment, 2048 consecutive points of
// it)).  Each lane keeps the twelve partial sums in registers; block_sum writes the workgroup's partial [12] into the workspace and
// segment_sum_kernel adds a segment's partials in index order.  No atomics anywhere: the summation order is a function of the
// launch shape alone, so two calls on the same input return the same bits.
// 24 B read per point against ~1 500 fp64 instructions (the dual-number SDF): VALU-bound, like dss_sdf_query.
#include "../../include/diffsdfsim_hip.h"
#include "shape_args.h"
#include "chunk_grid.h"
#include "../../include/pointcloud_loss.h"
#include "pointcloud_point.h"

namespace {
using namespace dss;

// the strided loop of one lane over its points of the chunk, for a segment whose body is of type TYPE
template <int TYPE> __device__ __forceinline__ void pc_accumulate(const double *__restrict__ P, int i0, int hi, const double *pose,
                                                                  const double *prm4, double *acc)
{
    PcSegment S;
    pc_segment(S, pose, TYPE, prm4);
    for (int i = i0; i < hi; i += CG_THREADS) {
        const double x[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
        double term[PC_OUT];
        if (pc_point(S, x, term)) {
#pragma unroll
            for (int k = 0; k < PC_OUT; ++k) acc[k] += term[k];
        }
    }
}

// the segment's shape is the same for the whole workgroup: one loop per primitive, each compiled for its type alone
__device__ __forceinline__ bool pc_analytic(int type, const double *__restrict__ P, int i0, int hi, const double *ps, const double *pr, double *acc)
{
    switch (type) {
    case SHAPE_BOX: pc_accumulate<SHAPE_BOX>(P, i0, hi, ps, pr, acc); break;
    case SHAPE_SPHERE: pc_accumulate<SHAPE_SPHERE>(P, i0, hi, ps, pr, acc); break;
    case SHAPE_CYLINDER: pc_accumulate<SHAPE_CYLINDER>(P, i0, hi, ps, pr, acc); break;
    case SHAPE_BOX_ROUNDED: pc_accumulate<SHAPE_BOX_ROUNDED>(P, i0, hi, ps, pr, acc); break;
    case SHAPE_BRICK: pc_accumulate<SHAPE_BRICK>(P, i0, hi, ps, pr, acc); break;
    case SHAPE_BOWL: pc_accumulate<SHAPE_BOWL>(P, i0, hi, ps, pr, acc); break;
    default: return false;
    }
    return true;
}

__global__ void __launch_bounds__(CG_THREADS) pointcloud_loss_kernel(int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                    const double *__restrict__ pts, const double *__restrict__ pose,
                                                                    const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                    double *__restrict__ partial)
{
    __shared__ double red[CG_WAVES][PC_OUT];
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    double acc[PC_OUT];
#pragma unroll
    for (int k = 0; k < PC_OUT; ++k) acc[k] = 0.0;
    if (!pc_analytic(shape_type[s], pts + 3 * (size_t)first, lo + (int)threadIdx.x, hi, pose + 7 * (size_t)s, prm + 4 * (size_t)s, acc))
        return;      // (neural and grid bodies: the launcher has refused them)
    block_sum<PC_OUT>(acc, red, partial + (size_t)blockIdx.x * PC_OUT);
}

// The same with voxel-grid segments: type SHAPE_GRID reads the segment's grid from the pooled table.  The value is geom.h's
// trilinear field and its tangent DiffGridSDF's rule as sdf_unit states it on duals (the once-normalised interpolated
// central-difference field, not the derivative of the interpolant); the scale is prm[3], a constant, so the three prm
// tangents stay exactly 0.  The grid pointer and dims go into the segment's Shape, the dual is not widened.
__global__ void __launch_bounds__(CG_THREADS) pointcloud_loss_grids_kernel(int max_seg_len, int chunks, const int *__restrict__ seg_off,
                                                                          const double *__restrict__ pts, const double *__restrict__ pose,
                                                                          const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                          const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                                                          const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                          double *__restrict__ partial)
{
    __shared__ double red[CG_WAVES][PC_OUT];
    int s, first, lo, hi;
    if (!pc_chunk(max_seg_len, chunks, seg_off, s, first, lo, hi)) return;
    double acc[PC_OUT];
#pragma unroll
    for (int k = 0; k < PC_OUT; ++k) acc[k] = 0.0;
    const double *P = pts + 3 * (size_t)first, *ps = pose + 7 * (size_t)s, *pr = prm + 4 * (size_t)s;
    const int type = shape_type[s];
    if (type == SHAPE_GRID) {
        const int g = grid_id[s];      // (>= 0 and < ngrid: the launcher has checked)
        PcSegment S;
        pc_segment(S, ps, SHAPE_GRID, pr);
        S.shape.grid = grid_data + grid_off[g];
        for (int i = 0; i < 3; ++i) S.shape.gn[i] = grid_dims[3 * g + i];
        for (int i = lo + (int)threadIdx.x; i < hi; i += CG_THREADS) {
            const double x[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
            double term[PC_OUT];
            if (pc_point(S, x, term)) {
#pragma unroll
                for (int k = 0; k < PC_OUT; ++k) acc[k] += term[k];
            }
        }
    } else if (!pc_analytic(type, P, lo + (int)threadIdx.x, hi, ps, pr, acc)) {
        return;      // (neural bodies: the launcher has refused them)
    }
    block_sum<PC_OUT>(acc, red, partial + (size_t)blockIdx.x * PC_OUT);
}

}  // namespace

extern "C" {

size_t dss_pointcloud_loss_workspace_bytes(int nseg, int max_seg_len)
{
    if (nseg <= 0 || max_seg_len <= 0) return 0;
    return (size_t)nseg * pc_chunks(max_seg_len) * PC_OUT * sizeof(double);
}

int dss_pointcloud_loss(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose, const int *shape_type,
                        const double *prm, double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (nseg <= 0 || max_seg_len < 0 || !seg_off || !pose || !shape_type || !prm || !out || (max_seg_len > 0 && !pts)) return DSS_E_BADARG;
    if ((long long)nseg * pc_chunks(max_seg_len) > 0x7fffffffLL / PC_OUT) return DSS_E_UNSUPPORTED;      // grid.x, int indices
    const size_t need = dss_pointcloud_loss_workspace_bytes(nseg, max_seg_len);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DSS_E_WORKSPACE;
    // the shape types decide the status (neural and grid bodies: not in this loss), so the host reads them before anything is enqueued
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = judge_shapes(nseg, shape_type, SHAPES_ANALYTIC, SHAPES_GRID, nullptr, 0, nullptr, st)) return rc;
    const int chunks = pc_chunks(max_seg_len);
    if (chunks > 0)
        hipLaunchKernelGGL(pointcloud_loss_kernel, dim3(chunks * nseg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, seg_off, pts, pose,
                           shape_type, prm, (double *)workspace);
    hipLaunchKernelGGL(segment_sum_kernel<PC_OUT>, dim3((nseg * PC_OUT + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, st, nseg,
                       max_seg_len, chunks, seg_off, (const double *)workspace, out);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_pointcloud_loss_grids(int nseg, int max_seg_len, const int *seg_off, const double *pts, const double *pose, const int *shape_type,
                              const double *prm, const int *grid_id, int ngrid, const int *grid_off, const int *grid_dims,
                              const double *grid_data, double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (nseg <= 0 || max_seg_len < 0 || !seg_off || !pose || !shape_type || !prm || !out || (max_seg_len > 0 && !pts) || !grid_id || ngrid < 0)
        return DSS_E_BADARG;
    if (ngrid > 0 && (!grid_off || !grid_dims || !grid_data)) return DSS_E_BADARG;
    if ((long long)nseg * pc_chunks(max_seg_len) > 0x7fffffffLL / PC_OUT) return DSS_E_UNSUPPORTED;      // grid.x, int indices
    const size_t need = dss_pointcloud_loss_workspace_bytes(nseg, max_seg_len);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DSS_E_WORKSPACE;
    // shape types, grid ids and the grids' dims decide the status: the host reads them before anything is enqueued
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = judge_shapes(nseg, shape_type, SHAPES_ANALYTIC, SHAPES_GRID, grid_id, ngrid, grid_dims, st)) return rc;
    const int chunks = pc_chunks(max_seg_len);
    if (chunks > 0)
        hipLaunchKernelGGL(pointcloud_loss_grids_kernel, dim3(chunks * nseg), dim3(CG_THREADS), 0, st, max_seg_len, chunks, seg_off, pts, pose,
                           shape_type, prm, grid_id, grid_off, grid_dims, grid_data, (double *)workspace);
    hipLaunchKernelGGL(segment_sum_kernel<PC_OUT>, dim3((nseg * PC_OUT + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, st, nseg,
                       max_seg_len, chunks, seg_off, (const double *)workspace, out);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
