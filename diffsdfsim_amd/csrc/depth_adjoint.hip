// depth_adjoint.hip -- the depth camera's derivative: d depth / d (pose, shape parameters, grid samples) of the images that
// dss_depth_render / dss_depth_render_grids (depth_camera.hip) return, contracted with the adjoint of depth.  ABI, the formula and
// what it leaves out (silhouette motion): depth_adjoint.h.  The terms of one hit point: depth_adjoint_point.h.
//
//   depth_adjoint_kernel       the renderer's launch shape (depth_trace.h: a pixel per lane, an 8 x 8 tile per wavefront, 2 x 2 of
//                              them per 256-thread workgroup).  The workgroup's first nbody threads build the view's bodies in LDS
//                              as PcSegment (R, 2 / q.q, Shape<PcDual> with the three parameters seeded), once, not per lane.  A
//                              lane recomputes its hit point o + t d_w, evaluates its own body (the one its seg names: no loop
//                              over bodies here) and holds ten terms and a dropped flag.  Then, per body, the terms of the lanes
//                              whose seg is that body are added by a wavefront butterfly (a wavefront none of whose lanes saw the
//                              body writes zeros without one) and by a fixed tree over the four wavefronts in LDS: one partial
//                              [nbody][11] per workgroup in the workspace.  The loop over bodies selects among the lane's eleven
//                              numbers; it keeps no state per body.
//   depth_adjoint_sum_kernel   a wavefront per (view, body): lane l adds the partials of tiles l, l + 64, ... in that order, then
//                              the butterfly.  No atomics on this path: the order is a function of the launch shape alone.
//
// Grid samples: a lane adds its eight terms with the hardware's fp64 global atomic add (-munsafe-fp-atomics), as
// pointcloud_loss_grid_adj.hip does; the order of the adds into one sample is the order of arrival.
#include "depth_trace.h"
#include "shape_args.h"
#include "depth_adjoint.h"
#include "depth_adjoint_point.h"

namespace {

constexpr int DA_TERMS = DA_OUT + 1;      // the ten derivatives and the dropped count (a whole number, exact in a double)
constexpr int DA_SEG_DOUBLES = (sizeof(PcSegment) + sizeof(double) - 1) / sizeof(double);

// a body's grid in the view's table: its samples, where their adjoint goes (NULL: not wanted), its dims; data == NULL: none
struct DaGrid {
    const double *data;
    double *adj;
    int n[3];
};

template <bool GRIDS>
__global__ void __launch_bounds__(DC_THREADS) depth_adjoint_kernel(int nbody, int tiles_x, int tiles_per_view, const double *__restrict__ pose,
                                                                  const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                  const double *__restrict__ cam, double fx, double fy, double cx, double cy,
                                                                  int W, int H, const double *__restrict__ depth, const int *__restrict__ seg,
                                                                  const double *__restrict__ g_depth, double min_cos,
                                                                  const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                                                  const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                  double *__restrict__ g_grid, double *__restrict__ partial)
{
    // (PcSegment has constructors, which LDS objects may not: the table lives in plain doubles)
    __shared__ double seg_store[DC_MAX_BODY * DA_SEG_DOUBLES];
    __shared__ DaGrid gtab[DC_MAX_BODY];
    __shared__ double red[DC_MAX_BODY][DC_THREADS / WAVE][DA_TERMS];
    PcSegment *segs = reinterpret_cast<PcSegment *>(seg_store);
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    if (tid < nbody) {
        const size_t b = (size_t)view * nbody + tid;
        const int ty = shape_type[b];
        pc_segment(segs[tid], pose + 7 * b, ty, prm + 4 * b);
        if (GRIDS) {
            const int g = (ty == SHAPE_GRID || ty == SHAPE_IGR) ? grid_id[b] : -1;      // (< ngrid: the launcher has checked)
            DaGrid &G = gtab[tid];
            G.data = g >= 0 ? grid_data + grid_off[g] : nullptr;
            G.adj = (g >= 0 && g_grid) ? g_grid + grid_off[g] : nullptr;
            for (int i = 0; i < 3; ++i) G.n[i] = g >= 0 ? grid_dims[3 * g + i] : 2;
        }
    }
    __syncthreads();

    int col, row;
    dc_pixel_of(tile_x, tile_y, tid, col, row);
    double term[DA_OUT], drop = 0.0;
#pragma unroll
    for (int k = 0; k < DA_OUT; ++k) term[k] = 0.0;
    int who = -1;      // (no early return: every lane takes part in the reductions below)
    if (col < W && row < H) {
        const size_t px = ((size_t)view * H + row) * W + col;
        const int s = seg[px];
        if (s >= 0 && s < nbody) {
            who = s;
            const double t = depth[px], gd = g_depth[px];
            double o[3], d[3], inv_len;
            dc_ray(cam, fx, fy, cx, cy, col, row, o, d, inv_len);
            const double x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
            const PcSegment &S = segs[s];
            double e[3], pb[3], db[3];
            pc_body_point(S, x, e, pb);
#pragma unroll
            for (int i = 0; i < 3; ++i) db[i] = S.R[i] * d[0] + S.R[3 + i] * d[1] + S.R[6 + i] * d[2];      // R^T d_w
            double phi = 0.0, g[3] = {0.0, 0.0, 0.0}, gprm[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
            int i0[3] = {0, 0, 0};
            bool ok = false, on_grid = false;
            if (GRIDS && gtab[s].data) {
                on_grid = true;
                ok = da_grid(gtab[s].data, gtab[s].n, val(S.shape.scale), pb, i0, w, phi, g);
            } else {
                switch (S.shape.type) {
                case SHAPE_BOX: ok = da_analytic<SHAPE_BOX>(S, pb, phi, g, gprm); break;
                case SHAPE_SPHERE: ok = da_analytic<SHAPE_SPHERE>(S, pb, phi, g, gprm); break;
                case SHAPE_CYLINDER: ok = da_analytic<SHAPE_CYLINDER>(S, pb, phi, g, gprm); break;
                case SHAPE_BOX_ROUNDED: ok = da_analytic<SHAPE_BOX_ROUNDED>(S, pb, phi, g, gprm); break;
                default: break;      // (the launcher has refused every other type)
                }
            }
            // n_w . d_w = (R g) . d_w = g . R^T d_w, |n_w| = |g|, |d_w| = 1 / inv_len
            const double nd = g[0] * db[0] + g[1] * db[1] + g[2] * db[2];
            const double cosine = fabs(nd) * inv_len / sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            if (ok && cosine >= min_cos && nd != 0.0) {      // (a NaN fails the comparison)
                const double k = -gd / nd;
                const double gs[3] = {k * g[0], k * g[1], k * g[2]};
                da_pose_chain(S, e, pb, gs, term);
#pragma unroll
                for (int i = 0; i < 3; ++i) term[7 + i] = k * gprm[i];
                if (GRIDS && on_grid && gtab[s].adj) {
                    double *A = gtab[s].adj;
                    const int n1 = gtab[s].n[1], n2 = gtab[s].n[2];
                    const double ks = k * val(S.shape.scale);
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                            for (int dz = 0; dz < 2; ++dz)
                                atomicAdd(A + ((size_t)(i0[0] + dx) * n1 + i0[1] + dy) * n2 + i0[2] + dz, ks * grid_corner_weight(w, dx, dy, dz));
                }
            } else {
                drop = 1.0;
            }
        }
    }

    const int wave = tid / WAVE, lane = lane_id();
    for (int j = 0; j < nbody; ++j) {
        const bool mine = who == j;
        if (__ballot(mine) == 0ull) {      // (the whole wavefront)
            if (lane < DA_TERMS) red[j][wave][lane] = 0.0;
            continue;
        }
#pragma unroll
        for (int k = 0; k < DA_OUT; ++k) {
            const double v = wave_sum(mine ? term[k] : 0.0);
            if (lane == 0) red[j][wave][k] = v;
        }
        const double v = wave_sum(mine ? drop : 0.0);
        if (lane == 0) red[j][wave][DA_OUT] = v;
    }
    __syncthreads();
    static_assert(DC_THREADS / WAVE == 4, "the tree below adds exactly four wavefronts");
    if (tid < nbody * DA_TERMS) {
        const int j = tid / DA_TERMS, k = tid - j * DA_TERMS;
        partial[((size_t)blockIdx.x * nbody + j) * DA_TERMS + k] = (red[j][0][k] + red[j][1][k]) + (red[j][2][k] + red[j][3][k]);
    }
}

__global__ void __launch_bounds__(WAVE) depth_adjoint_sum_kernel(int nbody, int tiles_per_view, const double *__restrict__ partial,
                                                                double *__restrict__ g_pose, double *__restrict__ g_prm,
                                                                int *__restrict__ dropped)
{
    const int vb = blockIdx.x, view = vb / nbody, j = vb - view * nbody, lane = threadIdx.x;
    for (int k = 0; k < DA_TERMS; ++k) {
        double acc = 0.0;
        for (int tile = lane; tile < tiles_per_view; tile += WAVE)
            acc += partial[(((size_t)view * tiles_per_view + tile) * nbody + j) * DA_TERMS + k];
        acc = wave_sum(acc);
        if (lane == 0) {
            if (k < 7) g_pose[7 * (size_t)vb + k] = acc;
            else if (k < DA_OUT) g_prm[3 * (size_t)vb + k - 7] = acc;
            else dropped[vb] = (int)acc;
        }
    }
}

}  // namespace

extern "C" {

size_t dss_depth_adjoint_workspace_bytes(int nview, int nbody, int W, int H)
{
    const DcLaunch L = dc_launch_shape(nview, nbody, W, H);
    if (nbody <= 0 || !L.ok) return 0;
    return (size_t)nview * L.tiles_per_view * nbody * DA_TERMS * sizeof(double);
}

int dss_depth_adjoint(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam, double fx,
                      double fy, double cx, double cy, int W, int H, const double *depth, const int *seg, const double *g_depth,
                      double min_cos, const int *grid_id, int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data,
                      double *g_pose, double *g_prm, double *g_grid, int *dropped, void *workspace, size_t workspace_bytes, void *stream)
{
    if (nview <= 0 || nbody <= 0 || W <= 0 || H <= 0 || !pose || !shape_type || !prm || !cam || !depth || !seg || !g_depth || !g_pose ||
        !g_prm || !dropped || ngrid < 0)
        return DSS_E_BADARG;
    if (ngrid > 0 && (!grid_id || !grid_off || !grid_dims || !grid_data)) return DSS_E_BADARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !(min_cos >= 0.0) || !(min_cos <= 1.0)) return DSS_E_BADARG;
    const DcLaunch L = dc_launch_shape(nview, nbody, W, H);
    if (!L.ok) return DSS_E_UNSUPPORTED;
    const size_t need = dss_depth_adjoint_workspace_bytes(nview, nbody, W, H);
    if (!workspace || workspace_bytes < need) return DSS_E_WORKSPACE;
    // Shape types, grid ids and the grids' dims decide the status, as in dss_shade_render: the host reads them first; without a
    // table (ngrid = 0) grid_id is not read, and a level-set body has no grid.
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    if (const int rc = judge_shapes((size_t)nview * nbody, shape_type, SHAPES_CONVEX, SHAPES_GRID_IGR, ngrid > 0 ? grid_id : nullptr, ngrid,
                                    grid_dims, st, &any))
        return rc;
    const int tiles_x = L.tiles_x, tiles_per_view = L.tiles_per_view;
    double *partial = (double *)workspace;
    if (any)
        hipLaunchKernelGGL(depth_adjoint_kernel<true>, dim3(tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, tiles_x, tiles_per_view,
                           pose, shape_type, prm, cam, fx, fy, cx, cy, W, H, depth, seg, g_depth, min_cos, grid_id, grid_off, grid_dims,
                           grid_data, g_grid, partial);
    else
        hipLaunchKernelGGL(depth_adjoint_kernel<false>, dim3(tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, tiles_x, tiles_per_view,
                           pose, shape_type, prm, cam, fx, fy, cx, cy, W, H, depth, seg, g_depth, min_cos, grid_id, grid_off, grid_dims,
                           grid_data, g_grid, partial);
    hipLaunchKernelGGL(depth_adjoint_sum_kernel, dim3(nview * nbody), dim3(WAVE), 0, st, nbody, tiles_per_view, (const double *)partial, g_pose,
                       g_prm, dropped);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
