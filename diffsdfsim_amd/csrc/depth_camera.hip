// depth_camera.hip -- the depth camera of experiments/trajectory_fitting/optim_pointcloud.py (Recorder3D with record_points
// and record_seg, sdf_physics/physics3d/utils.py) as a ray caster over the bodies' SDFs, and the selection of a body's
// observed points from its images (match_pointcloud, optim_pointcloud.py:168-187).  ABI and conventions: depth_camera.h.
//
//   dss_depth_render          a pixel per lane, an 8 x 8 pixel tile per wavefront, 2 x 2 of them per 256-thread workgroup
//                             (neighbouring rays meet the same body and take similar trip counts).  The workgroup's first
//                             nbody threads build the view's body table (R, pos, Shape<double>) in LDS.  Per body: ray into
//                             the body frame, slab test against the query cube (the cheap rejection), sphere tracing of
//                             query_sdf from the entry point; the nearest hit so far bounds the later bodies' traces.
//   dss_depth_render_grids    the same with voxel-grid bodies (SHAPE_GRID, and SHAPE_IGR seen through its value grid): a kernel
//                             of its own, the same per-pixel body compiled with the grid trace in it (dc_pixel<true>); a grid is
//                             walked cell by cell by a two-level 3-D DDA over the block minima of dss_grid_block_min
//   dss_grid_block_min        a thread per block of 4 x 4 x 4 cells: the least of its 5 x 5 x 5 corner samples
//   dss_depth_points_count    the row compaction of chunk_grid.h (a wavefront per image row) over dp_selected
//   dss_depth_points_emit     the same walk; writes the selected pixels' points in world coordinates
//
// fp64 VALU throughout; no atomics, so every output is a function of the input alone.
// The tables, the ray, the slab test and the traces are those of depth_trace.h, which the colour camera shares.
#include "chunk_grid.h"
#include "depth_trace.h"
#include "shape_args.h"

namespace {

// One pixel against the view's bodies (after the table's barrier).  GRIDS: bodies with a grid (gtab[j].data != NULL) are traced
// through it; without, gtab is not read and the code is that of the analytic renderer alone.
template <bool GRIDS> __device__ __forceinline__ void dc_pixel(const DcBody *tab, const DcGrid *gtab, int nbody, int view, int tile_x, int tile_y,
                                                               int tid, const double *__restrict__ cam, double fx, double fy, double cx,
                                                               double cy, int W, int H, double znear, double zfar,
                                                               double *__restrict__ depth, int *__restrict__ seg)
{
    int col, row;
    dc_pixel_of(tile_x, tile_y, tid, col, row);
    if (col >= W || row >= H) return;      // (no barrier below)
    double o[3], d[3], inv_len;
    dc_ray(cam, fx, fy, cx, cy, col, row, o, d, inv_len);
    double best = zfar;
    int who = -1;
    bool capped = false;
    for (int j = 0; j < nbody; ++j) {
        const DcBody &B = tab[j];
        double ob[3], db[3];
        double t0 = znear, t1 = best;      // within [znear, nearest hit so far]
        if (!dc_slab(B, o, d, ob, db, t0, t1)) continue;
        double t_hit = 0.0;
        const int got = dc_trace_body<GRIDS>(B, GRIDS ? gtab + j : nullptr, ob, db, inv_len, t0, t1, t_hit);
        if (got == DC_CAP) capped = true;
        else if (got == DC_HIT && t_hit < best) { best = t_hit; who = j; }      // a tie stays with the lower index
    }
    const size_t px = ((size_t)view * H + row) * W + col;
    depth[px] = (capped || who < 0) ? 0.0 : best;
    seg[px] = capped ? -2 : who;
}

__global__ void __launch_bounds__(DC_THREADS) depth_render_kernel(int nbody, int tiles_x, int tiles_per_view, const double *__restrict__ pose,
                                                                 const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                 const double *__restrict__ cam, double fx, double fy, double cx, double cy,
                                                                 int W, int H, double znear, double zfar, double *__restrict__ depth,
                                                                 int *__restrict__ seg)
{
    __shared__ DcBody tab[DC_MAX_BODY];
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    dc_table(tab, view, nbody, tid, pose, shape_type, prm);
    __syncthreads();
    dc_pixel<false>(tab, nullptr, nbody, view, tile_x, tile_y, tid, cam, fx, fy, cx, cy, W, H, znear, zfar, depth, seg);
}

// the same with the view's grid bodies: grid_id [nview][nbody] into the pooled table (checked by the launcher)
__global__ void __launch_bounds__(DC_THREADS) depth_render_grids_kernel(int nbody, int tiles_x, int tiles_per_view, const double *__restrict__ pose,
                                                                       const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                       const double *__restrict__ cam, double fx, double fy, double cx,
                                                                       double cy, int W, int H, double znear, double zfar,
                                                                       const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                                                       const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                       const int *__restrict__ blk_off, const double *__restrict__ blk_min,
                                                                       double *__restrict__ depth, int *__restrict__ seg)
{
    __shared__ DcBody tab[DC_MAX_BODY];
    __shared__ DcGrid gtab[DC_MAX_BODY];
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    dc_table(tab, view, nbody, tid, pose, shape_type, prm);
    dc_grid_table(gtab, view, nbody, tid, shape_type, grid_id, grid_off, grid_dims, grid_data, blk_off, blk_min);
    __syncthreads();
    dc_pixel<true>(tab, gtab, nbody, view, tile_x, tile_y, tid, cam, fx, fy, cx, cy, W, H, znear, zfar, depth, seg);
}

// blk_min of every block of every grid: a thread per block, the least of its (up to) 5 x 5 x 5 corner samples
__global__ void __launch_bounds__(DC_THREADS) grid_block_min_kernel(int ngrid, int nblk, const int *__restrict__ grid_off,
                                                                   const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                   const int *__restrict__ blk_off, double *__restrict__ blk_min)
{
    const int t = blockIdx.x * DC_THREADS + threadIdx.x;
    if (t >= nblk) return;
    int g = 0;
    while (g + 1 < ngrid && blk_off[g + 1] <= t) ++g;
    const int n0 = grid_dims[3 * g], n1 = grid_dims[3 * g + 1], n2 = grid_dims[3 * g + 2];
    const int nb1 = (n1 - 1 + GB - 1) / GB, nb2 = (n2 - 1 + GB - 1) / GB;
    const int r = t - blk_off[g], b0 = r / (nb1 * nb2), b1 = (r / nb2) % nb1, b2 = r % nb2;
    const int i1 = dc_imin(GB * b0 + GB, n0 - 1), j1 = dc_imin(GB * b1 + GB, n1 - 1), k1 = dc_imin(GB * b2 + GB, n2 - 1);
    const double *G = grid_data + grid_off[g];
    double m = G[((size_t)(GB * b0) * n1 + GB * b1) * n2 + GB * b2];
    for (int i = GB * b0; i <= i1; ++i)
        for (int j = GB * b1; j <= j1; ++j)
            for (int k = GB * b2; k <= k1; ++k) m = fmin(m, G[((size_t)i * n1 + j) * n2 + k]);
    blk_min[t] = m;
}

// is pixel (r, c) of the image at `base` an observed point of `body`: inside the mask eroded by one pixel, depth not 0
__device__ __forceinline__ bool dp_selected(const double *__restrict__ depth, const int *__restrict__ seg, size_t base, int W, int H,
                                            int r, int c, int body)
{
    if (r <= 0 || r >= H - 1 || c <= 0 || c >= W - 1) return false;      // the border has an unset neighbour
    const size_t i = base + (size_t)r * W + c;
    return seg[i] == body && seg[i - 1] == body && seg[i + 1] == body && seg[i - W] == body && seg[i + W] == body && depth[i] != 0.0;
}

__global__ void __launch_bounds__(CG_THREADS) depth_points_count_kernel(int nrow, int H, int W, int body, const double *__restrict__ depth,
                                                                       const int *__restrict__ seg, int *__restrict__ row_count)
{
    int g;
    if (!row_of_wave(nrow, g)) return;
    const int view = g / H, r = g - view * H;
    const size_t base = (size_t)view * H * W;
    const int n = dss::row_count(W, [&](int c) { return dp_selected(depth, seg, base, W, H, r, c, body); });
    if (lane_id() == 0) row_count[g] = n;
}

__global__ void __launch_bounds__(CG_THREADS) depth_points_emit_kernel(int nrow, int H, int W, int body, const double *__restrict__ depth,
                                                                      const int *__restrict__ seg, const int *__restrict__ row_off,
                                                                      const double *__restrict__ cam, double fx, double fy, double cx, double cy,
                                                                      double *__restrict__ pts)
{
    int g;
    if (!row_of_wave(nrow, g)) return;
    const int view = g / H, r = g - view * H;
    const size_t base = (size_t)view * H * W;
    const double ny = (r + 0.5 - cy) / fy;
    row_emit(W, row_off[g], [&](int c) { return dp_selected(depth, seg, base, W, H, r, c, body); }, [&](int slot, int c) {
        const double dz = depth[base + (size_t)r * W + c], nx = (c + 0.5 - cx) / fx;
        const double x = nx * dz, y = -(ny * dz), z = -dz;      // OpenGL camera frame: y and z flipped
        double *out = pts + 3 * (size_t)slot;
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = cam[4 * i] * x + cam[4 * i + 1] * y + cam[4 * i + 2] * z + cam[4 * i + 3];
    });
}

}  // namespace

extern "C" {

int dss_depth_render(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam, double fx,
                     double fy, double cx, double cy, int W, int H, double znear, double zfar, double *depth, int *seg, void *stream)
{
    if (nview <= 0 || nbody <= 0 || W <= 0 || H <= 0 || !pose || !shape_type || !prm || !cam || !depth || !seg) return DSS_E_BADARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !(znear >= 0.0) || !(znear < zfar)) return DSS_E_BADARG;
    const DcLaunch L = dc_launch_shape(nview, nbody, W, H);
    if (!L.ok) return DSS_E_UNSUPPORTED;
    // The shape types decide the status, so the host reads them before anything is enqueued.  Brick, bowl: not shown to bound the
    // distance; neural and grid bodies: not in this renderer (no table: a level-set body has no grid).
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = judge_shapes((size_t)nview * nbody, shape_type, SHAPES_CONVEX, SHAPES_GRID_IGR, nullptr, 0, nullptr, st)) return rc;
    hipLaunchKernelGGL(depth_render_kernel, dim3(L.tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, L.tiles_x, L.tiles_per_view, pose,
                       shape_type, prm, cam, fx, fy, cx, cy, W, H, znear, zfar, depth, seg);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_grid_block_min(int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off, int nblk,
                       double *blk_min, void *stream)
{
    if (ngrid <= 0 || nblk <= 0 || !grid_off || !grid_dims || !grid_data || !blk_off || !blk_min) return DSS_E_BADARG;
    hipLaunchKernelGGL(grid_block_min_kernel, dim3((nblk + DC_THREADS - 1) / DC_THREADS), dim3(DC_THREADS), 0, (hipStream_t)stream, ngrid,
                       nblk, grid_off, grid_dims, grid_data, blk_off, blk_min);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_depth_render_grids(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam,
                           double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar, const int *grid_id,
                           int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off,
                           const double *blk_min, double *depth, int *seg, void *stream)
{
    if (nview <= 0 || nbody <= 0 || W <= 0 || H <= 0 || !pose || !shape_type || !prm || !cam || !depth || !seg || !grid_id || ngrid < 0)
        return DSS_E_BADARG;
    if (ngrid > 0 && (!grid_off || !grid_dims || !grid_data || !blk_off || !blk_min)) return DSS_E_BADARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !(znear >= 0.0) || !(znear < zfar)) return DSS_E_BADARG;
    const DcLaunch L = dc_launch_shape(nview, nbody, W, H);
    if (!L.ok) return DSS_E_UNSUPPORTED;
    // shape types, grid ids and the grids' dims decide the status, so the host reads them before anything is enqueued
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    if (const int rc = judge_shapes((size_t)nview * nbody, shape_type, SHAPES_CONVEX, SHAPES_GRID_IGR, grid_id, ngrid, grid_dims, st, &any))
        return rc;
    if (any)
        hipLaunchKernelGGL(depth_render_grids_kernel, dim3(L.tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, L.tiles_x,
                           L.tiles_per_view, pose, shape_type, prm, cam, fx, fy, cx, cy, W, H, znear, zfar, grid_id, grid_off, grid_dims,
                           grid_data, blk_off, blk_min, depth, seg);
    else      // no body is seen through a grid: the analytic renderer's own kernel, the same bits as dss_depth_render
        hipLaunchKernelGGL(depth_render_kernel, dim3(L.tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, L.tiles_x, L.tiles_per_view,
                           pose, shape_type, prm, cam, fx, fy, cx, cy, W, H, znear, zfar, depth, seg);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_depth_points_count(int nview, int H, int W, int body, const double *depth, const int *seg, int *row_count, void *stream)
{
    if (nview <= 0 || H <= 0 || W <= 0 || !depth || !seg || !row_count) return DSS_E_BADARG;
    if (!dc_images_ok(nview, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nview * H;
    hipLaunchKernelGGL(depth_points_count_kernel, dim3(row_blocks(nrow)), dim3(CG_THREADS), 0, (hipStream_t)stream, nrow, H, W, body,
                       depth, seg, row_count);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_depth_points_emit(int nview, int H, int W, int body, const double *depth, const int *seg, const int *row_off, const double *cam,
                          double fx, double fy, double cx, double cy, double *pts, void *stream)
{
    // (pts may be NULL: no pixel selected, nothing is written)
    if (nview <= 0 || H <= 0 || W <= 0 || !depth || !seg || !row_off || !cam || !(fx != 0.0) || !(fy != 0.0)) return DSS_E_BADARG;
    if (!dc_images_ok(nview, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nview * H;
    hipLaunchKernelGGL(depth_points_emit_kernel, dim3(row_blocks(nrow)), dim3(CG_THREADS), 0, (hipStream_t)stream, nrow, H, W, body,
                       depth, seg, row_off, cam, fx, fy, cx, cy, pts);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
