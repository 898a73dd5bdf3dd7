// shade_camera.hip -- the colour camera: a deferred shading pass over the depth camera's images (what Recorder3D's
// renderer.render(scene, flags=SHADOWS_ALL) draws in sdf_physics/physics3d/utils.py, with the bodies' exact surfaces in place of
// pyrender's triangles and a stated shading model in place of its shaders).  ABI and the model: shade_camera.h.
//
//   dss_shade_render   a pixel per lane, mapped as in dss_depth_render (an 8 x 8 tile per wavefront, 2 x 2 of them per
//                      256-thread workgroup); the workgroup's first threads build the view's body table, its grid table and
//                      the normalised lights in LDS.  Per hit pixel: the point on the pixel's ray at the given depth, the
//                      body's gradient there (query_sdf, or the trilinear cell's closed form), and per light with n . l > 0 a
//                      shadow ray through every body by the traces of depth_trace.h; the loops over lights and bodies stay
//                      rolled.  Two kernels, as in the depth camera: with the grid trace compiled in, and without.
//
// fp64 VALU throughout; no atomics, so every output is a function of the input alone.
#include <math.h>

#include "depth_trace.h"
#include "shape_args.h"
#include "../../include/shade_camera.h"

namespace {

constexpr int SH_MAX_LIGHT = 4;
constexpr double SH_MIN_GRAD = 1e-300;

struct ShLight {
    double l[3], intensity;      // unit direction towards the light
};

// everything a pixel needs beyond the tables (one struct: the kernel's argument list stays readable)
struct ShArgs {
    const double *cam;
    double fx, fy, cx, cy;
    int W, H;
    double zfar;
    const double *depth;
    const int *seg;
    const double *color;
    double ambient, bg[3];
    int shadows;
    double bias;
    double *normal, *shade;
    unsigned char *rgb, *flags;
};

__device__ __forceinline__ unsigned char sh_level(double v) { return (unsigned char)fmin(fmax(floor(255.0 * v + 0.5), 0.0), 255.0); }

// The lights in LDS, by the workgroup's first nlight threads (the caller's barrier follows).  A direction of length 0 gives
// NaNs, whose cosine is not > 0: such a light adds nothing.
__device__ __forceinline__ void sh_light_table(ShLight *ltab, int nlight, int tid, const double *__restrict__ light)
{
    if (tid < nlight) {
        const double *l = light + 4 * tid;
        const double inv = 1.0 / sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
        for (int i = 0; i < 3; ++i) ltab[tid].l[i] = l[i] * inv;
        ltab[tid].intensity = l[3];
    }
}

// Body-frame gradient of grid G's trilinear interpolant at the body-frame point p (inside the query cube of half edge sc): the
// cell that holds p as geom.h's SHAPE_GRID branch picks it, d/dw of the interpolant from the 8 corners, times (n_d - 1) / 2 per
// axis (the common factor 1 / sc of the cell's size is dropped: the caller normalises).
__device__ __forceinline__ void sh_grid_grad(const DcGrid &G, double sc, const double *p, double *g)
{
    const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
    const double h0 = 0.5 * (n0 - 1), h1 = 0.5 * (n1 - 1), h2 = 0.5 * (n2 - 1);
    const double u0 = (p[0] / sc + 1.0) * h0, u1 = (p[1] / sc + 1.0) * h1, u2 = (p[2] / sc + 1.0) * h2;
    const int c0 = dc_floor_clamped(u0, 0, n0 - 2), c1 = dc_floor_clamped(u1, 0, n1 - 2), c2 = dc_floor_clamped(u2, 0, n2 - 2);
    const double w0 = u0 - c0, w1 = u1 - c1, w2 = u2 - c2, m0 = 1.0 - w0, m1 = 1.0 - w1, m2 = 1.0 - w2;
    DcCell cell;
    cell.load(G.data, n1, n2, c0, c1, c2);
    const double *v = cell.v;      // v[4 dx + 2 dy + dz]
    g[0] = h0 * (m1 * (m2 * (v[4] - v[0]) + w2 * (v[5] - v[1])) + w1 * (m2 * (v[6] - v[2]) + w2 * (v[7] - v[3])));
    g[1] = h1 * (m0 * (m2 * (v[2] - v[0]) + w2 * (v[3] - v[1])) + w0 * (m2 * (v[6] - v[4]) + w2 * (v[7] - v[5])));
    g[2] = h2 * (m0 * (m1 * (v[1] - v[0]) + w1 * (v[3] - v[2])) + w0 * (m1 * (v[5] - v[4]) + w1 * (v[7] - v[6])));
}

// One pixel (after the tables' barrier).  GRIDS as in dc_pixel.
template <bool GRIDS> __device__ __forceinline__ void sh_pixel(const DcBody *tab, const DcGrid *gtab, const ShLight *ltab, int nbody, int nlight,
                                                               int view, int tile_x, int tile_y, int tid, const ShArgs &A)
{
    int col, row;
    dc_pixel_of(tile_x, tile_y, tid, col, row);
    if (col >= A.W || row >= A.H) return;      // (no barrier below)
    const size_t px = ((size_t)view * A.H + row) * A.W + col;
    const int who = A.seg[px];
    if (who < 0 || who >= nbody) {      // nothing hit (-1), a capped trace (-2) or no body's index: the background
        for (int i = 0; i < 3; ++i) { A.normal[3 * px + i] = 0.0; A.rgb[3 * px + i] = sh_level(A.bg[i]); }
        A.shade[px] = 0.0;
        A.flags[px] = 0;
        return;
    }
    double o[3], d[3], inv_len;
    dc_ray(A.cam, A.fx, A.fy, A.cx, A.cy, col, row, o, d, inv_len);
    const double z = A.depth[px];
    double x[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = o[i] + z * d[i];
    const DcBody &B = tab[who];
    const double *R = B.R;
    const double sc = B.shape.scale, e[3] = {x[0] - B.pos[0], x[1] - B.pos[1], x[2] - B.pos[2]};
    double p[3], g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = fmin(fmax(R[i] * e[0] + R[3 + i] * e[1] + R[6 + i] * e[2], -sc), sc);
    if (GRIDS && gtab[who].data) {
        sh_grid_grad(gtab[who], sc, p, g);
    } else {
        double phi;
        query_sdf(B.shape, p, phi, g, true);
    }
    const double len = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    unsigned flag = 0;
    double n[3];
    if (!(len >= SH_MIN_GRAD)) {      // (a NaN comes here too)
        for (int i = 0; i < 3; ++i) n[i] = -(d[i] * inv_len);
        flag |= 2u;
    } else {
        const double nb[3] = {g[0] / len, g[1] / len, g[2] / len};
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i] = R[3 * i] * nb[0] + R[3 * i + 1] * nb[1] + R[3 * i + 2] * nb[2];
    }
    double so[3];      // where the shadow rays start
#pragma unroll
    for (int i = 0; i < 3; ++i) so[i] = x[i] + A.bias * n[i];
    double sum = 0.0;
#pragma nounroll
    for (int k = 0; k < nlight; ++k) {
        const double l[3] = {ltab[k].l[0], ltab[k].l[1], ltab[k].l[2]};
        const double c = n[0] * l[0] + n[1] * l[1] + n[2] * l[2];
        if (!(c > 0.0)) continue;
        bool lit = true;
        if (A.shadows) {
#pragma nounroll
            for (int j = 0; j < nbody; ++j) {
                double ob[3], db[3], t0 = 0.0, t1 = A.zfar, t_hit = 0.0;
                if (!dc_slab(tab[j], so, l, ob, db, t0, t1)) continue;
                const int got = dc_trace_body<GRIDS>(tab[j], GRIDS ? gtab + j : nullptr, ob, db, 1.0, t0, t1, t_hit);      // |l| = 1
                if (got == DC_HIT) { lit = false; break; }
                if (got == DC_CAP) flag |= 1u;
            }
        }
        if (lit) sum += ltab[k].intensity * c;
    }
    const double sh = fmin(1.0, A.ambient + sum);
    const double *colr = A.color + 3 * ((size_t)view * nbody + who);
    for (int i = 0; i < 3; ++i) { A.normal[3 * px + i] = n[i]; A.rgb[3 * px + i] = sh_level(colr[i] * sh); }
    A.shade[px] = sh;
    A.flags[px] = (unsigned char)flag;
}

__global__ void __launch_bounds__(DC_THREADS) shade_render_kernel(int nbody, int nlight, int tiles_x, int tiles_per_view,
                                                                 const double *__restrict__ pose, const int *__restrict__ shape_type,
                                                                 const double *__restrict__ prm, const double *__restrict__ light, ShArgs A)
{
    __shared__ DcBody tab[DC_MAX_BODY];
    __shared__ ShLight ltab[SH_MAX_LIGHT];
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    dc_table(tab, view, nbody, tid, pose, shape_type, prm);
    sh_light_table(ltab, nlight, tid, light);
    __syncthreads();
    sh_pixel<false>(tab, nullptr, ltab, nbody, nlight, view, tile_x, tile_y, tid, A);
}

__global__ void __launch_bounds__(DC_THREADS) shade_render_grids_kernel(int nbody, int nlight, int tiles_x, int tiles_per_view,
                                                                       const double *__restrict__ pose, const int *__restrict__ shape_type,
                                                                       const double *__restrict__ prm, const double *__restrict__ light,
                                                                       const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                                                       const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                                                       const int *__restrict__ blk_off, const double *__restrict__ blk_min, ShArgs A)
{
    __shared__ DcBody tab[DC_MAX_BODY];
    __shared__ DcGrid gtab[DC_MAX_BODY];
    __shared__ ShLight ltab[SH_MAX_LIGHT];
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    dc_table(tab, view, nbody, tid, pose, shape_type, prm);
    dc_grid_table(gtab, view, nbody, tid, shape_type, grid_id, grid_off, grid_dims, grid_data, blk_off, blk_min);
    sh_light_table(ltab, nlight, tid, light);
    __syncthreads();
    sh_pixel<true>(tab, gtab, ltab, nbody, nlight, view, tile_x, tile_y, tid, A);
}

}  // namespace

extern "C" int dss_shade_render(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam,
                                double fx, double fy, double cx, double cy, int W, int H, double zfar, const int *grid_id, int ngrid,
                                const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off,
                                const double *blk_min, const double *depth, const int *seg, const double *color, int nlight,
                                const double *light, double ambient, const double *background, int shadows, double shadow_bias,
                                double *normal, double *shade, unsigned char *rgb, unsigned char *flags, void *stream)
{
    if (nview <= 0 || nbody <= 0 || W <= 0 || H <= 0 || !pose || !shape_type || !prm || !cam || !depth || !seg || !color || !background ||
        !normal || !shade || !rgb || !flags || ngrid < 0)
        return DSS_E_BADARG;
    if (nlight < 0 || nlight > SH_MAX_LIGHT || (nlight > 0 && !light) || !(shadow_bias > 0.0)) return DSS_E_BADARG;
    if (ngrid > 0 && (!grid_id || !grid_off || !grid_dims || !grid_data || !blk_off || !blk_min)) return DSS_E_BADARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !(zfar > 0.0)) return DSS_E_BADARG;
    const DcLaunch L = dc_launch_shape(nview, nbody, W, H);
    if (!L.ok) return DSS_E_UNSUPPORTED;
    // Shape types, grid ids and the grids' dims decide the status, so the host reads them before anything is enqueued; without a
    // table (ngrid = 0) grid_id is not read, and a level-set body has no grid.
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    if (const int rc = judge_shapes((size_t)nview * nbody, shape_type, SHAPES_CONVEX, SHAPES_GRID_IGR, ngrid > 0 ? grid_id : nullptr, ngrid,
                                    grid_dims, st, &any))
        return rc;
    ShArgs A;
    A.cam = cam; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.W = W; A.H = H; A.zfar = zfar;
    A.depth = depth; A.seg = seg; A.color = color; A.ambient = ambient;
    for (int i = 0; i < 3; ++i) A.bg[i] = background[i];
    A.shadows = shadows != 0; A.bias = shadow_bias;
    A.normal = normal; A.shade = shade; A.rgb = rgb; A.flags = flags;
    if (any)
        hipLaunchKernelGGL(shade_render_grids_kernel, dim3(L.tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, nlight, L.tiles_x,
                           L.tiles_per_view, pose, shape_type, prm, light, grid_id, grid_off, grid_dims, grid_data, blk_off, blk_min, A);
    else
        hipLaunchKernelGGL(shade_render_kernel, dim3(L.tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, nlight, L.tiles_x,
                           L.tiles_per_view, pose, shape_type, prm, light, A);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}
