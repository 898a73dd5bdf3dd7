// depth_trace.h -- the ray tracing shared by the depth camera (depth_camera.hip) and the colour camera (shade_camera.hip):
// the view's body and grid tables in LDS, a pixel's ray, the slab test against a body's query cube, sphere tracing of the
// four convex primitives and the cell walk of a voxel grid.  Everything sits in an anonymous namespace: each of the two
// translation units compiles its own copy, and the operations are the same in both.
#pragma once
#include "../../include/diffsdfsim_hip.h"
#include "../../include/depth_camera.h"
#include "geom.h"
#include "wave_utils.h"

namespace {
using namespace dss;

constexpr int DC_THREADS = 256, DC_TILE = 16, DC_MAX_BODY = 8, DC_MAX_ITER = 512;
constexpr double DC_TAU = 1e-10;      // a hit: phi <= DC_TAU (world units)

struct DcBody {
    double R[9], pos[3];
    Shape<double> shape;
};

enum { DC_MISS = 0, DC_HIT = 1, DC_CAP = 2 };

// Sphere tracing of one body of type TYPE along p(t) = ob + t db (body frame) for t in [t0, t1], both inside the query cube.
// inv_len = 1 / |db|: phi is a distance, t counts depth.  p is clamped to the cube: the end points of the slab test may lie
// outside it by a rounding error, where query_sdf would return its constant (the fields are 1-Lipschitz, so the clamp moves
// phi by no more than it moves p).
// The four bodies are convex, so phi is convex along the ray and lies on or above the line through its last two samples
// beyond them: that line's zero is never past the surface, and never short of the plain step phi / |db| (the slope is at most
// |db|).  The trace takes the longer of the two -- on a plane it arrives in two steps, and at grazing incidence, where the
// plain step shrinks by the factor 1 - cos per iteration and needs log(1e10) / cos of them, it still converges within the
// cap.  A sample that is not below the one before it ends the trace: phi only grows from there on.
template <int TYPE> __device__ __forceinline__ int dc_trace(const DcBody &B, const double *ob, const double *db, double inv_len,
                                                            double t0, double t1, double &t_hit)
{
    Shape<double> s = B.shape;
    s.type = TYPE;      // (a constant: sdf_unit folds to this primitive's branch)
    const double sc = s.scale;
    double t = t0, t_prev = t0, phi_prev = 0.0;
    for (int it = 0; it < DC_MAX_ITER; ++it) {
        double p[3], phi, unused[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = fmin(fmax(ob[i] + t * db[i], -sc), sc);
        query_sdf(s, p, phi, unused, false);
        if (phi <= DC_TAU) { t_hit = t; return DC_HIT; }
        double step = phi * inv_len;
        if (it > 0) {
            if (phi >= phi_prev) return DC_MISS;
            step = fmax(step, phi * (t - t_prev) / (phi_prev - phi));
        }
        t_prev = t; phi_prev = phi;
        t += step;
        if (t > t1) return DC_MISS;
    }
    return DC_CAP;
}

// ---- voxel-grid bodies ---------------------------------------------------------------------------------------------------
constexpr int GB = DSS_GRID_BLOCK;      // cells per block edge of dss_grid_block_min

// a grid body of the view's table: its samples [n0][n1][n2] (x slowest), its block minima [nb0][nb1][nb2]; data == NULL: none
struct DcGrid {
    const double *data, *bmin;
    int n[3], nb[3];
};

// The trilinear field of one cell along the ray, from its 8 corners in registers: v[4 dx + 2 dy + dz], cell index c, index
// position xo + t xd.  (In units of the grid's samples: the caller compares with 0 only, the scale is positive.)
struct DcCell {
    double v[8];
    __device__ __forceinline__ void load(const double *__restrict__ g, int n1, int n2, int c0, int c1, int c2)
    {
        const double *p = g + ((size_t)c0 * n1 + c1) * n2 + c2;
        const size_t sx = (size_t)n1 * n2;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[n2]; v[3] = p[n2 + 1];
        v[4] = p[sx]; v[5] = p[sx + 1]; v[6] = p[sx + n2]; v[7] = p[sx + n2 + 1];
    }
    __device__ __forceinline__ double at(double w0, double w1, double w2) const
    {
        const double u2 = 1.0 - w2, u1 = 1.0 - w1;
        const double a = u2 * v[0] + w2 * v[1], b = u2 * v[2] + w2 * v[3], c = u2 * v[4] + w2 * v[5], d = u2 * v[6] + w2 * v[7];
        return (1.0 - w0) * (u1 * a + w1 * b) + w0 * (u1 * c + w1 * d);
    }
};

__device__ __forceinline__ int dc_floor_clamped(double u, int lo, int hi) { return (int)fmin(fmax(floor(u), (double)lo), (double)hi); }
__device__ __forceinline__ int dc_imin(int a, int b) { return a < b ? a : b; }

// One grid body along p(t) = ob + t db (body frame) for t in [t0, t1], both inside the query cube of half edge sc.
// Index position x_d(t) = xo_d + t xd_d = (p_d / sc + 1) / 2 (n_d - 1).  The ray is walked cell by cell; every plane crossing is
// computed from the plane's integer index, t = (k - xo_d) / xd_d, never by adding increments, and every iteration moves the cell
// index of one axis by at least one in the direction of the ray while no other axis moves back: at most n0 + n1 + n2 iterations,
// which is the loop's bound and not a cap (no status for it).  Blocks of GB cells whose corner minimum is positive are left in one
// iteration: the interpolant is a convex combination of a cell's corners, so such a block holds no zero, whatever the field.
// Invariant: the value at the entry of the current cell is > 0 (v_in; after a skipped block it is evaluated afresh).  The first
// cell whose exit value is <= 0 holds the hit: bisection on its 8 corners until the bracket is 4 ulp of t wide, at most 60
// halvings; the end whose value is <= 0 is returned.  A dip below zero inside one cell with both ends positive is not seen.
__device__ __forceinline__ int dc_trace_grid(const DcGrid &G, double sc, const double *ob, const double *db, double t0, double t1,
                                             double &t_hit)
{
    const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
    const double h0 = 0.5 * (n0 - 1), h1 = 0.5 * (n1 - 1), h2 = 0.5 * (n2 - 1);
    const double xo0 = (ob[0] / sc + 1.0) * h0, xo1 = (ob[1] / sc + 1.0) * h1, xo2 = (ob[2] / sc + 1.0) * h2;
    const double xd0 = db[0] / sc * h0, xd1 = db[1] / sc * h1, xd2 = db[2] / sc * h2;
    const int s0 = xd0 > 0.0 ? 1 : (xd0 < 0.0 ? -1 : 0), s1 = xd1 > 0.0 ? 1 : (xd1 < 0.0 ? -1 : 0), s2 = xd2 > 0.0 ? 1 : (xd2 < 0.0 ? -1 : 0);
    int c0 = dc_floor_clamped(xo0 + t0 * xd0, 0, n0 - 2), c1 = dc_floor_clamped(xo1 + t0 * xd1, 0, n1 - 2),
        c2 = dc_floor_clamped(xo2 + t0 * xd2, 0, n2 - 2);
    const double inf = 1.0 / 0.0;
    double t_in = t0, v_in = 0.0;
    bool fresh = true;      // v_in is not known for the current cell
    int last_blk = -1;
    DcCell cell;
    for (int it = 0, bound = n0 + n1 + n2; it <= bound; ++it) {
        const int b0 = c0 / GB, b1 = c1 / GB, b2 = c2 / GB, blk = (b0 * G.nb[1] + b1) * G.nb[2] + b2;
        bool skip = false;
        if (blk != last_blk) { last_blk = blk; skip = G.bmin[blk] > 0.0; }
        // the planes through which the ray leaves the cell (the block, if it is skipped), by their integer indices
        int k0, k1, k2;
        if (skip) {
            k0 = s0 > 0 ? dc_imin(GB * (b0 + 1), n0 - 1) : GB * b0;
            k1 = s1 > 0 ? dc_imin(GB * (b1 + 1), n1 - 1) : GB * b1;
            k2 = s2 > 0 ? dc_imin(GB * (b2 + 1), n2 - 1) : GB * b2;
        } else {
            k0 = c0 + (s0 > 0); k1 = c1 + (s1 > 0); k2 = c2 + (s2 > 0);
        }
        const double ta = s0 ? (k0 - xo0) / xd0 : inf, tb = s1 ? (k1 - xo1) / xd1 : inf, tc = s2 ? (k2 - xo2) / xd2 : inf;
        const int axis = (ta <= tb && ta <= tc) ? 0 : (tb <= tc ? 1 : 2);
        const double t_out = axis == 0 ? ta : (axis == 1 ? tb : tc);
        const double t_ex = fmin(fmax(t_out, t_in), t1);
        if (!skip) {
            cell.load(G.data, n1, n2, c0, c1, c2);
            if (fresh) {
                v_in = cell.at(xo0 + t_in * xd0 - c0, xo1 + t_in * xd1 - c1, xo2 + t_in * xd2 - c2);
                if (v_in <= 0.0) { t_hit = t_in; return DC_HIT; }      // the slab entry is inside the body (or the rounding of a block's face)
                fresh = false;
            }
            const double v_out = cell.at(xo0 + t_ex * xd0 - c0, xo1 + t_ex * xd1 - c1, xo2 + t_ex * xd2 - c2);
            if (v_out <= 0.0) {
                double lo = t_in, hi = t_ex;
                for (int h = 0; h < 60 && hi - lo > 8.881784197001252e-16 * hi; ++h) {      // 4 ulp: 4 * 2^-52 relative
                    const double mid = 0.5 * (lo + hi);
                    if (cell.at(xo0 + mid * xd0 - c0, xo1 + mid * xd1 - c1, xo2 + mid * xd2 - c2) <= 0.0) hi = mid; else lo = mid;
                }
                t_hit = hi;
                return DC_HIT;
            }
            v_in = v_out;
        } else {
            fresh = true;
        }
        if (!(t_out < t1)) return DC_MISS;      // the ray ends (the cube's far side, zfar or a nearer hit) inside this cell
        // into the next cell: one past the plane on the leaving axis; after a skipped block the other two from the position,
        // kept within the block and never behind where they were
        if (skip) {
            const double u0 = xo0 + t_ex * xd0, u1 = xo1 + t_ex * xd1, u2 = xo2 + t_ex * xd2;
            const int e0 = dc_imin(GB * b0 + GB - 1, n0 - 2), e1 = dc_imin(GB * b1 + GB - 1, n1 - 2), e2 = dc_imin(GB * b2 + GB - 1, n2 - 2);
            const int m0 = s0 > 0 ? dc_floor_clamped(u0, c0, e0) : (s0 < 0 ? dc_floor_clamped(u0, GB * b0, c0) : c0);
            const int m1 = s1 > 0 ? dc_floor_clamped(u1, c1, e1) : (s1 < 0 ? dc_floor_clamped(u1, GB * b1, c1) : c1);
            const int m2 = s2 > 0 ? dc_floor_clamped(u2, c2, e2) : (s2 < 0 ? dc_floor_clamped(u2, GB * b2, c2) : c2);
            c0 = axis == 0 ? (s0 > 0 ? k0 : k0 - 1) : m0;
            c1 = axis == 1 ? (s1 > 0 ? k1 : k1 - 1) : m1;
            c2 = axis == 2 ? (s2 > 0 ? k2 : k2 - 1) : m2;
        } else {
            c0 += axis == 0 ? s0 : 0; c1 += axis == 1 ? s1 : 0; c2 += axis == 2 ? s2 : 0;
        }
        if (c0 < 0 || c0 > n0 - 2 || c1 < 0 || c1 > n1 - 2 || c2 < 0 || c2 > n2 - 2) return DC_MISS;      // out of the grid
        t_in = t_ex;
    }
    return DC_MISS;      // (not reached: see the bound above)
}

// The view's body table in LDS, by the workgroup's first nbody threads (the caller's barrier follows).
__device__ __forceinline__ void dc_table(DcBody *tab, int view, int nbody, int tid, const double *__restrict__ pose,
                                         const int *__restrict__ shape_type, const double *__restrict__ prm)
{
    if (tid < nbody) {
        const size_t b = (size_t)view * nbody + tid;
        DcBody &B = tab[tid];
        quat_to_mat(pose + 7 * b, B.R);
        for (int i = 0; i < 3; ++i) B.pos[i] = pose[7 * b + 4 + i];
        make_shape(B.shape, shape_type[b], prm + 4 * b, prm[4 * b + 3]);
    }
}

// The view's grid table in LDS, by the same threads: grid_id [nview][nbody] into the pooled table (checked by the launcher).
__device__ __forceinline__ void dc_grid_table(DcGrid *gtab, int view, int nbody, int tid, const int *__restrict__ shape_type,
                                              const int *__restrict__ grid_id, const int *__restrict__ grid_off,
                                              const int *__restrict__ grid_dims, const double *__restrict__ grid_data,
                                              const int *__restrict__ blk_off, const double *__restrict__ blk_min)
{
    if (tid < nbody) {
        const int ty = shape_type[(size_t)view * nbody + tid];
        const int g = (ty == SHAPE_GRID || ty == SHAPE_IGR) ? grid_id[(size_t)view * nbody + tid] : -1;      // (an analytic body's id is not read)
        DcGrid &G = gtab[tid];
        G.data = g >= 0 ? grid_data + grid_off[g] : nullptr;
        G.bmin = g >= 0 ? blk_min + blk_off[g] : nullptr;
        for (int i = 0; i < 3; ++i) {
            G.n[i] = g >= 0 ? grid_dims[3 * g + i] : 2;
            G.nb[i] = (G.n[i] - 1 + GB - 1) / GB;
        }
    }
}

// The pixel of thread tid in the workgroup's 16 x 16 tile: an 8 x 8 tile per wavefront, 2 x 2 of them.
__device__ __forceinline__ void dc_pixel_of(int tile_x, int tile_y, int tid, int &col, int &row)
{
    const int wave = tid / WAVE, lane = tid & (WAVE - 1);
    col = tile_x * DC_TILE + (wave & 1) * 8 + (lane & 7);
    row = tile_y * DC_TILE + (wave >> 1) * 8 + (lane >> 3);
}

// The ray of pixel (row, col) in the world frame: origin o = the camera's centre, direction d = Rc (nx, -ny, -1), not
// normalised (a hit at parameter t has depth t); inv_len = 1 / |d|.
__device__ __forceinline__ void dc_ray(const double *__restrict__ cam, double fx, double fy, double cx, double cy, int col, int row,
                                       double *o, double *d, double &inv_len)
{
    const double nx = (col + 0.5 - cx) / fx, ny = (row + 0.5 - cy) / fy;
    o[0] = cam[3]; o[1] = cam[7]; o[2] = cam[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = cam[4 * i] * nx - cam[4 * i + 1] * ny - cam[4 * i + 2];
    inv_len = 1.0 / sqrt(nx * nx + ny * ny + 1.0);
}

// The ray o + t d in the frame of body B (ob = R^T (o - pos), db = R^T d) and its slab test against |p| <= scale within
// [t0, t1]: false if the ray misses the cube there, else [t0, t1] narrowed to the part inside it.
__device__ __forceinline__ bool dc_slab(const DcBody &B, const double *o, const double *d, double *ob, double *db, double &t0, double &t1)
{
    const double *R = B.R;
    const double e[3] = {o[0] - B.pos[0], o[1] - B.pos[1], o[2] - B.pos[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {      // R^T e, R^T d
        ob[i] = R[i] * e[0] + R[3 + i] * e[1] + R[6 + i] * e[2];
        db[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
    }
    const double sc = B.shape.scale;
    bool miss = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (db[i] != 0.0) {
            const double inv = 1.0 / db[i], ta = (-sc - ob[i]) * inv, tb = (sc - ob[i]) * inv;
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        } else if (fabs(ob[i]) > sc) {
            miss = true;
        }
    }
    return !(miss || !(t0 <= t1));
}

// One body along a ray that passed dc_slab.  GRIDS: a body with a grid (G && G->data) is traced through it.
template <bool GRIDS> __device__ __forceinline__ int dc_trace_body(const DcBody &B, const DcGrid *G, const double *ob, const double *db,
                                                                   double inv_len, double t0, double t1, double &t_hit)
{
    if (GRIDS && G->data) return dc_trace_grid(*G, B.shape.scale, ob, db, t0, t1, t_hit);
    switch (B.shape.type) {
    case SHAPE_BOX: return dc_trace<SHAPE_BOX>(B, ob, db, inv_len, t0, t1, t_hit);
    case SHAPE_SPHERE: return dc_trace<SHAPE_SPHERE>(B, ob, db, inv_len, t0, t1, t_hit);
    case SHAPE_CYLINDER: return dc_trace<SHAPE_CYLINDER>(B, ob, db, inv_len, t0, t1, t_hit);
    case SHAPE_BOX_ROUNDED: return dc_trace<SHAPE_BOX_ROUNDED>(B, ob, db, inv_len, t0, t1, t_hit);
    default: return DC_MISS;      // (the launcher has refused every other type)
    }
}

inline bool dc_images_ok(int nview, int H, int W) { return nview > 0 && H > 0 && W > 0 && (long long)nview * H * W <= 0x7fffffffLL; }

// The launch shape of the tiled camera kernels (a workgroup per DC_TILE x DC_TILE pixels of a view, grid.x = tiles_per_view * nview)
// and whether the compiled limits hold it: nbody, the pixels' int indices, grid.x.  Host code.
struct DcLaunch {
    int tiles_x, tiles_per_view;
    bool ok;
};
inline DcLaunch dc_launch_shape(int nview, int nbody, int W, int H)
{
    DcLaunch L = {0, 0, nbody <= DC_MAX_BODY && dc_images_ok(nview, H, W)};
    if (L.ok) {      // (the pixels fit an int, so the tiles do)
        L.tiles_x = (W - 1) / DC_TILE + 1;
        L.tiles_per_view = L.tiles_x * ((H - 1) / DC_TILE + 1);
        L.ok = (long long)L.tiles_per_view * nview <= 0x7fffffffLL;      // grid.x
    }
    return L;
}

}  // namespace
