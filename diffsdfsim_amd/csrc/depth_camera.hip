// depth_camera.hip -- the depth camera of experiments/trajectory_fitting/optim_pointcloud.py (Recorder3D with record_points
// and record_seg, sdf_physics/physics3d/utils.py) as a ray caster over the bodies' SDFs, and the selection of a body's
// observed points from its images (match_pointcloud, optim_pointcloud.py:168-187).  ABI and conventions: depth_camera.h.
//
//   dss_depth_render          a pixel per lane, an 8 x 8 pixel tile per wavefront, 2 x 2 of them per 256-thread workgroup
//                             (neighbouring rays meet the same body and take similar trip counts).  The workgroup's first
//                             nbody threads build the view's body table (R, pos, Shape<double>) in LDS.  Per body: ray into
//                             the body frame, slab test against the query cube (the cheap rejection), sphere tracing of
//                             query_sdf from the entry point; the nearest hit so far bounds the later bodies' traces.
//   dss_depth_points_count    a wavefront per image row, 64 columns at a time: ballot of the selected pixels, popcount
//   dss_depth_points_emit     the same walk; a selected pixel's slot is the row's offset + the popcount of the lanes below it
//
// fp64 VALU throughout; no atomics, so every output is a function of the input alone.
#include <vector>

#include "../../include/diffsdfsim_hip.h"
#include "depth_camera.h"
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

__global__ void __launch_bounds__(DC_THREADS) depth_render_kernel(int nbody, int tiles_x, int tiles_per_view, const double *__restrict__ pose,
                                                                 const int *__restrict__ shape_type, const double *__restrict__ prm,
                                                                 const double *__restrict__ cam, double fx, double fy, double cx, double cy,
                                                                 int W, int H, double znear, double zfar, double *__restrict__ depth,
                                                                 int *__restrict__ seg)
{
    __shared__ DcBody tab[DC_MAX_BODY];
    const int view = blockIdx.x / tiles_per_view, tile = blockIdx.x - view * tiles_per_view;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x, tid = threadIdx.x;
    if (tid < nbody) {
        const size_t b = (size_t)view * nbody + tid;
        DcBody &B = tab[tid];
        quat_to_mat(pose + 7 * b, B.R);
        for (int i = 0; i < 3; ++i) B.pos[i] = pose[7 * b + 4 + i];
        make_shape(B.shape, shape_type[b], prm + 4 * b, prm[4 * b + 3]);
    }
    __syncthreads();
    const int wave = tid / WAVE, lane = tid & (WAVE - 1);
    const int col = tile_x * DC_TILE + (wave & 1) * 8 + (lane & 7), row = tile_y * DC_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (col >= W || row >= H) return;      // (no barrier below)
    // the pixel's ray in the world frame: origin = the camera's centre, direction = Rc (nx, -ny, -1), not normalised
    const double nx = (col + 0.5 - cx) / fx, ny = (row + 0.5 - cy) / fy;
    const double o[3] = {cam[3], cam[7], cam[11]};
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = cam[4 * i] * nx - cam[4 * i + 1] * ny - cam[4 * i + 2];
    const double inv_len = 1.0 / sqrt(nx * nx + ny * ny + 1.0);
    double best = zfar;
    int who = -1;
    bool capped = false;
    for (int j = 0; j < nbody; ++j) {
        const DcBody &B = tab[j];
        const double *R = B.R;
        const double e[3] = {o[0] - B.pos[0], o[1] - B.pos[1], o[2] - B.pos[2]};
        double ob[3], db[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {      // R^T e, R^T d
            ob[i] = R[i] * e[0] + R[3 + i] * e[1] + R[6 + i] * e[2];
            db[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
        }
        // slab test against |p| <= scale, within [znear, nearest hit so far]
        const double sc = B.shape.scale;
        double t0 = znear, t1 = best;
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
        if (miss || !(t0 <= t1)) continue;
        double t_hit = 0.0;
        int got = DC_MISS;
        switch (B.shape.type) {
        case SHAPE_BOX: got = dc_trace<SHAPE_BOX>(B, ob, db, inv_len, t0, t1, t_hit); break;
        case SHAPE_SPHERE: got = dc_trace<SHAPE_SPHERE>(B, ob, db, inv_len, t0, t1, t_hit); break;
        case SHAPE_CYLINDER: got = dc_trace<SHAPE_CYLINDER>(B, ob, db, inv_len, t0, t1, t_hit); break;
        case SHAPE_BOX_ROUNDED: got = dc_trace<SHAPE_BOX_ROUNDED>(B, ob, db, inv_len, t0, t1, t_hit); break;
        default: break;      // (the launcher has refused every other type)
        }
        if (got == DC_CAP) capped = true;
        else if (got == DC_HIT && t_hit < best) { best = t_hit; who = j; }      // a tie stays with the lower index
    }
    const size_t px = ((size_t)view * H + row) * W + col;
    depth[px] = (capped || who < 0) ? 0.0 : best;
    seg[px] = capped ? -2 : who;
}

// is pixel (r, c) of the image at `base` an observed point of `body`: inside the mask eroded by one pixel, depth not 0
__device__ __forceinline__ bool dp_selected(const double *__restrict__ depth, const int *__restrict__ seg, size_t base, int W, int H,
                                            int r, int c, int body)
{
    if (r <= 0 || r >= H - 1 || c <= 0 || c >= W - 1) return false;      // the border has an unset neighbour
    const size_t i = base + (size_t)r * W + c;
    return seg[i] == body && seg[i - 1] == body && seg[i + 1] == body && seg[i - W] == body && seg[i + W] == body && depth[i] != 0.0;
}

__global__ void __launch_bounds__(DC_THREADS) depth_points_count_kernel(int nrow, int H, int W, int body, const double *__restrict__ depth,
                                                                       const int *__restrict__ seg, int *__restrict__ row_count)
{
    const int g = blockIdx.x * (DC_THREADS / WAVE) + threadIdx.x / WAVE, lane = lane_id();
    if (g >= nrow) return;      // (the whole wavefront)
    const int view = g / H, r = g - view * H;
    const size_t base = (size_t)view * H * W;
    int n = 0;
    for (int c0 = 0; c0 < W; c0 += WAVE) n += __popcll(__ballot(dp_selected(depth, seg, base, W, H, r, c0 + lane, body)));
    if (lane == 0) row_count[g] = n;
}

__global__ void __launch_bounds__(DC_THREADS) depth_points_emit_kernel(int nrow, int H, int W, int body, const double *__restrict__ depth,
                                                                      const int *__restrict__ seg, const int *__restrict__ row_off,
                                                                      const double *__restrict__ cam, double fx, double fy, double cx, double cy,
                                                                      double *__restrict__ pts)
{
    const int g = blockIdx.x * (DC_THREADS / WAVE) + threadIdx.x / WAVE, lane = lane_id();
    if (g >= nrow) return;
    const int view = g / H, r = g - view * H;
    const size_t base = (size_t)view * H * W;
    const double ny = (r + 0.5 - cy) / fy;
    int at = row_off[g];
    for (int c0 = 0; c0 < W; c0 += WAVE) {
        const int c = c0 + lane;
        const bool sel = dp_selected(depth, seg, base, W, H, r, c, body);
        const unsigned long long mask = __ballot(sel);
        if (sel) {
            const double dz = depth[base + (size_t)r * W + c], nx = (c + 0.5 - cx) / fx;
            const double x = nx * dz, y = -(ny * dz), z = -dz;      // OpenGL camera frame: y and z flipped
            double *out = pts + 3 * (size_t)(at + __popcll(mask & ((1ull << lane) - 1ull)));
#pragma unroll
            for (int i = 0; i < 3; ++i) out[i] = cam[4 * i] * x + cam[4 * i + 1] * y + cam[4 * i + 2] * z + cam[4 * i + 3];
        }
        at += __popcll(mask);
    }
}

bool dc_images_ok(int nview, int H, int W) { return nview > 0 && H > 0 && W > 0 && (long long)nview * H * W <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int dss_depth_render(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam, double fx,
                     double fy, double cx, double cy, int W, int H, double znear, double zfar, double *depth, int *seg, void *stream)
{
    if (nview <= 0 || nbody <= 0 || W <= 0 || H <= 0 || !pose || !shape_type || !prm || !cam || !depth || !seg) return DSS_E_BADARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !(znear >= 0.0) || !(znear < zfar)) return DSS_E_BADARG;
    if (nbody > DC_MAX_BODY || !dc_images_ok(nview, H, W)) return DSS_E_UNSUPPORTED;
    const int tiles_x = (W + DC_TILE - 1) / DC_TILE, tiles_per_view = tiles_x * ((H + DC_TILE - 1) / DC_TILE);
    if ((long long)tiles_per_view * nview > 0x7fffffffLL) return DSS_E_UNSUPPORTED;      // grid.x
    // the shape types decide the status, so the host reads them before anything is enqueued
    hipStream_t st = (hipStream_t)stream;
    const size_t ntype = (size_t)nview * nbody;
#if defined(DSS_EMU)
    const int *types = shape_type;      // (the emulator's device memory is the host's)
#else
    std::vector<int> host_types(ntype);
    if (hipMemcpyAsync(host_types.data(), shape_type, sizeof(int) * ntype, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return DSS_E_BADARG;
    const int *types = host_types.data();
#endif
    for (size_t i = 0; i < ntype; ++i)
        if (types[i] != DSS_SHAPE_BOX && types[i] != DSS_SHAPE_SPHERE && types[i] != DSS_SHAPE_CYLINDER && types[i] != DSS_SHAPE_BOX_ROUNDED)
            return DSS_E_UNSUPPORTED;      // brick, bowl: not shown to bound the distance; neural and grid bodies: not in this renderer
    hipLaunchKernelGGL(depth_render_kernel, dim3(tiles_per_view * nview), dim3(DC_THREADS), 0, st, nbody, tiles_x, tiles_per_view, pose,
                       shape_type, prm, cam, fx, fy, cx, cy, W, H, znear, zfar, depth, seg);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_depth_points_count(int nview, int H, int W, int body, const double *depth, const int *seg, int *row_count, void *stream)
{
    if (nview <= 0 || H <= 0 || W <= 0 || !depth || !seg || !row_count) return DSS_E_BADARG;
    if (!dc_images_ok(nview, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nview * H, per = DC_THREADS / WAVE;
    hipLaunchKernelGGL(depth_points_count_kernel, dim3((nrow + per - 1) / per), dim3(DC_THREADS), 0, (hipStream_t)stream, nrow, H, W, body,
                       depth, seg, row_count);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

int dss_depth_points_emit(int nview, int H, int W, int body, const double *depth, const int *seg, const int *row_off, const double *cam,
                          double fx, double fy, double cx, double cy, double *pts, void *stream)
{
    // (pts may be NULL: no pixel selected, nothing is written)
    if (nview <= 0 || H <= 0 || W <= 0 || !depth || !seg || !row_off || !cam || !(fx != 0.0) || !(fy != 0.0)) return DSS_E_BADARG;
    if (!dc_images_ok(nview, H, W)) return DSS_E_UNSUPPORTED;
    const int nrow = nview * H, per = DC_THREADS / WAVE;
    hipLaunchKernelGGL(depth_points_emit_kernel, dim3((nrow + per - 1) / per), dim3(DC_THREADS), 0, (hipStream_t)stream, nrow, H, W, body,
                       depth, seg, row_off, cam, fx, fy, cx, cy, pts);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
