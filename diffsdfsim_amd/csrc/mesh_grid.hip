// mesh_grid.hip -- closed triangle meshes to the samples of voxel grids: the exact signed distance of every sample to its mesh,
// for a batch of meshes in one call (the front door of SDFGrid3D.from_mesh).  ABI, geometry and the launcher's rule: mesh_grid.h.
//
//   mesh_grid_sdf_kernel   256-thread workgroups on a flat grid, ceil(max_samples / 256) per mesh; a lane per sample, lanes along
//                          the last grid axis, so the one store per lane coalesces.  The workgroup walks the mesh's faces MG_TILE
//                          at a time: thread t gathers triangle t of the tile through `faces` (three indices, each checked against
//                          [0, nv) before any vertex is read), classifies it (left out / regular / zero-area) and writes its nine
//                          coordinates to LDS as nine arrays; then every lane walks the tile reading the same address (a
//                          broadcast: no bank conflict; the class is uniform over the workgroup, so its branch does not diverge).
//                          Per pair: the closest point by region (selects, no divergent branch), the least squared distance, and
//                          the solid angle's atan2 added in face order.  One square root per sample at the end.
//
// All fp64 VALU work, O(samples x faces) per mesh; no atomics, so every output is a function of the input alone.
#include "../../include/diffsdfsim_hip.h"
#include "mesh_grid.h"
#include "dss_device.h"

namespace {

constexpr int MG_THREADS = 256, MG_TILE = DSS_MESH_GRID_TILE;
static_assert(MG_TILE == MG_THREADS, "a thread stages one triangle of a tile");
constexpr int MG_SKIP = 0, MG_REGULAR = 1, MG_FLAT = 2;      // a staged triangle's class
constexpr double MG_FLAT_SIN2 = 1e-20;                        // |ab x ac|^2 <= this * |ab|^2 |ac|^2: zero-area

// squared distance from the origin to the segment from p0 along e (p0: an end minus the sample)
__device__ __forceinline__ double mg_segment_d2(double px, double py, double pz, double ex, double ey, double ez)
{
    const double ee = ex * ex + ey * ey + ez * ez;
    double t = ee > 0.0 ? -(px * ex + py * ey + pz * ez) / ee : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double qx = px + t * ex, qy = py + t * ey, qz = pz + t * ez;
    return qx * qx + qy * qy + qz * qz;
}

__global__ void __launch_bounds__(MG_THREADS) mesh_grid_sdf_kernel(int blocks, int max_samples, int max_faces, const double *__restrict__ verts,
                                                                  const int *__restrict__ faces, const int *__restrict__ vert_off,
                                                                  const int *__restrict__ face_off, const int *__restrict__ grid_dims,
                                                                  const int *__restrict__ grid_off, const double *__restrict__ scale,
                                                                  double *__restrict__ grid_data, int *__restrict__ status)
{
    __shared__ double tri[9][MG_TILE];      // ax ay az bx by bz cx cy cz
    __shared__ int cls[MG_TILE];
    const int tid = threadIdx.x, m = blockIdx.x / blocks, blk = blockIdx.x - m * blocks;
    const int n0 = grid_dims[3 * m], n1 = grid_dims[3 * m + 1], n2 = grid_dims[3 * m + 2];
    const long long all = (long long)n0 * n1 * n2;
    if (n0 < 2 || n1 < 2 || n2 < 2 || all > 0x7fffffffLL) {      // (the whole workgroup: no sample has a place)
        status[m] = DSS_MESH_GRID_MALFORMED;
        return;
    }
    const int nsamp = all < max_samples ? (int)all : max_samples;      // (the grid was sized for max_samples)
    if ((long long)blk * MG_THREADS >= nsamp) return;      // (the whole workgroup: this grid has no sample in the block)
    const int v0 = vert_off[m], nv = vert_off[m + 1] - v0, f0 = face_off[m];
    int nf = face_off[m + 1] - f0;
    nf = nf < max_faces ? nf : max_faces;
    if (nf <= 0) status[m] = DSS_MESH_GRID_MALFORMED;

    const int s = blk * MG_THREADS + tid, sc = s < nsamp ? s : nsamp - 1;      // (a lane past the end works on the last sample)
    const int i = sc / (n1 * n2), j = (sc - i * n1 * n2) / n2, k = sc - (i * n1 + j) * n2;
    const double h = scale[m];
    const double px = h * (-1.0 + 2.0 * i / (n0 - 1)), py = h * (-1.0 + 2.0 * j / (n1 - 1)), pz = h * (-1.0 + 2.0 * k / (n2 - 1));

    double best = __builtin_huge_val(), angle = 0.0;      // least squared distance; sum of half solid angles
    for (int t0 = 0; t0 < nf; t0 += MG_TILE) {
        const int n = nf - t0 < MG_TILE ? nf - t0 : MG_TILE;
        __syncthreads();      // (the previous tile has been read by every wavefront)
        if (tid < n) {
            const int *f = faces + 3 * (size_t)(f0 + t0 + tid);
            const int ia = f[0], ib = f[1], ic = f[2];
            int c = MG_SKIP;
            if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {
                const double *a = verts + 3 * (size_t)(v0 + ia), *b = verts + 3 * (size_t)(v0 + ib), *cc = verts + 3 * (size_t)(v0 + ic);
                const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = cc[0], cy = cc[1], cz = cc[2];
                tri[0][tid] = ax; tri[1][tid] = ay; tri[2][tid] = az;
                tri[3][tid] = bx; tri[4][tid] = by; tri[5][tid] = bz;
                tri[6][tid] = cx; tri[7][tid] = cy; tri[8][tid] = cz;
                const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
                const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                const double uu = ux * ux + uy * uy + uz * uz, ww = wx * wx + wy * wy + wz * wz;
                c = nx * nx + ny * ny + nz * nz <= MG_FLAT_SIN2 * uu * ww ? MG_FLAT : MG_REGULAR;
            } else {
                status[m] = DSS_MESH_GRID_MALFORMED;      // (the same value from whichever lane sees a bad face)
            }
            cls[tid] = c;
        }
        __syncthreads();
        for (int q = 0; q < n; ++q) {
            const int c = cls[q];
            if (c == MG_SKIP) continue;
            // the corners minus the sample
            const double ax = tri[0][q] - px, ay = tri[1][q] - py, az = tri[2][q] - pz;
            const double bx = tri[3][q] - px, by = tri[4][q] - py, bz = tri[5][q] - pz;
            const double cx = tri[6][q] - px, cy = tri[7][q] - py, cz = tri[8][q] - pz;
            const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;      // ab, ac
            if (c == MG_FLAT) {
                double d = mg_segment_d2(ax, ay, az, ux, uy, uz);
                const double e = mg_segment_d2(ax, ay, az, wx, wy, wz), g = mg_segment_d2(bx, by, bz, cx - bx, cy - by, cz - bz);
                d = e < d ? e : d;
                d = g < d ? g : d;
                best = d < best ? d : best;
                continue;
            }
            // closest point a + v ab + w ac by region (ap = -a: the sample is the origin)
            const double d1 = -(ux * ax + uy * ay + uz * az), d2 = -(wx * ax + wy * ay + wz * az);
            const double d3 = -(ux * bx + uy * by + uz * bz), d4 = -(wx * bx + wy * by + wz * bz);
            const double d5 = -(ux * cx + uy * cy + uz * cz), d6 = -(wx * cx + wy * cy + wz * cz);
            const double va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
            const double inv = 1.0 / (va + vb + vc);
            double v = vb * inv, w = vc * inv;                                            // face
            const double e43 = d4 - d3, e56 = d5 - d6;
            if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) { w = e43 / (e43 + e56); v = 1.0 - w; }      // edge bc
            if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }               // edge ac
            if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }                                      // vertex c
            if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }               // edge ab
            if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }                                      // vertex b
            if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }                                     // vertex a
            const double qx = ax + v * ux + w * wx, qy = ay + v * uy + w * wy, qz = az + v * uz + w * wz;
            const double d = qx * qx + qy * qy + qz * qz;
            best = d < best ? d : best;
            // half the solid angle
            const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz), lc = sqrt(cx * cx + cy * cy + cz * cz);
            const double num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
            const double den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la +
                               (cx * ax + cy * ay + cz * az) * lb;
            angle += atan2(num, den);
        }
    }
    if (s < nsamp) {
        const double wind = angle * 0.15915494309189535;      // 2 angle / (4 pi)
        const double dist = sqrt(best) / h;
        grid_data[(size_t)grid_off[m] + s] = wind > 0.5 ? -dist : dist;
    }
}

}  // namespace

extern "C" {

int dss_mesh_grid_sdf(int nmesh, const double *verts, const int *faces, const int *vert_off, const int *face_off, const int *grid_dims,
                      const int *grid_off, const double *scale, int max_samples, int max_faces, double *grid_data, int *status,
                      void *stream)
{
    if (nmesh <= 0 || max_samples <= 0 || max_faces <= 0 || !verts || !faces || !vert_off || !face_off || !grid_dims || !grid_off ||
        !scale || !grid_data || !status)
        return DSS_E_BADARG;
    const long long blocks = ((long long)max_samples + MG_THREADS - 1) / MG_THREADS, lim = 0x7fffffffLL;
    if ((long long)nmesh * blocks * MG_THREADS > lim) return DSS_E_UNSUPPORTED;      // (bounds the grid and nmesh * max_samples)
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)nmesh * sizeof(int), st) != hipSuccess) return DSS_E_UNSUPPORTED;
    hipLaunchKernelGGL(mesh_grid_sdf_kernel, dim3((unsigned)(nmesh * blocks)), dim3(MG_THREADS), 0, st, (int)blocks, max_samples, max_faces,
                       verts, faces, vert_off, face_off, grid_dims, grid_off, scale, grid_data, status);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
