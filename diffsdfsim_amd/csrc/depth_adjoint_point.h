// depth_adjoint_point.h -- one hit point of the depth camera's adjoint (depth_adjoint.hip): the SDF phi itself (not phi^2, which
// is pointcloud_point.h's term) at a body-frame point, its gradient with respect to the point and the shape parameters, and the
// chain from the point to the body's pose.  Host and device; tests/emu/check_depth_adjoint.cpp holds 2 phi times these terms to
// pc_point's on the points it walks, so the two statements of the chain cannot drift apart unnoticed.
//
//   p = R(q)^T (x - pos),  F = phi(p; prm, samples)
//   d F / d pos = -R g                                       g = d phi / d p
//   d F / d q_k = s (d . dN/dq_k g) - s q_k (g . (p - d))    d = x - pos, s = 2 / (q.q), R = 1 + s N(q)   (pointcloud_point.h)
//   d F / d prm_i = the dual slot 3 + i (the corner radius and a grid's scale are constants of the body)
//   d F / d sample_c = scale * grid_corner_weight(w, c)      for the 8 corners of the point's cell
//
// For a grid body g is the gradient of the trilinear interpolant in the point's cell -- the field whose zero the camera's cell
// walk finds -- and not the central-difference field sdf_unit returns for grids.
#pragma once
#include "pointcloud_point.h"

namespace dss {

constexpr int DA_OUT = 10;      // d / d quat (4), d / d pos (3), d / d prm (3): the order of g_pose [7] followed by g_prm [3]

// the pose chain of the covector g (body frame) at d = x - pos, p = R^T d -> out[0..3] = d / d q, out[4..6] = d / d pos
__host__ __device__ inline void da_pose_chain(const PcSegment &S, const double *d, const double *p, const double *g, double *out)
{
    const double *R = S.R;
    const double r = S.q[0], qi = S.q[1], qj = S.q[2], qk = S.q[3];
    const double a00 = d[0] * g[0], a01 = d[0] * g[1], a02 = d[0] * g[2];
    const double a10 = d[1] * g[0], a11 = d[1] * g[1], a12 = d[1] * g[2];
    const double a20 = d[2] * g[0], a21 = d[2] * g[1], a22 = d[2] * g[2];
    const double sr = qk * (a10 - a01) + qj * (a02 - a20) + qi * (a21 - a12);
    const double si = qj * (a01 + a10) + qk * (a02 + a20) + r * (a21 - a12) - 2.0 * qi * (a11 + a22);
    const double sj = qi * (a01 + a10) + qk * (a12 + a21) + r * (a02 - a20) - 2.0 * qj * (a00 + a22);
    const double sk = qi * (a02 + a20) + qj * (a12 + a21) + r * (a10 - a01) - 2.0 * qk * (a00 + a11);
    const double gn = g[0] * (p[0] - d[0]) + g[1] * (p[1] - d[1]) + g[2] * (p[2] - d[2]);
    out[0] = S.two_s * (sr - r * gn);
    out[1] = S.two_s * (si - qi * gn);
    out[2] = S.two_s * (sj - qj * gn);
    out[3] = S.two_s * (sk - qk * gn);
    for (int i = 0; i < 3; ++i) out[4 + i] = -(R[3 * i] * g[0] + R[3 * i + 1] * g[1] + R[3 * i + 2] * g[2]);
}

// phi of an analytic body of type TYPE at the body-frame point pb, with g = d phi / d p and gprm = d phi / d prm; false (nothing
// written) for a point outside the query cube
template <int TYPE> __host__ __device__ inline bool da_analytic(const PcSegment &S, const double *pb, double &phi, double *g, double *gprm)
{
    Shape<PcDual> s = S.shape;
    s.type = TYPE;      // (a constant: sdf_unit folds to this primitive's branch)
    PcDual p[3];
    for (int i = 0; i < 3; ++i) {
        p[i] = PcDual(pb[i]);
        p[i].d[i] = 1.0;
    }
    PcDual f, unused[3];
    if (!query_sdf(s, p, f, unused, false)) return false;
    phi = f.v;
    for (int i = 0; i < 3; ++i) { g[i] = f.d[i]; gprm[i] = f.d[3 + i]; }
    return true;
}

// phi = sc * the trilinear value of a grid of gn[3] samples at pb, the cell i0 and the place w in it (grid_cell, as
// pc_grid_point), and g = the gradient of that interpolant within the cell: d w_d / d p_d = (gn[d] - 1) / (2 sc), and the value is
// linear in each w_d, so d / d w_0 is the difference of the cell's two x faces, each interpolated in (w_1, w_2), and so on.
__host__ __device__ inline bool da_grid(const double *grid, const int *gn, double sc, const double *pb, int *i0, double *w, double &phi,
                                        double *g)
{
    if (!in_cube(pb, sc)) return false;
    double u[3];
    div3(pb, sc, u);
    grid_cell(gn, u, i0, w);
    const int n1 = gn[1], n2 = gn[2];
    double v[8], pv = 0.0;
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz) {
                v[4 * dx + 2 * dy + dz] = grid[((size_t)(i0[0] + dx) * n1 + i0[1] + dy) * n2 + i0[2] + dz];
                pv = pv + v[4 * dx + 2 * dy + dz] * grid_corner_weight(w, dx, dy, dz);
            }
    phi = pv * sc;
    const double u0 = 1.0 - w[0], u1 = 1.0 - w[1], u2 = 1.0 - w[2];
    const double gx = u1 * (u2 * (v[4] - v[0]) + w[2] * (v[5] - v[1])) + w[1] * (u2 * (v[6] - v[2]) + w[2] * (v[7] - v[3]));
    const double gy = u0 * (u2 * (v[2] - v[0]) + w[2] * (v[3] - v[1])) + w[0] * (u2 * (v[6] - v[4]) + w[2] * (v[7] - v[5]));
    const double gz = u0 * (u1 * (v[1] - v[0]) + w[1] * (v[3] - v[2])) + w[0] * (u1 * (v[5] - v[4]) + w[1] * (v[7] - v[6]));
    g[0] = gx * (0.5 * (gn[0] - 1));
    g[1] = gy * (0.5 * (gn[1] - 1));
    g[2] = gz * (0.5 * (gn[2] - 1));
    return true;
}

}  // namespace dss
