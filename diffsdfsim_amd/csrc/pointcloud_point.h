// pointcloud_point.h -- one observed point of the point-cloud loss (experiments/trajectory_fitting/optim_pointcloud.py:166-201,
// `match_pointcloud`): the squared SDF of a world-frame point in the frame of a body estimate, and its derivative with respect
// to the estimate's pose and shape parameters.  Host and device: pointcloud_loss.hip sums these terms per segment,
// tests/emu/check_pointcloud_loss.cpp checks them against a long double restatement and central differences.
//
//   p    = R(q)^T (x - pos)            R = quat_to_mat(q): normalised by 2 / (q.q), so d / d q is taken w.r.t. the four raw
//                                      components and holds for a non-unit q too
//   in   = all(|p| <= scale)           decided on values; a point outside the query cube adds nothing to any output
//   phi  = query_sdf(shape, p)         values only (want_grad = false)
//   term = phi^2, 1, d phi^2 / d pose[7], d phi^2 / d prm[3]
//
// The derivative comes from geom.h on Dual<6>: slots 0-2 seed the body-frame point, slots 3-5 the three shape parameters
// (make_shape on duals carries them through `scale` and the unit-frame constants, as the reference's autograd does; the
// corner radius is a constant of the body).  The chain from p to pos and q is written out:
//   d p / d pos = -R^T                                    ->  d / d pos = -R g            (g = d phi^2 / d p)
//   R = 1 + s N(q), s = 2 / (q.q), N quadratic in q       ->  d / d q_k = s (d . dN/dq_k g) - s q_k (g . (p - d)),  d = x - pos
// (the second term is -s^2 q_k (d . N g) with N^T d = (p - d) / s).
#pragma once
#include "geom.h"

namespace dss {

constexpr int PC_OUT = 12;   // sum phi^2, count, d / d quat (4), d / d pos (3), d / d prm (3)
// The scalar of this loss: a Dual<6> under a name of its own, so that what is said about it below holds for this header's
// instantiations of geom.h alone (Shape<PcDual>, make_shape / query_sdf on PcDual) and for no other user of Dual<6>.
struct PcDual : Dual<6> {
    __host__ __device__ PcDual() {}
    __host__ __device__ PcDual(double x) : Dual<6>(x) {}
    __host__ __device__ PcDual(const Dual<6> &o) : Dual<6>(o) {}
};

// geom.h's t_max hands back one of its arguments whole.  For a dual that is a copy from an address chosen at run time, and in
// make_shape, which takes the largest of the three dims that way, it left the three seeded parameters in private memory (a
// select between the tangents is folded back into the same indexed load).  For PcDual the tangents are blended with a 0 / 1
// weight instead -- exact for finite numbers, ties to the first argument as there -- and everything stays in registers.
// These overloads take the place of the template wherever geom.h calls t_max on PcDual: once per segment in make_shape, and
// per point in sdf_unit (the inside distance of the box family, cylinder, brick and bowl).  The mixed forms serve calls such
// as t_max(prm[0], prm[1] / 2.0), whose second argument is the base type.
__host__ __device__ inline PcDual pc_max(const Dual<6> &a, const Dual<6> &b)
{
    const double wb = b.v > a.v ? 1.0 : 0.0, wa = 1.0 - wb;
    PcDual r;
    r.v = b.v > a.v ? b.v : a.v;
    for (int i = 0; i < 6; ++i) r.d[i] = wa * a.d[i] + wb * b.d[i];
    return r;
}
__host__ __device__ inline PcDual t_max(const PcDual &a, const PcDual &b) { return pc_max(a, b); }
__host__ __device__ inline PcDual t_max(const PcDual &a, const Dual<6> &b) { return pc_max(a, b); }
__host__ __device__ inline PcDual t_max(const Dual<6> &a, const PcDual &b) { return pc_max(a, b); }

struct PcSegment {
    double q[4], pos[3], R[9], two_s;
    Shape<PcDual> shape;
};

// prm4: three shape parameters and the corner radius
__host__ __device__ inline void pc_segment(PcSegment &S, const double *pose, int type, const double *prm4)
{
    for (int i = 0; i < 4; ++i) S.q[i] = pose[i];
    for (int i = 0; i < 3; ++i) S.pos[i] = pose[4 + i];
    quat_to_mat(S.q, S.R);
    S.two_s = 2.0 / (S.q[0] * S.q[0] + S.q[1] * S.q[1] + S.q[2] * S.q[2] + S.q[3] * S.q[3]);
    PcDual prm[3];
    for (int i = 0; i < 3; ++i) { prm[i] = PcDual(prm4[i]); prm[i].d[3 + i] = 1.0; }
    make_shape(S.shape, type, prm, prm4[3]);
}

// the world-frame point x in the segment's body frame: d = x - pos, p = R^T d
__host__ __device__ inline void pc_body_point(const PcSegment &S, const double *x, double *d, double *p)
{
    for (int i = 0; i < 3; ++i) d[i] = x[i] - S.pos[i];
    const double *R = S.R;
    for (int i = 0; i < 3; ++i) p[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
}

// terms of the world-frame point x; returns `in` (terms are written only for a point inside the query cube)
__host__ __device__ inline bool pc_point(const PcSegment &S, const double *x, double *term /*[PC_OUT]*/)
{
    double d[3], pb[3];
    pc_body_point(S, x, d, pb);
    const double *R = S.R;
    PcDual p[3];
    for (int i = 0; i < 3; ++i) {
        p[i] = PcDual(pb[i]);
        p[i].d[i] = 1.0;
    }
    PcDual phi, unused[3];
    if (!query_sdf(S.shape, p, phi, unused, false)) return false;
    term[0] = phi.v * phi.v;
    term[1] = 1.0;
    const double k = 2.0 * phi.v;
    const double g[3] = {k * phi.d[0], k * phi.d[1], k * phi.d[2]};
    // a[j][i] = d_j g_i contracted with d N / d q_k (N = (R - 1) / s, linear in q after one derivative)
    const double r = S.q[0], qi = S.q[1], qj = S.q[2], qk = S.q[3];
    const double a00 = d[0] * g[0], a01 = d[0] * g[1], a02 = d[0] * g[2];
    const double a10 = d[1] * g[0], a11 = d[1] * g[1], a12 = d[1] * g[2];
    const double a20 = d[2] * g[0], a21 = d[2] * g[1], a22 = d[2] * g[2];
    const double sr = qk * (a10 - a01) + qj * (a02 - a20) + qi * (a21 - a12);
    const double si = qj * (a01 + a10) + qk * (a02 + a20) + r * (a21 - a12) - 2.0 * qi * (a11 + a22);
    const double sj = qi * (a01 + a10) + qk * (a12 + a21) + r * (a02 - a20) - 2.0 * qj * (a00 + a22);
    const double sk = qi * (a02 + a20) + qj * (a12 + a21) + r * (a10 - a01) - 2.0 * qk * (a00 + a11);
    const double gn = g[0] * (p[0].v - d[0]) + g[1] * (p[1].v - d[1]) + g[2] * (p[2].v - d[2]);
    term[2] = S.two_s * (sr - r * gn);
    term[3] = S.two_s * (si - qi * gn);
    term[4] = S.two_s * (sj - qj * gn);
    term[5] = S.two_s * (sk - qk * gn);
    for (int i = 0; i < 3; ++i) term[6 + i] = -(R[3 * i] * g[0] + R[3 * i + 1] * g[1] + R[3 * i + 2] * g[2]);
    for (int i = 0; i < 3; ++i) term[9 + i] = k * phi.d[3 + i];
    return true;
}

// The same point of a voxel-grid segment (S.shape.grid and gn set) as the adjoint of the samples needs it
// (pointcloud_loss_grid_adj.hip): the membership test, the cell i0 and the place w in it, and phi = scale * the trilinear
// value -- the value pc_point squares, by query_sdf's cube test and division (geom.h's in_cube and div3), grid_cell and
// grid_corner_weight, which sdf_unit's SHAPE_GRID branch calls too.  The 8-term sum itself stands here a second time: in sdf_unit
// it shares its loop with the central-difference field, and taking it out of that loop changes the code of every kernel that
// queries grids (narrow phase, reverse sweep, camera).  tests/emu/check_pointcloud_grid_adj.cpp holds phi^2 here to the bits of
// pc_point's term[0] on every point it walks, so the two cannot drift apart unnoticed.
// phi is linear in the samples: d phi / d sample(corner) = scale * grid_corner_weight(w, corner).
__host__ __device__ inline bool pc_grid_point(const PcSegment &S, const double *x, int *i0, double *w, double &phi)
{
    double d[3], pb[3], u[3];
    pc_body_point(S, x, d, pb);
    const double sc = val(S.shape.scale);
    if (!in_cube(pb, sc)) return false;
    div3(pb, sc, u);
    grid_cell(S.shape.gn, u, i0, w);
    const int n1 = S.shape.gn[1], n2 = S.shape.gn[2];
    double pv = 0.0;
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz)
                pv = pv + S.shape.grid[((size_t)(i0[0] + dx) * n1 + i0[1] + dy) * n2 + i0[2] + dz] * grid_corner_weight(w, dx, dy, dz);
    phi = pv * sc;
    return true;
}

}  // namespace dss
