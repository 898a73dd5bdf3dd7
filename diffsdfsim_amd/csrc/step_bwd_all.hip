// step_bwd_all.hip -- the first stage of the reverse sweep (bwd_pre_kernel, step_bwd_pre.h) with every primitive SDF, neural and
// grid bodies and mesh-vertex adjoints: the full variant, behind launch_bwd_pre_all, which dss_step_backward (step_bwd.hip)
// calls when DssWorld.shape_rare is set.  Its contact adjoint runs in forward mode (contact_vjp below).
#define DSS_ALL_SHAPES 1
#include <type_traits>
#include "step_bwd_pre.h"
#include "launchers.h"

namespace {

template <class T> __device__ inline void attach_grid(const DssWorld &W, int sc, int b, Shape<T> &s)
{
    if (s.type != SHAPE_GRID || !W.grid_id) return;
    const int gi = W.grid_id[(size_t)sc * W.nb + b];
    s.grid = W.grid_data + W.grid_off[gi];
    for (int i = 0; i < 3; ++i) s.gn[i] = W.grid_dims[3 * gi + i];
}
// the latent code of a neural body: its row of the latent table (constants here; contact_vjp seeds them in the pass that
// differentiates them), or without a table shape parameters 0 and 1 with whatever seeds the caller gave those
inline __device__ const double *latent_row(const DssWorld &W, int sc, int b)
{
    return (W.igr_latent && W.shape_type[(size_t)sc * W.nb + b] == DSS_SHAPE_IGR) ? W.igr_latent + ((size_t)sc * W.nb + b) * DSS_IGR_LATENT_MAX : nullptr;
}
template <class T> __device__ inline void attach_latent(const DssWorld &W, const double *row, Shape<T> &s, const T *prm)
{
    static_assert(IGR_LAT_MAX == DSS_IGR_LATENT_MAX, "geom.h and the ABI agree on the widest latent code");
    if (s.type != SHAPE_IGR) return;
    T code[IGR_LAT_MAX];
    for (int j = 0; j < IGR_LAT_MAX; ++j) code[j] = row ? T(row[j]) : prm[j < 2 ? j : 0];
    set_latent(s, code, row ? (W.igr.latent ? W.igr.latent : 2) : 2);
}

// d(n, p1, p2)/d(pose1, pose2, prm1, prm2) contracted with gbar[9]; out[CONTACT_OUT + 2] = q1(4) x1(3) q2(4) x2(3) prm1(3) prm2(3) and
// two more: prm1 / prm2 of a neural body with a row in the latent table (DssWorld.igr_latent) are the first three derivatives
// w.r.t. its latent code and the two more the fourth (body 1 / body 2).
// Forward-mode duals, four seeds per pass.  Only q1 and prm1 enter the body-1 half of the contact (contact_head: two
// SDF queries and the Newton step): they take two full passes.  q2, x2 and prm2 enter the body-2 half alone
// (contact_tail: one query, two rotations), so their three passes differentiate that half with the head as constants;
// x1 appears only in rel = p1 + x1 - x2, hence d/dx1 = -d/dx2 and needs no pass of its own.
// lin1 / lin2: igr_lin records of a neural body 1 / body 2 for this contact (NULL: analytic body); stable_in >= 0: which
// body's normal the contact used, decided by the caller (for neural bodies the Laplacian probes are not repeated).
__device__ void contact_vjp(const DssWorld &W, int sc, const double *pose_n, int b1, int b2, int face,
                            const double *abc, const double *gbar, double *out, double *g_verts,
                            const double *lin1 = nullptr, const double *lin2 = nullptr, int stable_in = -1)
{
    constexpr int N = 4;
    typedef Dual<N> D;
    const size_t i1 = (size_t)sc * W.nb + b1, i2 = (size_t)sc * W.nb + b2;
    const bool det2 = (W.grad_flags & DSS_GRAD_DETACH_B2) != 0;
    const double *P1 = pose_n + 7 * b1, *P2 = pose_n + 7 * b2, *prm1 = W.shape_prm + i1 * 3, *prm2 = W.shape_prm + i2 * 3;
    const int ty1 = W.shape_type[i1], ty2 = W.shape_type[i2];
    const double aux1 = W.shape_aux[i1], aux2 = W.shape_aux[i2];
    // a neural body whose code lives in the latent table: the parameter pass of that body seeds the code's (up to four)
    // numbers in place of the three shape parameters, which such a body does not read
    const double *lt1 = latent_row(W, sc, b1), *lt2 = latent_row(W, sc, b2);
    // The two bodies of a pass, BodyG<T> with T = double (values) or Dual<4> (derivatives): poses and shape parameters as
    // constants, on which seed(B1, B2, pr1, pr2) places the pass's dual parts before the shapes are made from them.
    auto bodies = [&](auto &B1, auto &B2, auto seed) {
        typedef std::decay_t<decltype(B1.pos[0])> T;
        T pr1[3], pr2[3];
        for (int i = 0; i < 4; ++i) { B1.q[i] = T(P1[i]); B2.q[i] = T(P2[i]); }
        for (int i = 0; i < 3; ++i) { B1.pos[i] = T(P1[4 + i]); B2.pos[i] = T(P2[4 + i]); pr1[i] = T(prm1[i]); pr2[i] = T(prm2[i]); }
        seed(B1, B2, pr1, pr2);
        make_shape(B1.shape, ty1, pr1, aux1);
        make_shape(B2.shape, ty2, pr2, aux2);
        B1.shape.lin = lin1; B2.shape.lin = lin2; attach_grid(W, sc, b1, B1.shape); attach_grid(W, sc, b2, B2.shape);
        attach_latent(W, lt1, B1.shape, pr1); attach_latent(W, lt2, B2.shape, pr2);
    };
    auto no_seed = [](auto &, auto &, auto *, auto *) {};
    const Triangle t = load_triangle(W, i1, face);
    // value pass: the head as constants for the body-2 passes, and the normal-selection decision for all of them
    int stable = stable_in;
    double cp1v[3], n1v[3], d1v, p1v[3];
    {
        BodyG<double> B1, B2;
        bodies(B1, B2, no_seed);
        double nn[3], pp2[3], pen;
        contact_head(B1, t.v, abc, cp1v, n1v, d1v, p1v);
        contact_tail(B1, B2, cp1v, n1v, d1v, p1v, 1e-3, nn, pp2, pen, &stable);
    }
    for (int t = 0; t < CONTACT_OUT + 2; ++t) out[t] = 0.0;
    double lat1[N], lat2[N];        // derivatives w.r.t. a table-held latent code of body 1 / body 2
    auto contract = [&](const D *n, const D *p1, const D *p2, double *dst, int cnt) {
        for (int s = 0; s < cnt; ++s) {
            double acc = 0.0;
            for (int i = 0; i < 3; ++i) acc += gbar[i] * n[i].d[s] + (p1 ? gbar[3 + i] * p1[i].d[s] : 0.0) + gbar[6 + i] * p2[i].d[s];
            dst[s] = acc;
        }
    };
    // seeds of a table-held latent code: coordinate j on dual slot j
    auto seed_latent = [](Shape<D> &s) {
#pragma unroll
        for (int j = 0; j < IGR_LAT_MAX; ++j) if (j < s.nlat) s.lat[j].d[j] = 1.0;
    };
    // a full pass: the contact from the triangle on whose coordinates seed_tri(d, v, i) has placed their dual parts
    auto from_tri = [&](const BodyG<D> &B1, const BodyG<D> &B2, auto seed_tri, D *n, D *p1, D *p2) {
        D tri[3][3], pen;
        for (int v = 0; v < 3; ++v)
            for (int i = 0; i < 3; ++i) { D d(t.v[v][i]); seed_tri(d, v, i); tri[v][i] = d; }
        contact_from_bary(B1, B2, tri, abc, 1e-3, n, p1, p2, pen, &stable, det2);
    };
    // ---- body-1 inputs: full passes, seeds q1 | prm1 -------------------------------------------------------
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
        BodyG<D> B1, B2;
        bodies(B1, B2, [&](BodyG<D> &B1, BodyG<D> &, D *pr1, D *) {
            if (grp == 0) for (int i = 0; i < 4; ++i) B1.q[i].d[i] = 1.0;
            else if (!lt1) for (int i = 0; i < 3; ++i) pr1[i].d[i] = 1.0;
        });
        if (grp == 1 && lt1) seed_latent(B1.shape);
        D n[3], p1[3], p2[3];
        from_tri(B1, B2, [&](D &d, int v, int i) {
            if (grp != 1 || lt1) return;
            // box: own axis; sphere: radius; cylinder: x,y <- rad, z <- height
            const int s = (ty1 == SHAPE_BOX || ty1 == SHAPE_BOX_ROUNDED || ty1 == SHAPE_BRICK) ? i : ((ty1 == SHAPE_CYLINDER && i == 2) ? 1 : 0);
#pragma unroll
            for (int sl = 0; sl < 3; ++sl) if (sl == s) d.d[sl] = t.g[v][i];   // selects: a run-time index would put d in scratch
        }, n, p1, p2);
        if (grp == 0) contract(n, p1, p2, out + CS_Q1, 4);
        else if (lt1) contract(n, p1, p2, lat1, 4);
        else contract(n, p1, p2, out + CS_PRM1, 3);
    }
    // ---- body-2 inputs: the tail alone, seeds q2 | x2 | prm2 -----------------------------------------------
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
        BodyG<D> B1, B2;
        bodies(B1, B2, [&](BodyG<D> &, BodyG<D> &B2, D *, D *pr2) {
            if (grp == 0) for (int i = 0; i < 4; ++i) B2.q[i].d[i] = 1.0;
            else if (grp == 1) for (int i = 0; i < 3; ++i) B2.pos[i].d[i] = 1.0;
            else if (!lt2) for (int i = 0; i < 3; ++i) pr2[i].d[i] = 1.0;
        });
        if (grp == 2 && lt2) seed_latent(B2.shape);
        D cp1[3], n1[3], d1(d1v), p1[3], n[3], p2[3], pen;
        for (int i = 0; i < 3; ++i) { cp1[i] = D(cp1v[i]); n1[i] = D(n1v[i]); p1[i] = D(p1v[i]); }
        contact_tail(B1, B2, cp1, n1, d1, p1, 1e-3, n, p2, pen, &stable, det2);
        if (grp == 0) contract(n, nullptr, p2, out + CS_Q2, 4);
        else if (grp == 1) { contract(n, nullptr, p2, out + CS_X2, 3); for (int i = 0; i < 3; ++i) out[CS_X1 + i] = -out[CS_X2 + i]; }
        else if (lt2) contract(n, nullptr, p2, lat2, 4);
        else contract(n, nullptr, p2, out + CS_PRM2, 3);
    }
    // a table-held code: its first three derivatives take the parameter slots, the fourth goes to out[20] / out[21]
    if (lt1) { for (int i = 0; i < 3; ++i) out[CS_PRM1 + i] = lat1[i]; out[CONTACT_OUT] = lat1[3]; }
    if (lt2) { for (int i = 0; i < 3; ++i) out[CS_PRM2 + i] = lat2[i]; out[CONTACT_OUT + 1] = lat2[3]; }
    // ---- the triangle's vertices: one full pass per vertex, seeds = its three coordinates ------------------
    // Level-set meshes have no per-vertex parameter tangent (vgrad = 0); their shape gradient flows through the vertex
    // positions themselves and is chained to the parameters by the mesher's backward (MeshSDF, bodies.py:680-702).
    if (g_verts) {
        for (int vtx = 0; vtx < 3; ++vtx) {
            BodyG<D> B1, B2;
            bodies(B1, B2, no_seed);
            D n[3], p1[3], p2[3];
            from_tri(B1, B2, [&](D &d, int v, int i) {
#pragma unroll
                for (int sl = 0; sl < 3; ++sl) if (v == vtx && sl == i) d.d[sl] = 1.0;
            }, n, p1, p2);
            double gv[3];
            contract(n, p1, p2, gv, 3);
            for (int s = 0; s < 3; ++s) atomicAdd(g_verts + (size_t)t.id[vtx] * 3 + s, gv[s]);
        }
    }
}

// ---- neural SDF bodies in the reverse sweep ------------------------------------------------------------------------------
// The contact geometry of a neural body is differentiated through records of the network at the points it was queried at
// (geom.h: igr_lin).  bwd_igr_prep_kernel lists those points for the sub-step every scene is about to undo -- body 1 at the
// barycentric point of the contact's triangle, body 2 at the contact point in its frame -- igr_query_kernel evaluates the
// list twice on the matrix cores (d/dxyz, d/dlatent), igr_records turns the answers into the records of one contact.
__global__ void __launch_bounds__(64) bwd_igr_prep_kernel(DssWorld W_arg, DssAdjoint A_arg)
{
    DSS_KERNARG_REF(DssWorld, W, W_arg);
    DSS_KERNARG_REF_AT(DssAdjoint, A, A_arg, sizeof(DssWorld));
    const int sc = blockIdx.x, lane = threadIdx.x, nb = W.nb, MX = W.maxc;
    int k, act, init;
    SlotView v;
    bwd_select(W, A, sc, k, act, init, v);
    if (!act && !init) return;
    for (int c = lane; c < v.nc_n; c += 64) {
        const int b1 = v.body_n[c], b2 = v.body_n[MX + c];
        int idx[2] = {-1, -1};
        for (int side = 0; side < 2 && v.face_n[c] >= 0; ++side) {
            const int b = side ? b2 : b1;
            if (W.shape_type[(size_t)sc * nb + b] != DSS_SHAPE_IGR) continue;
            const double scale = W.shape_aux[(size_t)sc * nb + b];
            double pt[3];
            if (side == 0) {
                const int mesh = W.mesh_id[(size_t)sc * nb + b1];
                const int *fv = W.faces + (size_t)(W.mesh_foff[mesh] + DSS_FACE_ID(v.face_n[c])) * 3;
                pt[0] = pt[1] = pt[2] = 0.0;
                for (int q = 0; q < 3; ++q) {
                    const double *vp = W.verts + (size_t)(W.mesh_voff[mesh] + fv[q]) * 3, w = v.abc_n[(size_t)q * MX + c];
                    for (int i = 0; i < 3; ++i) pt[i] = pt[i] + vp[i] * w;        // (the order of contact_head)
                }
                // contact_head forms tri[0] abc[0] + tri[1] abc[1] + tri[2] abc[2]: the same sum, left to right
            } else {
                const double *P1 = v.pose_n + 7 * b1, *P2 = v.pose_n + 7 * b2;
                double rel[3];
                for (int i = 0; i < 3; ++i) rel[i] = (v.geom_n[(size_t)(3 + i) * MX + c] + P1[4 + i]) - P2[4 + i];
                quat_apply_inv(P2, rel, pt);
            }
            if (!in_cube(pt, scale)) { idx[side] = -2; continue; }       // query_sdfs: phi = scale, grad = 0 out there
            const int slot = atomicAdd(A.igr_bw_n, 1);
            double u[3];
            div3(pt, scale, u);
            for (int i = 0; i < 3; ++i) A.igr_bw_pts[(size_t)slot * 3 + i] = u[i];
            A.igr_bw_lat[slot] = sc * nb + b;
            idx[side] = slot;
        }
        A.igr_bw_idx[((size_t)sc * 2 + 0) * MX + c] = idx[0];
        A.igr_bw_idx[((size_t)sc * 2 + 1) * MX + c] = idx[1];
    }
}

// records of contact c: lin[0 .. 2 IGR_LIN) body 1 (queries at the triangle point and after the Newton step), lin[2 IGR_LIN ..)
// body 2; `stable` = which normal the forward pass picked (the flag in the contact's face word)
__device__ void igr_records(const DssWorld &W, const DssAdjoint &A, int sc, const SlotView &v, int c, int i1, int i2, double *lin,
                            int &stable)
{
    const int nb = W.nb, MX = W.maxc, b1 = v.body_n[c], b2 = v.body_n[MX + c];
    const size_t cap = (size_t)W.B * 2 * MX;
    const double *sdfX = A.igr_bw_sdf, *gX = A.igr_bw_grad, *gL = A.igr_bw_grad + cap * 3;
    // the latent pass writes rows of three (two derivatives and a zero), or of four for a four-number code (igr_mlp.hip)
    const int nl = W.igr.latent ? W.igr.latent : 2, ls = nl > 3 ? nl : 3;
    const double *P1 = v.pose_n + 7 * b1;
    for (int i = 0; i < 3 * IGR_LIN; ++i) lin[i] = 0.0;
    auto fill = [&](double *r, int idx, double scale) {
        if (idx < 0) { r[0] = scale; return; }      // outside the query cube: phi = scale, everything else zero
        r[0] = sdfX[idx] * scale;
        const double raw[3] = {gX[(size_t)idx * 3], gX[(size_t)idx * 3 + 1], gX[(size_t)idx * 3 + 2]};
        for (int i = 0; i < 3; ++i) r[1 + i] = raw[i];                  // d (scale f(pt / scale)) / d pt
        for (int j = 0; j < nl; ++j) r[4 + j] = gL[(size_t)idx * ls + j] * scale;
        normalize(raw, r + IGR_LIN_NRM);
    };
    if (i1 != -1) fill(lin, i1, W.shape_aux[(size_t)sc * nb + b1]);
    if (i2 != -1) fill(lin + 2 * IGR_LIN, i2, W.shape_aux[(size_t)sc * nb + b2]);
    // which body's normal the contact carries was decided in the forward pass and travels with the face id
    const double nt[3] = {v.geom_n[c], v.geom_n[(size_t)MX + c], v.geom_n[(size_t)2 * MX + c]};
    stable = (v.face_n[c] & DSS_FACE_NORMAL1) ? 0 : 1;
    if (i1 != -1 && !stable) {       // the normal used is body 1's after the Newton step: n = -R1 n1'  ->  n1' = -R1^T n
        double t[3];
        quat_apply_inv(P1, nt, t);
        for (int i = 0; i < 3; ++i) lin[IGR_LIN + IGR_LIN_NRM + i] = -t[i];
    }
}

struct FullSweep {
    static constexpr int NOUT = CONTACT_OUT + 2;
    static __device__ void contact_adjoint(const DssWorld &W, const DssAdjoint &A, int sc, const SlotView &v, int c, const double *abc,
                                           const double *gb, double *out)
    {
        const int MX = W.maxc;
        const double *l1 = nullptr, *l2 = nullptr;
        int st = -1;
        double lin[3 * IGR_LIN];
        if (A.igr_bw_idx) {
            const int i1 = A.igr_bw_idx[((size_t)sc * 2 + 0) * MX + c], i2 = A.igr_bw_idx[((size_t)sc * 2 + 1) * MX + c];
            if (i1 != -1 || i2 != -1) {
                igr_records(W, A, sc, v, c, i1, i2, lin, st);
                if (i1 != -1) l1 = lin;
                if (i2 != -1) l2 = lin + 2 * IGR_LIN;
            }
        }
        // the forward pass's normal choice travels with the face id: the Laplacian probes are not repeated
        if (st < 0) st = (v.face_n[c] & DSS_FACE_NORMAL1) ? 0 : 1;
        contact_vjp(W, sc, v.pose_n, v.body_n[c], v.body_n[MX + c], DSS_FACE_ID(v.face_n[c]), abc, gb, out, A.g_verts, l1, l2, st);
    }
    static __device__ double *latent_grad(const DssWorld &W, const DssAdjoint &A, int sc, int b)
    {
        return latent_row(W, sc, b) ? A.g_latent + ((size_t)sc * W.nb + b) * DSS_IGR_LATENT_MAX : nullptr;
    }
};

__global__ void __launch_bounds__(64) bwd_pre_kernel(DssWorld W_arg, DssAdjoint A_arg)
{
    DSS_KERNARG_REF(DssWorld, W, W_arg);
    DSS_KERNARG_REF_AT(DssAdjoint, A, A_arg, sizeof(DssWorld));
    bwd_pre<FullSweep>(W, A);
}

}  // namespace

namespace dss {
void launch_bwd_pre_all(const DssWorld &W, const DssAdjoint &A, hipStream_t stream)
{
    if (W.igr.W0 && A.igr_bw_idx) {
        const int cap = W.B * 2 * W.maxc;
        (void)hipMemsetAsync(A.igr_bw_n, 0, sizeof(int), stream);
        hipLaunchKernelGGL(bwd_igr_prep_kernel, dim3(W.B), dim3(64), 0, stream, W, A);
        const double *lat = W.igr_latent ? W.igr_latent : W.shape_prm;
        const int stride = W.igr_latent ? DSS_IGR_LATENT_MAX : 3;
        launch_igr_list(W.igr, A.igr_bw_pts, A.igr_bw_lat, lat, stride, A.igr_bw_n, cap, DSS_IGR_XYZ, A.igr_bw_sdf, A.igr_bw_grad, stream, W.B * 8);
        launch_igr_list(W.igr, A.igr_bw_pts, A.igr_bw_lat, lat, stride, A.igr_bw_n, cap, DSS_IGR_LATENT, A.igr_bw_sdf + cap,
                        A.igr_bw_grad + (size_t)cap * 3, stream, W.B * 8);
    }
    hipLaunchKernelGGL(bwd_pre_kernel, dim3(W.B), dim3(64), 0, stream, W, A);
}
}  // namespace dss
