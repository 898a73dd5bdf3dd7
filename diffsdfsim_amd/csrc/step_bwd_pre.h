// step_bwd_pre.h -- what the variants of the reverse sweep's first stage share (step_bwd.hip, step_bwd_all.hip): the view of the
// tape slot a scene undoes, the rows of the per-contact scratch DssAdjoint.cscr, the ordered per-body sums and the body of
// bwd_pre_kernel, stated once over a variant policy V:
//   V::NOUT                      outputs of the contact adjoint: CONTACT_OUT, or two more (rows CS_LAT4_1 / CS_LAT4_2)
//   V::contact_adjoint(...)      d(n, p1, p2)/d(pose1, pose2, prm1, prm2) of one contact contracted with gb[9] -> out[NOUT]
//   V::latent_grad(W, A, sc, b)  with the two more: body b's row of DssAdjoint.g_latent if its parameter slots hold latent derivatives
// Everything sits in the including file's anonymous namespace and is included once that file has chosen its shape set.
#pragma once
#include <math.h>

#include "../../include/diffsdfsim_hip.h"
#include "contact_geom.h"
#include "wave_utils.h"

namespace {
using namespace dss;
static_assert(sizeof(DssWorld) % 8 == 0, "DSS_KERNARG_REF_AT: the adjoint descriptor follows the world descriptor without padding");

struct SlotView {   // where the data of "sub-step k" and of "the state after it" live
    const double *pose_k, *vel_k;               // [nb][7], [nb][6] start of sub-step k
    const double *pose_n;                       // [nb][7] pose after sub-step k
    double dt;
    int nc_k; const int *body_k; const double *geom_k;                   // contacts used by the LCP of k
    int nc_n; const int *body_n, *face_n; const double *abc_n, *geom_n;  // contacts detected after k
    const double *x, *lam, *slack, *nu;
};

__device__ inline void view_slot(const DssWorld &W, int sc, int k, SlotView &v)
{
    const int nb = W.nb, MX = W.maxc, NR = W.fric_dirs + 2;
    const size_t rec = (size_t)k * W.B + sc;
    v.pose_k = W.tp_pose + rec * nb * 7;
    v.vel_k = W.tp_vel + rec * nb * 6;
    v.dt = W.tp_dt[rec];
    v.nc_k = W.tp_nc[rec];
    v.body_k = W.tp_body + rec * 2 * MX;
    v.geom_k = W.tp_geom + rec * 10 * MX;
    v.x = W.tp_x + rec * 6 * nb;
    v.lam = W.tp_lam + rec * NR * MX;
    v.slack = W.tp_slack + rec * NR * MX;
    v.nu = W.tp_nu + rec * (W.neq > 0 ? W.neq : 1);
    if (k + 1 < W.nsub[sc]) {
        const size_t r2 = (size_t)(k + 1) * W.B + sc;
        v.pose_n = W.tp_pose + r2 * nb * 7;
        v.nc_n = W.tp_nc[r2]; v.body_n = W.tp_body + r2 * 2 * MX; v.face_n = W.tp_face + r2 * MX; v.abc_n = W.tp_abc + r2 * 3 * MX;
        v.geom_n = W.tp_geom + r2 * 10 * MX;
    } else {
        v.pose_n = W.pose + (size_t)sc * nb * 7;
        v.nc_n = W.nc[sc]; v.body_n = W.c_body + (size_t)sc * 2 * MX; v.face_n = W.c_face + (size_t)sc * MX;
        v.abc_n = W.c_abc + (size_t)sc * 3 * MX;
        v.geom_n = W.c_geom + (size_t)sc * 10 * MX;
    }
}

// which sub-step a scene undoes in this call, and the view of it (shared by the kernels of one dss_step_backward)
__device__ inline void bwd_select(const DssWorld &W, const DssAdjoint &A, int sc, int &k, int &act, int &init, SlotView &v)
{
    const int nb = W.nb, MX = W.maxc;
    k = A.cur_slot[sc];
    act = (k >= 0 && k >= A.lo_slot[sc] && k < W.nsub[sc] && k < W.max_sub);   // (a slot beyond the tape was never recorded)
    // slot -1 = the contacts found at construction (World.__init__, world.py:96): only their geometry
    // adjoint is left to push onto the initial pose and the shape parameters
    init = (k == -1 && A.lo_slot[sc] <= -1 && W.nsub[sc] > 0);
    if (init) {
        const size_t r0 = (size_t)sc;   // tape slot 0
        v.pose_n = W.tp_pose + r0 * nb * 7;
        v.nc_n = W.tp_nc[r0]; v.body_n = W.tp_body + r0 * 2 * MX; v.face_n = W.tp_face + r0 * MX; v.abc_n = W.tp_abc + r0 * 3 * MX;
        v.geom_n = W.tp_geom + r0 * 10 * MX;
    } else if (act) {
        view_slot(W, sc, k, v);
    }
}

// Rows of DssAdjoint.cscr [B][DSS_CSCR_ROWS][maxc] as bwd_pre_kernel uses them, one column per contact detected after the
// sub-step.  (bwd_post_kernel, which runs after these have been summed, keeps its own pieces in rows 0-13.)
constexpr int CONTACT_OUT = 20;
enum CscrRow {
    // the contact adjoint's outputs, in its order: out[i] lives in row i for i < CONTACT_OUT
    CS_Q1 = 0, CS_X1 = 4, CS_Q2 = 7, CS_X2 = 11, CS_PRM1 = 14, CS_PRM2 = 17,
    // a time-of-contact event (H.backward): the moved poses, the new velocities and f/m of both bodies, the step h
    CS_TOC_POSE1 = CONTACT_OUT, CS_TOC_POSE2 = 27, CS_TOC_VEL1 = 34, CS_TOC_VEL2 = 40, CS_TOC_ACC1 = 46, CS_TOC_ACC2 = 49, CS_TOC_H = 52,
    CS_MOVE_DT = 53,                    // d/d(dt) of a body's move: one column per BODY
    CS_LAT4_1 = 54, CS_LAT4_2 = 55,     // fourth derivative w.r.t. a table-held latent code of body 1 / body 2: out[20], out[21]
};
static_assert(CS_LAT4_2 + 1 == DSS_CSCR_ROWS, "the rows named here are the rows the ABI allocates");
__device__ constexpr int contact_out_row(int i) { return i < CONTACT_OUT ? i : CS_LAT4_1 + (i - CONTACT_OUT); }

// face `face` of the mesh of body `body` (= scene * nb + b): vertex positions, their tangents w.r.t. the shape parameters, rows in W.verts
struct Triangle { double v[3][3], g[3][3]; int id[3]; };
__device__ inline Triangle load_triangle(const DssWorld &W, size_t body, int face)
{
    Triangle t;
    const int mesh = W.mesh_id[body];
    const int voff = W.mesh_voff[mesh];
    const int *fv = W.faces + (size_t)(W.mesh_foff[mesh] + face) * 3;
    for (int v = 0; v < 3; ++v) {
        t.id[v] = voff + fv[v];
        for (int i = 0; i < 3; ++i) { t.v[v][i] = W.verts[(size_t)t.id[v] * 3 + i]; t.g[v][i] = W.vgrad[(size_t)t.id[v] * 3 + i]; }
    }
    return t;
}

// Ordered per-body sums of per-contact pieces:
//   sums[b * NC + q] = sum over contacts c, in contact order, of [body1(c) = b] cs[row0[q]][c] + [body2(c) = b] cs[row1[q]][c].
// One lane per (body, component) instead of one lane per body walking every component: the loads of a contact do not
// depend on the running sums, so the unrolled loop keeps four contacts in flight; a term that does not belong to the
// lane's body is added as 0.0, which leaves the sum -- and therefore its summation order -- exactly as before.
template <int NC>
__device__ inline void contact_sums(const int *body, int MX, int nc, int nb, const double *cs, const int *row0,
                                    const int *row1, double *sums)
{
    const int lane = threadIdx.x;
    for (int e = lane; e < nb * NC; e += 64) {
        const int b = e / NC, q = e % NC;
        const double *c0 = cs + (size_t)row0[q] * MX, *c1 = cs + (size_t)row1[q] * MX;
        double acc = 0.0;
        int c = 0;
        for (; c + 4 <= nc; c += 4) {
            int b1[4], b2[4];
            double v0[4], v1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { b1[u] = body[c + u]; b2[u] = body[MX + c + u]; v0[u] = c0[c + u]; v1[u] = c1[c + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { acc += (b1[u] == b) ? v0[u] : 0.0; acc += (b2[u] == b) ? v1[u] : 0.0; }
        }
        for (; c < nc; ++c) { acc += (body[c] == b) ? c0[c] : 0.0; acc += (body[MX + c] == b) ? c1[c] : 0.0; }
        sums[e] = acc;
    }
    __syncthreads();
}

// the body of bwd_pre_kernel (one wavefront per scene) for variant V
template <class V>
__device__ __forceinline__ void bwd_pre(const DssWorld &W, const DssAdjoint &A)
{
    const int sc = blockIdx.x, lane = threadIdx.x, nb = W.nb, MX = W.maxc;
    int k, act, init;
    SlotView v;
    bwd_select(W, A, sc, k, act, init, v);
    if (lane == 0) A.bw_active[sc] = act;
    if (!act && !init) return;
    double *a_pose = A.a_pose + (size_t)sc * nb * 7, *a_vel = A.a_vel + (size_t)sc * nb * 6;
    double *a_geom = A.a_geom + (size_t)sc * 10 * MX, *cs = A.cscr + (size_t)sc * DSS_CSCR_ROWS * MX;

    // (0) time-of-contact event (world.py:272-341): dt_h = H(dt_, theta).  Its adjoint is that of the redone
    //     move plus the carry from the next sub-step (whose dt_ = -last_dt + ...); H.backward (world.py:195-237)
    //     turns it into adjoints of the new contacts' geometry, the new velocities, the moved poses and f/m.
    const int flags = init ? 0 : W.tp_flags[(size_t)k * W.B + sc];
    const int ev = flags & 1;
    double dt_int = 0.0;   // d(loss)/d(dt) through the pose integration, seed = pose adjoint before the TOC terms
    // Jacobian of this body's move (Body3D.move, bodies.py:488-496: q' = quat(exp(w dt)) (x) q, x' = x + v dt) from ONE
    // dual-number pass over theta = w dt: d q'/d theta (4 x 3).  Everything else follows in closed form -- d/dw = dt d/dtheta,
    // d/d dt = sum_i w_i d/dtheta_i, q' is linear in q (adjoint = conj(dq) (x) .), x' is affine -- where four full passes
    // (one seed, seven, six and one) used to set this kernel's register footprint.
    double Jt[4][3], dqv[4] = {1.0, 0.0, 0.0, 0.0}, qsg = 1.0, vnw[6] = {0, 0, 0, 0, 0, 0};
    for (int o = 0; o < 4; ++o) for (int s3 = 0; s3 < 3; ++s3) Jt[o][s3] = 0.0;
    if (!init && lane < nb) {
        typedef Dual<3> D;
        for (int i = 0; i < 6; ++i) vnw[i] = -v.x[6 * lane + i];
        D w[3], R[9], dq[4], qk[4], o4[4];
        for (int i = 0; i < 3; ++i) { w[i] = D(vnw[i] * v.dt); w[i].d[i] = 1.0; }
        so3_exp(w, R);
        mat_to_quat(R, dq);
        for (int i = 0; i < 4; ++i) qk[i] = D(v.pose_k[7 * lane + i]);
        quat_raw_mul(dq, qk, o4);
        qsg = o4[0].v < 0.0 ? -1.0 : 1.0;      // quaternion_multiply standardises to a non-negative real part
        for (int o = 0; o < 4; ++o) { dqv[o] = dq[o].v; for (int s3 = 0; s3 < 3; ++s3) Jt[o][s3] = qsg * o4[o].d[s3]; }
    }
    // adjoint of the move for a pose adjoint ap[7]: -> pose_k (apk), v_new (avn), dt (returned)
    auto move_adjoint = [&](const double *ap, double *apk, double *avn) -> double {
        double th[3], adt = 0.0;
        for (int s3 = 0; s3 < 3; ++s3) th[s3] = ap[0] * Jt[0][s3] + ap[1] * Jt[1][s3] + ap[2] * Jt[2][s3] + ap[3] * Jt[3][s3];
        for (int i = 0; i < 3; ++i) { adt += th[i] * vnw[i] + ap[4 + i] * vnw[3 + i]; if (avn) { avn[i] = th[i] * v.dt; avn[3 + i] = ap[4 + i] * v.dt; } }
        if (apk) {
            const double dc[4] = {dqv[0], -dqv[1], -dqv[2], -dqv[3]}, aq[4] = {qsg * ap[0], qsg * ap[1], qsg * ap[2], qsg * ap[3]};
            quat_raw_mul(dc, aq, apk);          // <a, dq (x) q> = <conj(dq) (x) a, q>
            for (int i = 0; i < 3; ++i) apk[4 + i] = ap[4 + i];
        }
        return adt;
    };
    if (!init) {
        double part = 0.0;
        if (lane < nb) part = move_adjoint(a_pose + 7 * lane, nullptr, nullptr);
        dt_int = wave_sum(part);
    }
    double hc_bar = 0.0;
    if (ev) {
        const double dtbar_h = dt_int + A.a_last_dt[sc];
        const double h = v.dt;
        double dDdh[3] = {0, 0, 0};
        int q = 0;
        double den = 0.0;
        auto fill = [&](int c, double *in) {
            const int b1 = v.body_n[c], b2 = v.body_n[MX + c];
            in[0] = h; in[1] = h;
            for (int i = 0; i < 3; ++i) { in[2 + i] = v.geom_n[(size_t)(3 + i) * MX + c]; in[5 + i] = v.geom_n[(size_t)(6 + i) * MX + c]; in[8 + i] = v.geom_n[(size_t)i * MX + c]; }
            for (int i = 0; i < 6; ++i) { in[11 + i] = -v.x[6 * b1 + i]; in[17 + i] = -v.x[6 * b2 + i]; }
            for (int i = 0; i < 7; ++i) { in[23 + i] = v.pose_n[7 * b1 + i]; in[30 + i] = v.pose_n[7 * b2 + i]; }
            for (int i = 0; i < 3; ++i) {
                in[37 + i] = W.fext[((size_t)sc * nb + b1) * 6 + 3 + i] / W.mass[(size_t)sc * nb + b1];
                in[40 + i] = W.fext[((size_t)sc * nb + b2) * 6 + 3 + i] / W.mass[(size_t)sc * nb + b2];
            }
        };
        auto is_toc = [&](int c) {
            const int a = v.body_n[c], b = v.body_n[MX + c];
            for (int j = 0; j < v.nc_k; ++j) {
                const int a0 = v.body_k[j], b0 = v.body_k[MX + j];
                if ((a0 == a && b0 == b) || (a0 == b && b0 == a)) return false;
            }
            return true;
        };
        auto dD_dh = [&](int c) -> double {
            if (!is_toc(c)) return 0.0;
            double in[43];
            fill(c, in);
            typedef Dual<1> D;
            D di[43];
            for (int i = 0; i < 43; ++i) di[i] = D(in[i]);
            di[0].d[0] = 1.0;
            const double g = toc_D(di).d[0];
            return g < 1e-6 / h ? 0.0 : g;      // only motion into collision (world.py:203; Defaults.TOL = 1e-6)
        };
        for (int c = lane; c < v.nc_n; c += 64, ++q) {
            const double g = dD_dh(c);
            if (q < 3) dDdh[q] = g;             // the first three contacts of a lane are cached, later ones recomputed below
            den += g * g;
        }
        den = wave_sum(den);
        q = 0;
        for (int c = lane; c < v.nc_n; c += 64) for (int r = CS_TOC_POSE1; r <= CS_TOC_H; ++r) cs[(size_t)r * MX + c] = 0.0;
        __syncthreads();
        // The gradient of D with respect to its 43 inputs, one dual-number pass per input.  A time-of-contact event is rare (a
        // handful per rollout and scene) but its sweep iteration is the slowest scene's: with the 43 passes walked by the lane
        // that owns the contact, a batch of free-running scenes -- where some scene meets an event in almost every iteration --
        // spent 270 us per iteration here.  The passes of ONE contact go to 43 lanes instead (lane = seed); the contacts of an
        // event (one to four) are taken one after the other.
        for (int base = 0; base < v.nc_n; base += 64, ++q) {
            const int c_own = base + lane;
            double gq = 0.0;
            if (c_own < v.nc_n && den > 1e-5) gq = q < 3 ? dDdh[q] : dD_dh(c_own);
            unsigned long long todo = __ballot(gq != 0.0);
            while (todo) {
                const int bit = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int c = base + bit;
                const double wgt = -(__shfl(gq, bit, 64) / den) * dtbar_h;
                double in[43];
                fill(c, in);
                double og = 0.0;
                if (lane < 43) {
                    typedef Dual<1> D;
                    D di[43];
                    for (int i = 0; i < 43; ++i) { di[i] = D(in[i]); di[i].d[0] = (i == lane) ? 1.0 : 0.0; }
                    og = wgt * toc_D(di).d[0];
                }
                // lane sd holds d/d in[sd]: geometry of the new contact (p1: 2-4, p2: 5-7, normal: 8-10), the two new velocities
                // (11-16, 17-22), the two moved poses (23-29, 30-36), f/m of both bodies (37-39, 40-42), h (1)
                const int sd = lane;
                if (sd >= 2 && sd <= 4) a_geom[(size_t)(3 + sd - 2) * MX + c] += og;
                else if (sd >= 5 && sd <= 7) a_geom[(size_t)(6 + sd - 5) * MX + c] += og;
                else if (sd >= 8 && sd <= 10) a_geom[(size_t)(sd - 8) * MX + c] += og;
                else if (sd >= 23 && sd <= 29) cs[(size_t)(CS_TOC_POSE1 + sd - 23) * MX + c] = og;
                else if (sd >= 30 && sd <= 36) cs[(size_t)(CS_TOC_POSE2 + sd - 30) * MX + c] = og;
                else if (sd >= 11 && sd <= 16) cs[(size_t)(CS_TOC_VEL1 + sd - 11) * MX + c] = og;
                else if (sd >= 17 && sd <= 22) cs[(size_t)(CS_TOC_VEL2 + sd - 17) * MX + c] = og;
                else if (sd >= 37 && sd <= 39) cs[(size_t)(CS_TOC_ACC1 + sd - 37) * MX + c] = og;
                else if (sd >= 40 && sd <= 42) cs[(size_t)(CS_TOC_ACC2 + sd - 40) * MX + c] = og;
                else if (sd == 1) cs[(size_t)CS_TOC_H * MX + c] = og;
            }
        }
        __syncthreads();
        double hp = 0.0;
        for (int c = lane; c < v.nc_n; c += 64) hp += cs[(size_t)CS_TOC_H * MX + c];
        hc_bar = wave_sum(hp);
    }

    // (a) contacts detected after the sub-step: geometry adjoint -> pose after the sub-step, shape params
    for (int c = lane; c < v.nc_n; c += 64) {
        double gb[9], out[V::NOUT];
        for (int i = 0; i < 9; ++i) gb[i] = a_geom[(size_t)i * MX + c];
        const double abc[3] = {v.abc_n[c], v.abc_n[MX + c], v.abc_n[2 * MX + c]};
        if (v.face_n[c] >= 0) V::contact_adjoint(W, A, sc, v, c, abc, gb, out);
        else for (int i = 0; i < V::NOUT; ++i) out[i] = 0.0;     // kept from a penetrating direction (world.py:345-347): computed under no_grad
        for (int i = 0; i < V::NOUT; ++i) cs[(size_t)contact_out_row(i) * MX + c] = out[i];
    }
    __syncthreads();
    // per body: pose (7), shape parameters (3) and, for NS = 11, the fourth number of a table-held latent code
    constexpr int NS = 10 + (V::NOUT - CONTACT_OUT) / 2;
    static constexpr int row0[11] = {CS_Q1, CS_Q1 + 1, CS_Q1 + 2, CS_Q1 + 3, CS_X1, CS_X1 + 1, CS_X1 + 2, CS_PRM1, CS_PRM1 + 1, CS_PRM1 + 2, CS_LAT4_1};
    static constexpr int row1[11] = {CS_Q2, CS_Q2 + 1, CS_Q2 + 2, CS_Q2 + 3, CS_X2, CS_X2 + 1, CS_X2 + 2, CS_PRM2, CS_PRM2 + 1, CS_PRM2 + 2, CS_LAT4_2};
    __shared__ double s_sums[64 * NS];
    contact_sums<NS>(v.body_n, MX, v.nc_n, nb, cs, row0, row1, s_sums);
    if (lane < nb) {
        double ap[7], gp[3];
        for (int i = 0; i < 7; ++i) ap[i] = a_pose[7 * lane + i] + s_sums[NS * lane + i];
        for (int i = 0; i < 3; ++i) gp[i] = s_sums[NS * lane + 7 + i];
        double *gl = nullptr;
        if constexpr (NS > 10) gl = V::latent_grad(W, A, sc, lane);
        if (gl) {       // (the parameter slots of such a body hold latent derivatives: g_prm stays as it is)
            for (int i = 0; i < 3; ++i) gl[i] += gp[i];
            gl[3] += s_sums[NS * lane + 10];
        } else
            for (int i = 0; i < 3; ++i) A.g_prm[((size_t)sc * nb + lane) * 3 + i] += gp[i];
        if (ev) {   // pieces of H.backward that land on this body: moved pose, new velocity, f/m
            double vx[6] = {0, 0, 0, 0, 0, 0}, ab[3] = {0, 0, 0};
            for (int c = 0; c < v.nc_n; ++c) {
                if (v.body_n[c] == lane) {
                    for (int i = 0; i < 7; ++i) ap[i] += cs[(size_t)(CS_TOC_POSE1 + i) * MX + c];
                    for (int i = 0; i < 6; ++i) vx[i] += cs[(size_t)(CS_TOC_VEL1 + i) * MX + c];
                    for (int i = 0; i < 3; ++i) ab[i] += cs[(size_t)(CS_TOC_ACC1 + i) * MX + c];
                }
                if (v.body_n[MX + c] == lane) {
                    for (int i = 0; i < 7; ++i) ap[i] += cs[(size_t)(CS_TOC_POSE2 + i) * MX + c];
                    for (int i = 0; i < 6; ++i) vx[i] += cs[(size_t)(CS_TOC_VEL2 + i) * MX + c];
                    for (int i = 0; i < 3; ++i) ab[i] += cs[(size_t)(CS_TOC_ACC2 + i) * MX + c];
                }
            }
            const size_t bi = (size_t)sc * nb + lane;
            const double m = W.mass[bi];
            for (int i = 0; i < 3; ++i) {   // a = f/m
                A.g_fext[bi * 6 + 3 + i] += ab[i] / m;
                A.g_mass[bi] -= ab[i] * W.fext[bi * 6 + 3 + i] / (m * m);
            }
            for (int i = 0; i < 6; ++i) a_vel[6 * lane + i] += vx[i];   // joins the adjoint of the new velocity
        }
        for (int i = 0; i < 7; ++i) a_pose[7 * lane + i] = ap[i];
    }
    if (init) {
        __syncthreads();
        for (int c = lane; c < MX; c += 64) for (int i = 0; i < 10; ++i) a_geom[(size_t)i * MX + c] = 0.0;
        if (lane == 0) A.cur_slot[sc] = -2;
        return;
    }
    if (lane < nb) {
        double ap[7];
        for (int i = 0; i < 7; ++i) ap[i] = a_pose[7 * lane + i] ;
        // (b) pose_n = integrate(pose_k, v_new, dt): adjoint -> pose_k, v_new, dt (with the complete pose adjoint: first move
        //     and redone move share it)
        double apk[7], avn[6];
        cs[(size_t)CS_MOVE_DT * MX + lane] = move_adjoint(ap, apk, avn);
        for (int i = 0; i < 7; ++i) a_pose[7 * lane + i] = apk[i];
        // total adjoint of v_new = (later uses, already in a_vel) + (integration); x = -v_new
        for (int i = 0; i < 6; ++i) A.a_x[(size_t)sc * 6 * nb + 6 * lane + i] = -(a_vel[6 * lane + i] + avn[i]);
        // (c) LCP operands of sub-step k: mass blocks
        const size_t bi = (size_t)sc * nb + lane;
        double Iw[9];
        world_inertia(v.pose_k + 7 * lane, W.inertia + bi * 9, Iw);
        double *M = W.Mblk + bi * 36;
        const double m = W.mass[bi];
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) M[6 * r + c] = (r < 3 && c < 3) ? Iw[3 * r + c] : ((r == c) ? m : 0.0);
        for (int i = 0; i < 6; ++i) W.x[(size_t)sc * 6 * nb + 6 * lane + i] = v.x[6 * lane + i];
    }
    __syncthreads();
    {
        double part = (lane < nb) ? cs[(size_t)CS_MOVE_DT * MX + lane] : 0.0;
        part = wave_sum(part);
        if (lane == 0) A.a_dt[sc] = part + hc_bar + (ev ? A.a_last_dt[sc] : 0.0);
    }
    if (lane < W.neq) W.nu[(size_t)sc * W.neq + lane] = v.nu[lane];
    const int ND = W.fric_dirs / 2, NF = 3 * (1 + ND) + 8, NR = W.fric_dirs + 2;
    double *cop = W.cop + (size_t)sc * NF * MX;
    for (int c = lane; c < v.nc_k; c += 64) {
        const int b1 = v.body_k[c], b2 = v.body_k[MX + c];
        W.cop_body[(size_t)sc * 2 * MX + c] = b1;
        W.cop_body[(size_t)sc * 2 * MX + MX + c] = b2;
        double n[3], p1[3], p2[3], D[4][3];
        for (int i = 0; i < 3; ++i) { n[i] = v.geom_k[(size_t)i * MX + c]; p1[i] = v.geom_k[(size_t)(3 + i) * MX + c]; p2[i] = v.geom_k[(size_t)(6 + i) * MX + c]; }
        friction_dirs(n, ND, D);
        for (int i = 0; i < 3; ++i) {
            cop[(size_t)i * MX + c] = n[i];
            for (int q = 0; q < ND; ++q) cop[(size_t)(3 * (q + 1) + i) * MX + c] = D[q][i];
        }
        const int o = 3 * (1 + ND);
        for (int i = 0; i < 3; ++i) { cop[(size_t)(o + i) * MX + c] = p1[i]; cop[(size_t)(o + 3 + i) * MX + c] = p2[i]; }
        cop[(size_t)(o + 6) * MX + c] = 0.5 * (W.fric[(size_t)sc * nb + b1] + W.fric[(size_t)sc * nb + b2]);
        cop[(size_t)(o + 7) * MX + c] = 0.0;  // h does not enter the backward system (lcp.py:176-183)
    }
    if (lane == 0) A.bw_nc[sc] = v.nc_k;
}

}  // namespace
