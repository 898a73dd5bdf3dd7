// step_bwd.hip -- reverse sweep over the stepper's tape (gfx950).
//
// One call of dss_step_backward undoes one accepted sub-step per scene (the newest unprocessed one):
//
//   bwd_pre_kernel    (a) adjoint of the contact geometry that was computed at the END of the
//                         sub-step (contacts.py:161-214 on the filtered set) -> pose, shape params
//                     (b) adjoint of Body3D.move (bodies.py:488-511)       -> start pose, new velocity
//                     (c) re-assembles the sub-step's LCP operands from the tape (engines.py:36-81)
//   lcp_contact_backward   implicit differentiation of the LCP (lcp.py:156-213)
//   bwd_post_kernel   adjoint of the assembly: u = M v + dt f, M = blockdiag(R I R^T, m),
//                     friction directions, mu / restitution averages, h = (Jc v) e
//                     (engines.py:36-81, physics3d/world.py:48-101, world.py:400-501)
//
// Small nonlinear stages are differentiated with forward-mode duals (geom.h) seeded a few inputs at a
// time and contracted with the incoming adjoint; linear stages are transposed by hand.  Sums over the
// contacts of a body run in contact order (no atomics): gradients are bit-reproducible.
//
// bwd_pre_kernel has two variants over one body (step_bwd_pre.h): the lean one here (box / sphere / cylinder, what the benchmark
// configs run) and the full one of step_bwd_all.hip, which dss_step_backward launches instead when DssWorld.shape_rare is set.
#define DSS_ALL_SHAPES 0
#include "step_bwd_pre.h"
#include "contact_rev.h"
#include "launchers.h"

namespace {

struct LeanSweep {       // the contact adjoint in reverse mode (contact_rev.h): one value pass, one adjoint pass
    static constexpr int NOUT = CONTACT_OUT;
    static __device__ void contact_adjoint(const DssWorld &W, const DssAdjoint &, int sc, const SlotView &v, int c, const double *abc,
                                           const double *gb, double *out)
    {
        const int nb = W.nb, MX = W.maxc, b1 = v.body_n[c], b2 = v.body_n[MX + c];
        const size_t i1 = (size_t)sc * nb + b1, i2 = (size_t)sc * nb + b2;
        const Triangle t = load_triangle(W, i1, DSS_FACE_ID(v.face_n[c]));
        const int st = (v.face_n[c] & DSS_FACE_NORMAL1) ? 0 : 1;   // the forward pass's normal choice travels with the face id
        contact_vjp_rev(v.pose_n + 7 * b1, v.pose_n + 7 * b2, W.shape_type[i1], W.shape_type[i2], W.shape_prm + i1 * 3, W.shape_prm + i2 * 3,
                        t.v, t.g, abc, gb, st, (W.grad_flags & DSS_GRAD_DETACH_B2) != 0, out);
    }
};

__global__ void __launch_bounds__(64) bwd_pre_kernel(DssWorld W_arg, DssAdjoint A_arg)
{
    DSS_KERNARG_REF(DssWorld, W, W_arg);
    DSS_KERNARG_REF_AT(DssAdjoint, A, A_arg, sizeof(DssWorld));
    bwd_pre<LeanSweep>(W, A);
}

__global__ void __launch_bounds__(64) bwd_post_kernel(DssWorld W_arg, DssAdjoint A_arg)
{
    static_assert(sizeof(DssWorld) % 8 == 0, "the adjoint descriptor follows the world descriptor without padding");
    DSS_KERNARG_REF(DssWorld, W, W_arg);
    DSS_KERNARG_REF_AT(DssAdjoint, A, A_arg, sizeof(DssWorld));
    const int sc = blockIdx.x, lane = threadIdx.x, nb = W.nb, MX = W.maxc;
    if (!A.bw_active[sc]) return;
    const int k = A.cur_slot[sc];
    SlotView v;
    view_slot(W, sc, k, v);
    const int ND = W.fric_dirs / 2, NF = 3 * (1 + ND) + 8, o = 3 * (1 + ND);
    double *a_pose = A.a_pose + (size_t)sc * nb * 7, *a_vel = A.a_vel + (size_t)sc * nb * 6;
    double *a_geom = A.a_geom + (size_t)sc * 10 * MX, *cs = A.cscr + (size_t)sc * DSS_CSCR_ROWS * MX;
    const double *dcop = A.dcop + (size_t)sc * NF * MX, *dM = A.dMblk + (size_t)sc * nb * 36, *du = A.dpvec + (size_t)sc * 6 * nb;

    // contacts of sub-step k: adjoint of (dirs, p1, p2, mu, h_n) -> geometry, friction, restitution, velocities
    for (int c = lane; c < MX; c += 64) {
        if (c >= v.nc_k) { for (int i = 0; i < 10; ++i) a_geom[(size_t)i * MX + c] = 0.0; continue; }
        const int b1 = v.body_k[c], b2 = v.body_k[MX + c];
        const size_t i1 = (size_t)sc * nb + b1, i2 = (size_t)sc * nb + b2;
        double n[3], p1[3], p2[3], nbar[3], p1bar[3], p2bar[3];
        for (int i = 0; i < 3; ++i) {
            n[i] = v.geom_k[(size_t)i * MX + c]; p1[i] = v.geom_k[(size_t)(3 + i) * MX + c]; p2[i] = v.geom_k[(size_t)(6 + i) * MX + c];
            nbar[i] = dcop[(size_t)i * MX + c]; p1bar[i] = dcop[(size_t)(o + i) * MX + c]; p2bar[i] = dcop[(size_t)(o + 3 + i) * MX + c];
        }
        {   // friction directions D_q(n)
            typedef Dual<3> D;
            D nd[3], Dq[4][3];
            for (int i = 0; i < 3; ++i) { nd[i] = D(n[i]); nd[i].d[i] = 1.0; }
            friction_dirs(nd, ND, Dq);
            for (int s = 0; s < 3; ++s) {
                double acc = 0.0;
                for (int q = 0; q < ND; ++q) for (int i = 0; i < 3; ++i) acc += dcop[(size_t)(3 * (q + 1) + i) * MX + c] * Dq[q][i].d[s];
                nbar[s] += acc;
            }
        }
        const double mubar = dcop[(size_t)(o + 6) * MX + c], hbar = dcop[(size_t)(o + 7) * MX + c];
        const double *v1 = v.vel_k + 6 * b1, *v2 = v.vel_k + 6 * b2;
        double c1[3], c2[3], jv = 0.0;
        cross(p1, n, c1);
        cross(p2, n, c2);
        for (int i = 0; i < 3; ++i) jv += c1[i] * v1[i] + n[i] * v1[3 + i] - c2[i] * v2[i] - n[i] * v2[3 + i];
        const double rc = 0.5 * (W.restitution[i1] + W.restitution[i2]);
        const double jvbar = hbar * rc, rcbar = hbar * jv;
        // jv = n . ((w1 x p1) + u1 - (w2 x p2) - u2)
        double w1p[3], w2p[3], nw1[3], nw2[3];
        cross(v1, p1, w1p);
        cross(v2, p2, w2p);
        cross(n, v1, nw1);
        cross(n, v2, nw2);
        // (stop_contact_grad: h = Jc v is formed from a detached Jc -- no gradient to the geometry, the one to v stays)
        const double jg = (W.grad_flags & DSS_GRAD_STOP_CONTACT) ? 0.0 : jvbar;
        for (int i = 0; i < 3; ++i) {
            nbar[i] += jg * (w1p[i] + v1[3 + i] - w2p[i] - v2[3 + i]);
            p1bar[i] += jg * nw1[i];
            p2bar[i] -= jg * nw2[i];
            a_geom[(size_t)i * MX + c] = nbar[i];
        }
        for (int i = 0; i < 3; ++i) { a_geom[(size_t)(3 + i) * MX + c] = p1bar[i]; a_geom[(size_t)(6 + i) * MX + c] = p2bar[i]; }
        a_geom[(size_t)9 * MX + c] = 0.0;
        // per-contact pieces for the ordered per-body sums: velocity adjoints (12), mu, restitution
        for (int i = 0; i < 3; ++i) {
            cs[(size_t)i * MX + c] = jvbar * c1[i]; cs[(size_t)(3 + i) * MX + c] = jvbar * n[i];
            cs[(size_t)(6 + i) * MX + c] = -jvbar * c2[i]; cs[(size_t)(9 + i) * MX + c] = -jvbar * n[i];
        }
        cs[(size_t)12 * MX + c] = 0.5 * mubar;
        cs[(size_t)13 * MX + c] = 0.5 * rcbar;
    }
    __syncthreads();
    __shared__ double s_sums[64 * 8];
    {
        static constexpr int row0[8] = {0, 1, 2, 3, 4, 5, 12, 13}, row1[8] = {6, 7, 8, 9, 10, 11, 12, 13};
        contact_sums<8>(v.body_k, MX, v.nc_k, nb, cs, row0, row1, s_sums);
    }
    if (lane < nb) {
        const size_t bi = (size_t)sc * nb + lane;
        const double *vk = v.vel_k + 6 * lane, *ub = du + 6 * lane;
        double Iw[9], av[6], Iwbar[9];
        world_inertia(v.pose_k + 7 * lane, W.inertia + bi * 9, Iw);
        const double m = W.mass[bi];
        // u = M v + dt f
        for (int r = 0; r < 3; ++r) {
            av[r] = Iw[r] * ub[0] + Iw[3 + r] * ub[1] + Iw[6 + r] * ub[2];   // Iw^T ubar
            av[3 + r] = m * ub[3 + r];
        }
        double mbar = ub[3] * vk[3] + ub[4] * vk[4] + ub[5] * vk[5] + dM[36 * lane + 21] + dM[36 * lane + 28] + dM[36 * lane + 35];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Iwbar[3 * r + c] = ub[r] * vk[c] + dM[36 * lane + 6 * r + c];
        for (int i = 0; i < 6; ++i) A.g_fext[bi * 6 + i] += v.dt * ub[i];
        for (int i = 0; i < 6; ++i) av[i] += s_sums[8 * lane + i];
        const double fricb = s_sums[8 * lane + 6], restb = s_sums[8 * lane + 7];
        for (int i = 0; i < 6; ++i) a_vel[6 * lane + i] = av[i];
        A.g_mass[bi] += mbar;
        A.g_fric[bi] += fricb;
        A.g_rest[bi] += restb;
        // Iw = R Ib R^T : Ib_bar = R^T Iw_bar R (linear), q_bar by duals
        double R[9], t[9];
        quat_to_mat(v.pose_k + 7 * lane, R);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) t[3 * a + b] = R[a] * Iwbar[b] + R[3 + a] * Iwbar[3 + b] + R[6 + a] * Iwbar[6 + b];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) A.g_inertia[bi * 9 + 3 * a + b] += t[3 * a] * R[b] + t[3 * a + 1] * R[3 + b] + t[3 * a + 2] * R[6 + b];
        {
            typedef Dual<4> D;
            D q[4], Ib[9], out[9];
            for (int i = 0; i < 4; ++i) { q[i] = D(v.pose_k[7 * lane + i]); q[i].d[i] = 1.0; }
            for (int i = 0; i < 9; ++i) Ib[i] = D(W.inertia[bi * 9 + i]);
            world_inertia(q, Ib, out);
            for (int s = 0; s < 4; ++s) { double acc = 0.0; for (int e = 0; e < 9; ++e) acc += Iwbar[e] * out[e].d[s]; a_pose[7 * lane + s] += acc; }
        }
    }
    {   // u = M v + dt f : d/d(dt) = ubar . f ;  a sub-step whose dt_ was formed with last_dt hands -dt_bar back
        double part = 0.0;
        if (lane < nb) for (int i = 0; i < 6; ++i) part += du[6 * lane + i] * W.fext[((size_t)sc * nb + lane) * 6 + i];
        part = wave_sum(part);
        if (lane == 0) {
            const double dtbar = A.a_dt[sc] + part;
            A.a_last_dt[sc] = (W.tp_flags[(size_t)k * W.B + sc] & 2) ? -dtbar : 0.0;
            A.cur_slot[sc] = k - 1;
        }
    }
}

}  // namespace

extern "C" {

size_t dss_adjoint_sizeof(void) { return sizeof(DssAdjoint); }

int dss_step_backward(const DssWorld *W, const DssAdjoint *A, void *stream_)
{
    if (!W || !A || !W->tp_pose) return DSS_E_BADARG;
    // a latent code of more than three numbers comes from the latent table, and a table's adjoint needs somewhere to go
    if ((W->igr.W0 && W->igr.latent > 3 && !W->igr_latent) || (W->igr_latent && !A->g_latent)) return DSS_E_BADARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (W->shape_rare) dss::launch_bwd_pre_all(*W, *A, stream);
    else hipLaunchKernelGGL(bwd_pre_kernel, dim3(W->B), dim3(64), 0, stream, *W, *A);
    // rows of G whose dependence on the contact geometry carries gradient: 1 normal (Jc), 2 friction (Jf)
    const int rows = ((W->grad_flags & DSS_GRAD_STOP_CONTACT) ? 0 : 1) | ((W->grad_flags & DSS_GRAD_STOP_FRICTION) ? 0 : 2);
    int rc = dss::lcp_contact_backward_rows(W->Mblk, W->Je, W->cop, W->cop_body, A->bw_nc, A->bw_active, W->B, W->nb, W->neq,
                                            W->maxc, W->fric_dirs, W->x, W->tp_lam, W->tp_slack, W->nu, A->a_x, A->dMblk, A->dpvec,
                                            A->dcop, nullptr, nullptr, rows, A->cur_slot, stream_);      // (multipliers read from the tape in place)
    if (rc) return rc;
    hipLaunchKernelGGL(bwd_post_kernel, dim3(W->B), dim3(64), 0, stream, *W, *A);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_UNSUPPORTED;
}

}  // extern "C"
