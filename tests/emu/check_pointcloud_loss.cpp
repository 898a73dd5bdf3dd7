// Test harness (CPU, test infrastructure): the per-point body of the point-cloud loss (csrc/pointcloud_point.h, geom.h on
// Dual<6> plus the hand-written chain to the pose) against a long double restatement of the value and long double central
// differences for the ten derivatives, on random points per primitive: anywhere in and around the query cube, inside the
// body, in the edge and corner regions of the box family, outside the cube.
// Prints "<cases> <inside> value <worst> deriv <worst>"; exit code 1 on a mask mismatch or a deviation above the bounds below.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../../diffsdfsim_amd/csrc/pointcloud_point.h"

using namespace dss;
typedef long double L;
static double rnd() { return rand() / (double)RAND_MAX; }

static L lmax(L a, L b) { return a > b ? a : b; }
static L lmin(L a, L b) { return a < b ? a : b; }
static L pos_part(L a) { return a > 0 ? a : 0; }

static L scale_of(int type, const L *prm)
{
    if (type == SHAPE_SPHERE) return 1.5L * prm[0];
    if (type == SHAPE_CYLINDER) return 1.5L * lmax(prm[0], prm[1] / 2);
    if (type == SHAPE_BOWL) return (prm[0] + prm[1]) * 1.3333L;
    return 1.5L * lmax(lmax(prm[0], prm[1]), prm[2]) / 2;
}

// the primitives of sdf_physics/physics3d/bodies.py:38-185 in the unit frame, times the scale
static L sdf_ref(int type, const L *prm, L rc, const L *pw)
{
    const L s = scale_of(type, prm);
    const L p[3] = {pw[0] / s, pw[1] / s, pw[2] / s};
    L u = 0;
    if (type == SHAPE_BOX || type == SHAPE_BOX_ROUNDED) {
        const L r = type == SHAPE_BOX ? 0 : rc;
        L q[3];
        for (int i = 0; i < 3; ++i) q[i] = fabsl(p[i]) - (prm[i] - 2 * r) / s / 2;
        u = sqrtl(pos_part(q[0]) * pos_part(q[0]) + pos_part(q[1]) * pos_part(q[1]) + pos_part(q[2]) * pos_part(q[2])) +
            lmin(lmax(lmax(q[0], q[1]), q[2]), 0) - r / s;
    } else if (type == SHAPE_BRICK) {
        const L hr = rc / s;
        const L q0 = fabsl(p[0]) - (prm[0] / s / 2 - hr), q1 = fabsl(p[1]) - (prm[1] / s / 2 - hr), q2 = fabsl(p[2]) - prm[2] / s / 2;
        const L s01 = sqrtl(pos_part(q0) * pos_part(q0) + pos_part(q1) * pos_part(q1)) + lmin(lmax(q0, q1), 0) - hr;
        u = sqrtl(pos_part(s01) * pos_part(s01) + pos_part(q2) * pos_part(q2)) + lmin(lmax(s01, q2), 0);
    } else if (type == SHAPE_CYLINDER) {
        const L rho = sqrtl(p[0] * p[0] + p[1] * p[1]);
        const L q0 = rho - prm[0] / s, q1 = fabsl(p[2]) - prm[1] / s / 2;
        u = sqrtl(pos_part(q0) * pos_part(q0) + pos_part(q1) * pos_part(q1)) + lmin(lmax(q0, q1), 0);
    } else if (type == SHAPE_BOWL) {
        const L r = prm[0] / s, d = prm[1] / s, z = p[2] - r / 2, rho = sqrtl(p[0] * p[0] + p[1] * p[1]);
        L a = z < 0 ? sqrtl(rho * rho + z * z) : rho;
        a = fabsl(a - r) - d;
        u = sqrtl(pos_part(a) * pos_part(a) + pos_part(z) * pos_part(z)) + lmin(0, lmax(a, z));
    } else {
        u = sqrtl(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) - prm[0] / s;
    }
    return u * s;
}

static void body_point(const L *v /*pose[7], prm[3]*/, const L *x, L *p)
{
    const L r = v[0], i = v[1], j = v[2], k = v[3], ts = 2 / (r * r + i * i + j * j + k * k);
    const L R[9] = {1 - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r), ts * (i * j + k * r), 1 - ts * (i * i + k * k),
                    ts * (j * k - i * r), ts * (i * k - j * r), ts * (j * k + i * r), 1 - ts * (i * i + j * j)};
    const L d[3] = {x[0] - v[4], x[1] - v[5], x[2] - v[6]};
    for (int c = 0; c < 3; ++c) p[c] = R[c] * d[0] + R[3 + c] * d[1] + R[6 + c] * d[2];
}

// phi^2 as a function of the ten variables (the mask is decided at the point itself, not here)
static L loss_ref(int type, const L *v, L rc, const L *x)
{
    L p[3];
    body_point(v, x, p);
    const L phi = sdf_ref(type, v + 7, rc, p);
    return phi * phi;
}

int main()
{
    srand(11);
    // Bounds.  Value: ~100 double operations of relative error 2^-53 each on numbers of order one -> 1e-14; held to 1e-12.
    // Derivatives: central differences in long double with h = 1e-7: truncation h^2 / 6 |f'''| < 2e-15 |f'''|, rounding
    // ~ 1e-19 |f| / h = 1e-12 |f|; with |f'''| up to ~1e3 away from the singular sets (points closer than 0.05 to the centre
    // or the axis are not drawn) both stay below 1e-11; held to 1e-9 max(1, |derivative|).
    const L h = 1e-7L;
    const double tol_v = 1e-12, tol_d = 1e-9;
    double worst_v = 0.0, worst_d = 0.0;
    int ncase = 0, nin = 0, bad_mask = 0;
    for (int type = SHAPE_BOX; type <= SHAPE_BOWL; ++type) {
        for (int it = 0; it < 2000; ++it) {
            double pose[7], prm4[4] = {0.0, 0.0, 0.0, 0.0};
            double n2 = 0.0;
            for (int i = 0; i < 4; ++i) { pose[i] = rnd() - 0.5; n2 += pose[i] * pose[i]; }
            const double qn = (it % 3 == 0) ? 0.7 + 0.8 * rnd() : 1.0;      // every third quaternion is not of unit length
            for (int i = 0; i < 4; ++i) pose[i] *= qn / sqrt(n2);
            for (int i = 0; i < 3; ++i) pose[4 + i] = 4.0 * (rnd() - 0.5);
            // distinct parameters: the largest dim (the scale) is a kink where two are equal
            if (type == SHAPE_SPHERE) prm4[0] = 0.4 + rnd();
            else if (type == SHAPE_CYLINDER) { prm4[0] = 0.3 + 0.5 * rnd(); prm4[1] = 0.5 + 1.5 * rnd(); }
            else if (type == SHAPE_BOWL) { prm4[0] = 0.5 + 0.5 * rnd(); prm4[1] = 0.05 + 0.1 * rnd(); }
            else { prm4[0] = 0.6 + 0.2 * rnd(); prm4[1] = 0.9 + 0.2 * rnd(); prm4[2] = 1.2 + 0.3 * rnd(); }
            if (type == SHAPE_BOX_ROUNDED || type == SHAPE_BRICK) prm4[3] = 0.05 + 0.15 * rnd();
            L v[10];
            for (int i = 0; i < 7; ++i) v[i] = pose[i];
            for (int i = 0; i < 3; ++i) v[7 + i] = prm4[i];
            const L sc = scale_of(type, v + 7);
            // a body-frame point of the wanted kind, then its world-frame image (rounded to double: that IS the input)
            double pb[3], x[3];
            L xl[3], pl[3];
            bool ok = false;
            for (int tries = 0; tries < 100 && !ok; ++tries) {
                const int kind = it % 4;
                const double hd[3] = {type <= SHAPE_SPHERE || type >= SHAPE_BOX_ROUNDED ? prm4[0] / 2 : prm4[0],
                                      type == SHAPE_CYLINDER ? prm4[0] : prm4[1] / 2, type == SHAPE_CYLINDER ? prm4[1] / 2 : prm4[2] / 2};
                for (int i = 0; i < 3; ++i) {
                    const double sg = rnd() < 0.5 ? -1.0 : 1.0;
                    if (kind == 0) pb[i] = 1.25 * (double)sc * (2 * rnd() - 1);                       // in and around the query cube
                    else if (kind == 1) pb[i] = 0.9 * (type == SHAPE_SPHERE || type == SHAPE_BOWL ? 0.55 * prm4[0] : hd[i]) * (2 * rnd() - 1);   // inside the body
                    else if (kind == 2) pb[i] = sg * (type == SHAPE_SPHERE || type == SHAPE_BOWL ? prm4[0] : hd[i]) * (1.02 + 0.3 * rnd());      // corner regions
                    else pb[i] = i == (it / 4) % 3 ? 0.5 * hd[i] * (2 * rnd() - 1)                                                             // edge regions
                                                   : sg * (type == SHAPE_SPHERE || type == SHAPE_BOWL ? prm4[0] : hd[i]) * (1.02 + 0.3 * rnd());
                }
                if (it % 16 == 15) pb[it % 3] = (rnd() < 0.5 ? -1.0 : 1.0) * (double)sc * (1.05 + rnd());   // certainly outside the cube
                double R[9];
                quat_to_mat(pose, R);
                for (int i = 0; i < 3; ++i) { x[i] = R[3 * i] * pb[0] + R[3 * i + 1] * pb[1] + R[3 * i + 2] * pb[2] + pose[4 + i]; xl[i] = x[i]; }
                body_point(v, xl, pl);
                ok = true;
                for (int i = 0; i < 3; ++i) ok = ok && fabsl(fabsl(pl[i]) - sc) > 1e-6L;                  // the mask cannot flip on a last bit
                ok = ok && sqrtl(pl[0] * pl[0] + pl[1] * pl[1]) > 0.05L && sqrtl(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2]) > 0.05L;
            }
            if (!ok) { printf("no admissible point, type %d case %d\n", type, it); return 1; }
            const bool in_ref = fabsl(pl[0]) <= sc && fabsl(pl[1]) <= sc && fabsl(pl[2]) <= sc;
            PcSegment S;
            pc_segment(S, pose, type, prm4);
            double term[PC_OUT];
            const bool in = pc_point(S, x, term);
            ++ncase;
            if (in != in_ref) { ++bad_mask; continue; }
            if (!in) continue;
            ++nin;
            const L f0 = loss_ref(type, v, prm4[3], xl);
            const double ev = (double)(fabsl(term[0] - f0) / lmax(1, fabsl(f0)));
            if (ev > worst_v) worst_v = ev;
            if (term[1] != 1.0) ++bad_mask;
            for (int k = 0; k < 10; ++k) {
                L vp[10], vm[10];
                for (int i = 0; i < 10; ++i) { vp[i] = v[i]; vm[i] = v[i]; }
                vp[k] += h; vm[k] -= h;
                const L fd = (loss_ref(type, vp, prm4[3], xl) - loss_ref(type, vm, prm4[3], xl)) / (2 * h);
                const double ed = (double)(fabsl(term[2 + k] - fd) / lmax(1, fabsl(fd)));
                if (ed > worst_d) {
                    worst_d = ed;
                    if (ed > tol_d) printf("type %d case %d output %d: %.15g vs %.15Lg\n", type, it, 2 + k, term[2 + k], fd);
                }
            }
        }
    }
    printf("%d %d value %.3e deriv %.3e\n", ncase, nin, worst_v, worst_d);
    return (bad_mask || worst_v > tol_v || worst_d > tol_d) ? 1 : 0;
}
