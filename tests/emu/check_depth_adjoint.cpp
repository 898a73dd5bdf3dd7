// Test harness (CPU, test infrastructure): csrc/depth_adjoint.hip through the fiber emulator as a program of its own, so that it can
// be built with the address and undefined-behaviour sanitizers: every array is a heap block of exactly the size the ABI asks for,
// and a read or a write outside one ends the run.  The seams of tests/test_emu_depth_adjoint.py: images of 1 x 1, 15 x 17, 16 x 16,
// 33 x 16 and 80 x 60 pixels, 1 and (at 16 x 16 and 33 x 16) 3 views (the second shows nothing), a floor box, a sphere and a 9^3 grid body (a sampled
// sphere) rendered by the emulated dss_depth_render_grids; g_grid wanted and NULL; min_cos 1e-3 and 0.99; two calls bit-equal in
// pose, parameter and dropped outputs; the refusals (brick, a grid body without a grid, a grid id >= ngrid, a short workspace)
// with outputs untouched.  Checked against a long double loop written here in world units -- the sphere's and the box's gradients
// in closed form, the grid's weights differentiated by hand, d R / d q as four explicit matrices -- to 1e-12 of the sum of the
// absolute contributions to every output (where a contribution vanishes analytically -- a sphere's quaternion outputs, a dim that acts
// only through the scale -- of the summands that cancel, as tests/depth_adjoint_ref.py states it).  Also held: 2 phi x the terms of depth_adjoint_point.h against pointcloud_point.h's pc_point
// (d phi^2 = 2 phi d phi) on the analytic hit points, to 1e-13 of the summands' magnitude (one more rounded product each).
// Prints "<calls> calls <pixels> pixels worst <error / bound>"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../diffsdfsim_amd/csrc/depth_camera.hip"
#include "../../diffsdfsim_amd/csrc/depth_adjoint.hip"

typedef long double ld;
static double worst = 0.0;
static long npixel = 0;

static void rot(const double *q, ld R[3][3])
{
    const ld r = q[0], i = q[1], j = q[2], k = q[3], s = 2.0L / (r * r + i * i + j * j + k * k);
    const ld M[3][3] = {{1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)},
                        {s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)},
                        {s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)}};
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) R[a][b] = M[a][b];
}
// d R / d q_c of R = 1 + s N(q), s = 2 / q.q: s dN/dq_c - s^2 q_c N, the four dN written out
static void drot(const double *q, int c, ld D[3][3])
{
    const ld r = q[0], i = q[1], j = q[2], k = q[3], s = 2.0L / (r * r + i * i + j * j + k * k);
    const ld N[3][3] = {{-(j * j + k * k), i * j - k * r, i * k + j * r}, {i * j + k * r, -(i * i + k * k), j * k - i * r},
                        {i * k - j * r, j * k + i * r, -(i * i + j * j)}};
    const ld dN[4][3][3] = {{{0, -k, j}, {k, 0, -i}, {-j, i, 0}},
                            {{0, j, k}, {j, -2 * i, -r}, {k, r, -2 * i}},
                            {{-2 * j, i, r}, {i, 0, k}, {-r, k, -2 * j}},
                            {{-2 * k, -r, i}, {r, -2 * k, j}, {i, j, 0}}};
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) D[a][b] = s * dN[c][a][b] - s * s * (ld)q[c] * N[a][b];
}

struct Scene {
    int nview, nbody, W, H;
    std::vector<double> pose, prm, cam, grid;
    std::vector<int> type, gid, off, dims, blk_off;
    double fx, fy, cx, cy;
};

static Scene scene(int nview, int W, int H)
{
    Scene S;
    S.nview = nview; S.nbody = 3; S.W = W; S.H = H;
    S.fx = S.fy = 64.375 * W / 80.0; S.cx = W / 2.0; S.cy = H / 2.0;
    const double c = std::sqrt(0.5);      // the camera: 8 back along z, then Ry(pi/4) Rx(-pi/4), looking at the origin
    const double Ry[3][3] = {{c, 0, c}, {0, 1, 0}, {-c, 0, c}}, Rx[3][3] = {{1, 0, 0}, {0, c, c}, {0, -c, c}};
    S.cam.assign(16, 0.0);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) for (int k = 0; k < 3; ++k) S.cam[4 * a + b] += Ry[a][k] * Rx[k][b];
        S.cam[4 * a + 3] = S.cam[4 * a + 2] * 8.0;
    }
    S.cam[15] = 1.0;
    const int n = 9;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) for (int k = 0; k < n; ++k) {
        const double x = -1 + 2.0 * i / (n - 1) - 0.1, y = -1 + 2.0 * j / (n - 1) + 0.05, z = -1 + 2.0 * k / (n - 1);
        S.grid.push_back(std::sqrt(x * x + y * y + z * z) - 0.6);
    }
    S.off = {0}; S.dims = {n, n, n}; S.blk_off = {0};
    for (int v = 0; v < nview; ++v) {
        const double lift = v == 1 ? 100.0 : 0.0, d = 0.03 * v;
        const double P[3][7] = {{1, 0, 0, 0, 0, -0.5 + lift, 0}, {0.9, 0.2, -0.3, 0.1, -0.8 + d, 1.2 + lift, 0.3}, {1.1, 0.4, 0.2, 0.2, 1.6, 1.3 + lift + d, -0.4}};
        const double Q[3][4] = {{20, 1, 20, 0}, {1.1, 0, 0, 0}, {0, 0, 0, 1.2}};
        for (int b = 0; b < 3; ++b) { S.pose.insert(S.pose.end(), P[b], P[b] + 7); S.prm.insert(S.prm.end(), Q[b], Q[b] + 4); }
        const int T[3] = {DSS_SHAPE_BOX, DSS_SHAPE_SPHERE, DSS_SHAPE_GRID}, G[3] = {-1, -1, 0};
        S.type.insert(S.type.end(), T, T + 3); S.gid.insert(S.gid.end(), G, G + 3);
    }
    return S;
}

struct Out { std::vector<double> gp, gq, gg; std::vector<int> dr; int rc; };

static Out call(const Scene &S, const std::vector<double> &depth, const std::vector<int> &seg, const std::vector<double> &gd, double min_cos,
                bool want_grid, bool table, size_t ws_short, double fill)
{
    Out o;
    const size_t nb = (size_t)S.nview * S.nbody;
    o.gp.assign(7 * nb, fill); o.gq.assign(3 * nb, fill); o.dr.assign(nb, (int)fill); o.gg.assign(S.grid.size(), want_grid ? 0.0 : fill);
    const size_t bytes = dss_depth_adjoint_workspace_bytes(S.nview, S.nbody, S.W, S.H);
    std::vector<double> ws(bytes / 8 - ws_short / 8);      // (exactly what is declared)
    o.rc = dss_depth_adjoint(S.nview, S.nbody, S.pose.data(), S.type.data(), S.prm.data(), S.cam.data(), S.fx, S.fy, S.cx, S.cy, S.W, S.H,
                             depth.data(), seg.data(), gd.data(), min_cos, table ? S.gid.data() : nullptr, table ? 1 : 0,
                             table ? S.off.data() : nullptr, table ? S.dims.data() : nullptr, table ? S.grid.data() : nullptr, o.gp.data(),
                             o.gq.data(), want_grid ? o.gg.data() : nullptr, o.dr.data(), ws.data(), bytes - ws_short, nullptr);
    return o;
}

static int untouched(const Out &o, double fill)
{
    for (double x : o.gp) if (x != fill) return 0;
    for (double x : o.gq) if (x != fill) return 0;
    for (int x : o.dr) if (x != (int)fill) return 0;
    return 1;
}

static int run(int nview, int W, int H, double min_cos, int &ncall)
{
    Scene S = scene(nview, W, H);
    const size_t npx = (size_t)nview * W * H, nb = (size_t)nview * S.nbody;
    std::vector<double> depth(npx, 0.0), gd(npx), bmin(8);
    std::vector<int> seg(npx, -1);
    if (dss_grid_block_min(1, S.off.data(), S.dims.data(), S.grid.data(), S.blk_off.data(), 8, bmin.data(), nullptr) != 0 ||
        dss_depth_render_grids(nview, S.nbody, S.pose.data(), S.type.data(), S.prm.data(), S.cam.data(), S.fx, S.fy, S.cx, S.cy, W, H, 0.1, 100.0,
                               S.gid.data(), 1, S.off.data(), S.dims.data(), S.grid.data(), S.blk_off.data(), bmin.data(), depth.data(), seg.data(),
                               nullptr) != 0) { printf("render\n"); return 1; }
    unsigned long long lcg = 12345;
    for (size_t i = 0; i < npx; ++i) { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; gd[i] = (double)(lcg >> 11) / 9007199254740992.0 * 2.0 - 1.0; }
    Out a = call(S, depth, seg, gd, min_cos, true, true, 0, 7.0), b = call(S, depth, seg, gd, min_cos, true, true, 0, -3.0);
    Out c = call(S, depth, seg, gd, min_cos, false, true, 0, 7.0);
    ncall += 3;
    if (a.rc || b.rc || c.rc) { printf("return code\n"); return 1; }
    if (a.gp != b.gp || a.gq != b.gq || a.dr != b.dr || a.gp != c.gp || a.gq != c.gq) { printf("two calls differ\n"); return 1; }
    for (double x : c.gg) if (x != 7.0) { printf("g_grid NULL, yet written\n"); return 1; }
    // the long double loop
    std::vector<ld> gp(7 * nb, 0), gq(3 * nb, 0), gg(S.grid.size(), 0), mp(7 * nb, 0), mq(3 * nb, 0), mg(S.grid.size(), 0);
    std::vector<int> dr(nb, 0);
    for (int v = 0; v < nview; ++v)
        for (int row = 0; row < H; ++row)
            for (int col = 0; col < W; ++col) {
                const size_t px = ((size_t)v * H + row) * W + col;
                const int s = seg[px];
                if (s < 0) continue;
                ++npixel;
                const size_t vb = (size_t)v * S.nbody + s;
                const double *ps = &S.pose[7 * vb], *pr = &S.prm[4 * vb];
                const ld nx = (col + 0.5L - S.cx) / S.fx, ny = (row + 0.5L - S.cy) / S.fy, t = depth[px];
                ld R[3][3], dw[3], e[3], p[3], db[3], g[3] = {0, 0, 0}, gpr[3] = {0, 0, 0};
                rot(ps, R);
                for (int i = 0; i < 3; ++i) {
                    dw[i] = S.cam[4 * i] * nx - S.cam[4 * i + 1] * ny - S.cam[4 * i + 2];
                    e[i] = S.cam[4 * i + 3] + t * dw[i] - ps[4 + i];
                }
                for (int i = 0; i < 3; ++i) { p[i] = R[0][i] * e[0] + R[1][i] * e[1] + R[2][i] * e[2]; db[i] = R[0][i] * dw[0] + R[1][i] * dw[1] + R[2][i] * dw[2]; }
                ld sc, wt[8] = {0};
                int ci[3] = {0, 0, 0};
                if (s == 0) {      // the floor box: on a face (hits lie within 1e-10 of the surface, far from the edges)
                    sc = 15.0L;
                    int ax = 0; ld best = -1e30L;
                    for (int i = 0; i < 3; ++i) { const ld qv = fabsl(p[i]) - pr[i] / 2; if (qv > best) { best = qv; ax = i; } }
                    g[ax] = p[ax] < 0 ? -1 : 1; gpr[ax] = -0.5L;
                } else if (s == 1) {
                    sc = 1.5L * pr[0];
                    const ld n = sqrtl(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                    for (int i = 0; i < 3; ++i) g[i] = p[i] / n;
                    gpr[0] = -1;
                } else {
                    sc = pr[3];
                    ld w[3];
                    for (int i = 0; i < 3; ++i) {
                        const ld u = (p[i] / sc + 1) * 0.5L * 8;
                        ci[i] = (int)floorl(u); ci[i] = ci[i] < 0 ? 0 : (ci[i] > 7 ? 7 : ci[i]);
                        w[i] = u - ci[i];
                    }
                    for (int k = 0; k < 8; ++k) {
                        const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
                        const ld f0 = dx ? w[0] : 1 - w[0], f1 = dy ? w[1] : 1 - w[1], f2 = dz ? w[2] : 1 - w[2];
                        const ld val = S.grid[((ci[0] + dx) * 9 + ci[1] + dy) * 9 + ci[2] + dz];
                        wt[k] = sc * f0 * f1 * f2;
                        g[0] += val * (dx ? 1 : -1) * f1 * f2 * 4; g[1] += val * f0 * (dy ? 1 : -1) * f2 * 4; g[2] += val * f0 * f1 * (dz ? 1 : -1) * 4;
                    }
                }
                const ld nd = g[0] * db[0] + g[1] * db[1] + g[2] * db[2];
                const ld cosv = fabsl(nd) / (sqrtl(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) * sqrtl(nx * nx + ny * ny + 1));
                const bool in = fabsl(p[0]) <= sc && fabsl(p[1]) <= sc && fabsl(p[2]) <= sc;
                if (!(in && cosv >= (ld)min_cos && nd != 0)) { ++dr[vb]; continue; }
                const ld k = -(ld)gd[px] / nd, ak = fabsl(k);
                for (int i = 0; i < 3; ++i) {
                    ld sum = 0, mag = 0;
                    for (int j = 0; j < 3; ++j) sum += R[i][j] * g[j];
                    gp[7 * vb + 4 + i] -= k * sum; mp[7 * vb + 4 + i] += ak * fabsl(sum);
                    gq[3 * vb + i] += k * gpr[i];
                    // (the floor's first dim sets its scale and is on no visible face: only the two cancelling paths through the scale are rounded)
                    const ld dsc = (s == 0 && i == 0) ? 0.75L : 0.0L;
                    mq[3 * vb + i] += ak * (gpr[i] != 0 ? fabsl(gpr[i]) : 2 * (fabsl(p[0]) + fabsl(p[1]) + fabsl(p[2])) / sc * dsc);
                }
                for (int cq = 0; cq < 4; ++cq) {
                    ld D[3][3], sum = 0, mag = 0;
                    drot(ps, cq, D);
                    for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) { sum += e[x] * D[x][y] * g[y]; mag += fabsl(e[x] * D[x][y] * g[y]); }
                    gp[7 * vb + cq] += k * sum; mp[7 * vb + cq] += ak * (s == 1 ? mag : fabsl(sum));      // (a sphere's vanish: the summands that are rounded)
                }
                if (s == 2)
                    for (int kk = 0; kk < 8; ++kk) {
                        const size_t at = ((ci[0] + (kk >> 2)) * 9 + ci[1] + ((kk >> 1) & 1)) * 9 + ci[2] + (kk & 1);
                        gg[at] += k * wt[kk]; mg[at] += ak * wt[kk];
                    }
                if (s != 2) {      // 2 phi x this header's terms against pc_point's
                    PcSegment seg_;
                    pc_segment(seg_, ps, S.type[vb], pr);
                    const double x[3] = {(double)(e[0] + ps[4]), (double)(e[1] + ps[5]), (double)(e[2] + ps[6])};
                    double term[PC_OUT], d[3], pb[3], phi, gv[3], gm[3], chain[7];
                    if (!pc_point(seg_, x, term)) { printf("pc_point: outside\n"); return 1; }
                    pc_body_point(seg_, x, d, pb);
                    const bool ok = s == 0 ? da_analytic<SHAPE_BOX>(seg_, pb, phi, gv, gm) : da_analytic<SHAPE_SPHERE>(seg_, pb, phi, gv, gm);
                    da_pose_chain(seg_, d, pb, gv, chain);
                    if (!ok || phi * phi != term[0]) { printf("phi^2 differs from pc_point's\n"); return 1; }
                    for (int i = 0; i < 10; ++i) {
                        const double mine = 2.0 * phi * (i < 7 ? chain[i] : gm[i - 7]);
                        if (std::fabs(mine - term[2 + i]) > 1e-13 * std::fabs(2.0 * phi) * 60.0) { printf("term %d: %.17g vs pc_point %.17g\n", i, mine, term[2 + i]); return 1; }
                    }
                }
            }
    for (size_t i = 0; i < nb; ++i) if (dr[i] != a.dr[i]) { printf("dropped[%zu]: %d, want %d\n", i, a.dr[i], dr[i]); return 1; }
    auto hold = [&](const char *what, const std::vector<double> &got, const std::vector<ld> &want, const std::vector<ld> &mag) {
        for (size_t i = 0; i < got.size(); ++i) {
            if (mag[i] == 0) { if (got[i] != 0.0) { printf("%s[%zu] = %.17g, want exactly 0\n", what, i, got[i]); return 1; } continue; }
            const ld err = fabsl(got[i] - want[i]), bound = 1e-12L * mag[i];
            if (!(err <= bound)) { printf("%s[%zu]: %.17g, want %.17Lg (bound %.3Lg)\n", what, i, got[i], want[i], bound); return 1; }
            if ((double)(err / bound) > worst) worst = (double)(err / bound);
        }
        return 0;
    };
    return hold("g_pose", a.gp, gp, mp) || hold("g_prm", a.gq, gq, mq) || hold("g_grid", a.gg, gg, mg);
}

int main()
{
    int ncall = 0;
    const int sizes[5][2] = {{1, 1}, {15, 17}, {16, 16}, {33, 16}, {80, 60}};
    for (const auto &wh : sizes)      // (three views at the sizes of one and of several ragged workgroups: the program stays quick)
        for (int nview : {1, 3})
            if ((nview == 1 || wh[0] == 16 || wh[0] == 33) && run(nview, wh[0], wh[1], 1e-3, ncall)) return 1;
    if (run(1, 33, 16, 0.99, ncall)) return 1;
    // refusals: nothing is written (the outputs keep their fill; a null output would be dereferenced otherwise)
    Scene S = scene(3, 16, 16);
    std::vector<double> depth(3 * 256, 5.0), gd(3 * 256, 1.0);
    std::vector<int> seg(3 * 256, 2);
    auto refused = [&](Scene T, bool table, size_t ws_short, int want) {
        Out o = call(T, depth, seg, gd, 1e-3, false, table, ws_short, -7.0);
        ++ncall;
        return o.rc == want && untouched(o, -7.0);
    };
    Scene brick = S, nogrid = S, badid = S, baddim = S;
    brick.type[4] = DSS_SHAPE_BRICK; nogrid.gid[8] = -1; badid.gid[8] = 1; baddim.dims[1] = 1;
    if (!refused(brick, true, 0, DSS_E_UNSUPPORTED) || !refused(nogrid, true, 0, DSS_E_UNSUPPORTED) || !refused(S, false, 0, DSS_E_UNSUPPORTED) ||
        !refused(badid, true, 0, DSS_E_BADARG) || !refused(baddim, true, 0, DSS_E_BADARG) || !refused(S, true, 8, DSS_E_WORKSPACE)) {
        printf("refusals\n");
        return 1;
    }
    printf("%d calls %ld pixels worst %.3f\n", ncall, npixel, worst);
    return 0;
}
