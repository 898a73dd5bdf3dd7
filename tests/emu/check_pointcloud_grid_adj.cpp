// Test harness (CPU, test infrastructure): dss_pointcloud_loss_grids_adjoint of csrc/pointcloud_loss_grid_adj.hip through the fiber
// emulator as a program of its own, so that it can be built with the address and undefined-behaviour sanitizers.  g_data is a
// heap block of exactly the table's size plus one guard word that must come back untouched (a write further out ends the run
// under the sanitizer).
// Walked: a table of 2x3x5, 3x3x3 (unused), 5x4x3, 9x9x9 and 4x3x2 samples; segments of 0, 1, 64, 65 and 2049 points (two chunks; the
// 64 points, one full wavefront, all inside the cube and alone on the 4x3x2 grid, every sample of which they must reach); points
// with |u_d| = 1 exactly on 1 - 3 axes (they count, the last cell clamped), with u_d = +-(1 + 2^-40) (they add nothing), on nodes
// and cell faces, and anywhere; two segments on one grid under weights of different sign, a segment of weight 0, an analytic
// segment; a pre-filled g_data (add semantics); the refused calls (null pointers, nseg 0, ngrid -1, a grid id past the table, a
// dim of 1, a neural segment, a grid segment without a grid), after each of which g_data must be what it was.  Every sample is
// compared with a long double restatement written here, to 1e-12 of the sum of its terms' magnitudes (plus what the float64
// rounding of phi itself moves a term by, which matters where phi nearly cancels).  On every point of every grid segment
// pc_grid_point must decide membership as pc_point does and its phi^2 must be pc_point's term[0] bit for bit: the value is
// stated in both (pointcloud_point.h says why), and this is what keeps the two statements one.
// Prints "<launches> launches <n> samples with a gradient"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../diffsdfsim_amd/csrc/pointcloud_loss_grid_adj.hip"

typedef long double L;
static const double GUARD = -7.25;
static double rnd() { return rand() / (double)RAND_MAX; }

struct Seg { std::vector<double> pts; double pose[7]; int type; double scale; int grid; double weight; };

struct Table {
    std::vector<int> off, dims;
    std::vector<double> data;
    void add(int n0, int n1, int n2)
    {
        off.push_back((int)data.size());
        dims.push_back(n0); dims.push_back(n1); dims.push_back(n2);
        for (int k = 0; k < n0 * n1 * n2; ++k) data.push_back(2.0 * rnd() - 1.0);
    }
};

// the restatement: terms per sample in long double, sum and sum of magnitudes
// slack: what the kernel's own float64 rounding of phi (8 products, 7 additions: below 16 x 2^-53 of sum w |s|) moves a term by
static void restate(const std::vector<Seg> &segs, const Table &T, std::vector<L> &sum, std::vector<L> &mag, std::vector<L> &slack)
{
    sum.assign(T.data.size(), 0); mag.assign(T.data.size(), 0); slack.assign(T.data.size(), 0);
    for (const Seg &S : segs) {
        if (S.type != 7 || S.grid < 0) continue;
        const L r = S.pose[0], i = S.pose[1], j = S.pose[2], k = S.pose[3], s = 2 / (r * r + i * i + j * j + k * k);
        const L R[3][3] = {{1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)}, {s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)},
                           {s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)}};
        const int *n = &T.dims[3 * S.grid];
        const double *G = &T.data[T.off[S.grid]];
        for (size_t p = 0; p < S.pts.size() / 3; ++p) {
            L u[3], f[3];
            int c[3];
            bool in = true;
            for (int a = 0; a < 3; ++a) {
                u[a] = 0;
                for (int b = 0; b < 3; ++b) u[a] += R[b][a] * ((L)S.pts[3 * p + b] - S.pose[4 + b]);
                in = in && fabsl(u[a]) <= S.scale;
                const L ind = (u[a] / S.scale + 1) / 2 * (n[a] - 1);
                c[a] = (int)floorl(ind);
                c[a] = c[a] < 0 ? 0 : (c[a] > n[a] - 2 ? n[a] - 2 : c[a]);
                f[a] = ind - c[a];
            }
            if (!in) continue;
            L phi = 0, rough = 0;
            for (int m = 0; m < 8; ++m) {
                const int dx = m >> 2, dy = (m >> 1) & 1, dz = m & 1;
                const L t = (dx ? f[0] : 1 - f[0]) * (dy ? f[1] : 1 - f[1]) * (dz ? f[2] : 1 - f[2]) * G[((c[0] + dx) * n[1] + c[1] + dy) * n[2] + c[2] + dz];
                phi += t; rough += fabsl(t);
            }
            phi *= S.scale;
            for (int m = 0; m < 8; ++m) {
                const int dx = m >> 2, dy = (m >> 1) & 1, dz = m & 1;
                const L t = 2 * S.weight * phi * S.scale * (dx ? f[0] : 1 - f[0]) * (dy ? f[1] : 1 - f[1]) * (dz ? f[2] : 1 - f[2]);
                const size_t at = T.off[S.grid] + ((c[0] + dx) * n[1] + c[1] + dy) * n[2] + c[2] + dz;
                sum[at] += t; mag[at] += fabsl(t);
                if (phi != 0) slack[at] += fabsl(t / phi) * 16 * 1.12e-16L * rough * S.scale;
            }
        }
    }
}

struct Packed {
    std::vector<int> off{0}, type, gid;
    std::vector<double> pts, pose, prm, w;
    int max_len = 0;
    explicit Packed(const std::vector<Seg> &segs)
    {
        for (const Seg &S : segs) {
            pts.insert(pts.end(), S.pts.begin(), S.pts.end());
            off.push_back(off.back() + (int)S.pts.size() / 3);
            if ((int)S.pts.size() / 3 > max_len) max_len = (int)S.pts.size() / 3;
            type.push_back(S.type); gid.push_back(S.grid); w.push_back(S.weight);
            pose.insert(pose.end(), S.pose, S.pose + 7);
            const double row[4] = {S.type == 7 ? 0.0 : 0.4, 0.0, 0.0, S.type == 7 ? S.scale : 0.0};
            prm.insert(prm.end(), row, row + 4);
        }
        if (pts.empty()) pts.push_back(0.0);
    }
};

static long launches = 0;
static int call(const Packed &P, const Table &T, std::vector<double> &g, int nseg = -1, int ngrid = -99)
{
    ++launches;
    return dss_pointcloud_loss_grids_adjoint(nseg < 0 ? (int)P.type.size() : nseg, P.max_len, P.off.data(), P.pts.data(), P.pose.data(), P.type.data(),
                                             P.prm.data(), P.gid.data(), ngrid == -99 ? (int)T.off.size() : ngrid, T.off.data(), T.dims.data(),
                                             T.data.data(), P.w.data(), g.data(), nullptr);
}

int main()
{
    srand(11);
    Table T;
    T.add(2, 3, 5); T.add(3, 3, 3); T.add(5, 4, 3); T.add(9, 9, 9); T.add(4, 3, 2);
    const double ex[7] = {2.0, 0.0, 0.0, 0.0, 0.25, -0.5, 1.0};      // the identity rotation from a raw quaternion of norm 2
    auto seg = [](int n, const double *pose, int type, double scale, int grid, double weight, double reach = 1.4) {
        Seg S; S.type = type; S.scale = scale; S.grid = grid; S.weight = weight;
        std::memcpy(S.pose, pose, sizeof S.pose);
        for (int k = 0; k < 3 * n; ++k) S.pts.push_back(pose[4 + k % 3] + (2.0 * rnd() - 1.0) * reach * scale);
        return S;
    };
    auto exact = [&](Seg &S, int k, double ux, double uy, double uz) {
        S.pts[3 * k] = ex[4] + 0.5 * ux; S.pts[3 * k + 1] = ex[5] + 0.5 * uy; S.pts[3 * k + 2] = ex[6] + 0.5 * uz;
    };
    const double pa[7] = {0.7, -0.3, 0.5, 0.2, 0.1, 0.2, -0.3}, pb[7] = {-0.4, 1.1, 0.3, -0.8, -1.0, 0.5, 0.2};
    std::vector<Seg> segs = {seg(2049, pa, 7, 0.8, 0, 1.3), seg(65, pb, 7, 1.7, 0, -0.7), seg(65, pa, 7, 1.1, 2, 0.9), seg(65, pb, 7, 1.1, 2, 0.0),
                             seg(64, pa, 1, 0.0, -1, 1.0), seg(65, ex, 7, 0.5, 3, 1.1), seg(1, ex, 7, 0.5, 3, -2.0), seg(0, ex, 7, 0.5, 3, 1.0),
                             seg(65, ex, 7, 0.5, 3, 1.0), seg(64, pb, 7, 1.3, 4, -0.4, 0.55)};      // (0.55 sqrt 3 < 1: all inside)
    const double eps = ldexp(1.0, -40);
    for (int k = 0; k < 65; ++k) {
        const double a = (k % 127 - 63) / 64.0, b = ((k * 7) % 127 - 63) / 64.0, sg = k % 2 ? 1.0 : -1.0;
        if (k < 20) exact(segs[5], k, k % 3 == 0 ? sg : a, k % 3 == 1 ? sg : b, k % 3 == 2 ? -sg : a);           // one face
        else if (k < 30) exact(segs[5], k, sg, -sg, b);                                                            // an edge
        else if (k < 38) exact(segs[5], k, k & 1 ? 1.0 : -1.0, k & 2 ? 1.0 : -1.0, k & 4 ? 1.0 : -1.0);            // the corners
        else if (k < 50) exact(segs[5], k, (k % 9) / 4.0 - 1.0, ((k * 5) % 9) / 4.0 - 1.0, ((k * 2) % 9) / 4.0 - 1.0);   // nodes
        else exact(segs[5], k, (k % 9) / 4.0 - 1.0, a, b);                                                         // cell faces
        exact(segs[8], k, k % 3 == 0 ? sg * (1.0 + eps) : a, k % 3 == 1 ? sg * (1.0 + eps) : b, k % 3 == 2 ? -sg * (1.0 + eps) : a);   // just outside
    }
    exact(segs[6], 0, 0.25, -0.5, 0.75);
    const Packed P(segs);
    std::vector<L> sum, mag, slack;
    restate(segs, T, sum, mag, slack);
    const size_t N = T.data.size();
    long with = 0;
    for (size_t k = T.off[4]; k < N; ++k) if (mag[k] == 0) { printf("the 64-point segment does not reach sample %zu of its grid\n", k); return 1; }
    // the value as the adjoint states it against the value the forward squares
    for (size_t si = 0; si < segs.size(); ++si) {
        const Seg &Sg = segs[si];
        if (Sg.type != 7) continue;
        const double prm4[4] = {0.0, 0.0, 0.0, Sg.scale};
        dss::PcSegment S;
        dss::pc_segment(S, Sg.pose, dss::SHAPE_GRID, prm4);
        S.shape.grid = &T.data[T.off[Sg.grid]];
        for (int a = 0; a < 3; ++a) S.shape.gn[a] = T.dims[3 * Sg.grid + a];
        long in = 0;
        for (size_t p = 0; p < Sg.pts.size() / 3; ++p) {
            double term[dss::PC_OUT], w[3], phi = 0.0;
            int i0[3];
            const bool a = dss::pc_point(S, &Sg.pts[3 * p], term), b = dss::pc_grid_point(S, &Sg.pts[3 * p], i0, w, phi);
            const double sq = phi * phi;
            if (a != b || (a && std::memcmp(&sq, &term[0], 8))) { printf("segment %zu point %zu: the two statements of the value differ\n", si, p); return 1; }
            in += a;
        }
        if (si == 9 && in != 64) { printf("the 64-point segment has %ld points inside\n", in); return 1; }
        if (si == 8 && in != 0) { printf("%ld points at 1 + 2^-40 count\n", in); return 1; }
    }
    for (int pre = 0; pre < 2; ++pre) {      // zeroed, then pre-filled: the call adds
        std::vector<double> g(N + 1, pre ? 3.0 : 0.0);
        g[N] = GUARD;
        if (call(P, T, g) != 0 || g[N] != GUARD) { printf("status or guard word\n"); return 1; }
        for (size_t k = 0; k < N; ++k) {
            const L got = (L)g[k] - (pre ? 3.0 : 0.0);
            if (mag[k] == 0 ? g[k] != (pre ? 3.0 : 0.0) : fabsl(got - sum[k]) > 1e-12L * mag[k] + slack[k] + (pre ? 3.0 * 2.3e-16 : 0.0)) {
                printf("sample %zu: %.17g, restated %.17Lg (magnitudes %.3Lg)\n", k, g[k], sum[k], mag[k]);
                return 1;
            }
            if (!pre) with += mag[k] != 0;
        }
        for (size_t k = T.off[1]; k < (size_t)T.off[2]; ++k) if (g[k] != (pre ? 3.0 : 0.0)) { printf("the unused grid got a gradient\n"); return 1; }
    }
    // the segment just outside alone: nothing
    {
        const Packed Q(std::vector<Seg>{segs[8]});
        std::vector<double> g(N + 1, 0.0);
        g[N] = GUARD;
        if (call(Q, T, g) != 0 || g[N] != GUARD) { printf("outside: status or guard word\n"); return 1; }
        for (size_t k = 0; k < N; ++k) if (g[k] != 0.0) { printf("a point at 1 + 2^-40 added to sample %zu\n", k); return 1; }
    }
    // refused calls leave g_data as it was
    {
        std::vector<double> g(N + 1, 5.0), keep;
        g[N] = GUARD; keep = g;
        int bad = 0;
        bad += call(P, T, g, 0) != DSS_E_BADARG;
        bad += call(P, T, g, -1, -1) != DSS_E_BADARG;           // ngrid -1
        launches += 3;
        bad += dss_pointcloud_loss_grids_adjoint((int)P.type.size(), P.max_len, P.off.data(), P.pts.data(), P.pose.data(), P.type.data(), P.prm.data(),
                                                 P.gid.data(), (int)T.off.size(), T.off.data(), T.dims.data(), T.data.data(), nullptr, g.data(), nullptr) != DSS_E_BADARG;
        bad += dss_pointcloud_loss_grids_adjoint((int)P.type.size(), P.max_len, P.off.data(), P.pts.data(), P.pose.data(), P.type.data(), P.prm.data(),
                                                 P.gid.data(), (int)T.off.size(), T.off.data(), T.dims.data(), T.data.data(), P.w.data(), nullptr, nullptr) != DSS_E_BADARG;
        bad += dss_pointcloud_loss_grids_adjoint((int)P.type.size(), P.max_len, nullptr, P.pts.data(), P.pose.data(), P.type.data(), P.prm.data(),
                                                 P.gid.data(), (int)T.off.size(), T.off.data(), T.dims.data(), T.data.data(), P.w.data(), g.data(), nullptr) != DSS_E_BADARG;
        bad += call(P, T, g, -1, 3) != DSS_E_BADARG;           // segments of grid 3 with a table of 3
        Table T1 = T; T1.dims[4] = 1;
        bad += call(P, T1, g) != DSS_E_BADARG;                 // a dim below 2
        Packed N6 = P; N6.type[2] = 6;
        bad += call(N6, T, g) != DSS_E_UNSUPPORTED;            // a neural segment
        Packed N7 = P; N7.gid[2] = -1;
        bad += call(N7, T, g) != DSS_E_UNSUPPORTED;            // a grid segment without a grid
        if (bad || std::memcmp(g.data(), keep.data(), g.size() * 8)) { printf("%d refused calls with another status, or g_data written\n", bad); return 1; }
    }
    printf("%ld launches %ld samples with a gradient\n", launches, with);
    return 0;
}
