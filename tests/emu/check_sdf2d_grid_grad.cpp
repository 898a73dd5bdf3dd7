// Test harness (CPU, test infrastructure): dss_sdf2d_contacts_backward_grids of csrc/sdf2d_contacts.hip through the fiber
// emulator as a program of its own, so that it can be built with the address and undefined-behaviour sanitizers.  g_vals,
// g_grads and g_verts are heap blocks of exactly the size of the table plus one guard word that must come back untouched (a
// write further out ends the run under the sanitizer); the other outputs likewise.
// Walked: a table of one 2 x 2 grid (every central difference zero: no contact, nothing added), of one 3 x 3 grid, of one
// 5 x 9 grid (x slowest), of two grids (offsets of all three arrays), one grid shared by three pairs (its gradient against
// the sum of the three pairs launched alone, 1e-12 of the largest entry), a pair of a grid with itself, a pair with count 0, a pair flagged over `cap` (contributes nothing), a null output (DSS_E_BADARG).  After every
// launch g_pose, g_prm, g_scale must be the bits dss_sdf2d_contacts_backward writes, and a second call the same bits where no
// grid is shared.  Prints "<launches> launches <entries> table entries with a gradient"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../diffsdfsim_amd/csrc/sdf2d_contacts.hip"

static const double GUARD = -7.25;
static long launches = 0, entries = 0;

struct Table {
    std::vector<int> dims, val_off, vert_off{0}, edge_off{0}, edges;
    std::vector<double> vals, grads, verts;
    void differences(size_t base, int n0, int n1)
    {
        for (int i = 0; i < n0; ++i)
            for (int j = 0; j < n1; ++j) {
                grads.push_back(i == 0 || i == n0 - 1 ? 0.0 : (vals[base + (size_t)(i + 1) * n1 + j] - vals[base + (size_t)(i - 1) * n1 + j]) / 2.0);
                grads.push_back(j == 0 || j == n1 - 1 ? 0.0 : (vals[base + (size_t)i * n1 + j + 1] - vals[base + (size_t)i * n1 + j - 1]) / 2.0);
            }
    }
    // a disc of radius 0.3 sampled n0 x n1 over [-0.5, 0.5]^2, its outline a regular polygon of ne edges
    void add_disc(int n0, int n1, int ne)
    {
        dims.push_back(n0); dims.push_back(n1);
        val_off.push_back((int)vals.size());
        const size_t base = vals.size();
        for (int i = 0; i < n0; ++i)
            for (int j = 0; j < n1; ++j) {
                const double x = -0.5 + (double)i / (n0 - 1), y = -0.5 + (double)j / (n1 - 1);
                vals.push_back(std::sqrt(x * x + y * y) - 0.3);
            }
        differences(base, n0, n1);
        for (int k = 0; k < ne; ++k) {
            verts.push_back(0.3 * std::cos(2.0 * M_PI * k / ne)); verts.push_back(0.3 * std::sin(2.0 * M_PI * k / ne));
            edges.push_back(k); edges.push_back((k + 1) % ne);
        }
        vert_off.push_back(vert_off.back() + ne); edge_off.push_back(edge_off.back() + ne);
    }
    // 2 x 2 samples with one corner inside: an outline of one edge
    void add_corner()
    {
        dims.push_back(2); dims.push_back(2);
        val_off.push_back((int)vals.size());
        const size_t base = vals.size();
        for (double v : {-0.1, 0.2, 0.2, 0.3}) vals.push_back(v);
        differences(base, 2, 2);
        for (double v : {-0.5, -1.0 / 6.0, -1.0 / 6.0, -0.5}) verts.push_back(v);
        edges.push_back(0); edges.push_back(1);
        vert_off.push_back(vert_off.back() + 2); edge_off.push_back(edge_off.back() + 1);
    }
    DssSdf2dGrids c() const
    {
        return DssSdf2dGrids{(int)dims.size() / 2, dims.data(), val_off.data(), vert_off.data(), edge_off.data(), edges.data(), vals.data(),
                             grads.data(), verts.data()};
    }
};

struct Side { int kind; double rot, x, y, p0, p1, scale; int grid; };
struct Pair { Side a, b; };

static std::vector<double> dbl(size_t n, double fill) { std::vector<double> v(n + 1, fill); v[n] = GUARD; return v; }

// forward with a roomy or a given cap, then the new backward (twice) and the old one.  counts: what the forward found.  0: fine
static int launch(const std::vector<Pair> &pairs, const Table &T, int cap, bool shared, std::vector<int> &counts, std::vector<int> &status,
                  std::vector<double> *table_grad = nullptr)
{
    const int P = (int)pairs.size();
    std::vector<int> kind(2 * P), gid(2 * P);
    std::vector<double> pose(6 * P), prm(4 * P), scale(2 * P);
    for (int p = 0; p < P; ++p)
        for (int s = 0; s < 2; ++s) {
            const Side &b = s ? pairs[p].b : pairs[p].a;
            const size_t o = (size_t)s * P + p;
            kind[o] = b.kind; gid[o] = b.grid; scale[o] = b.scale;
            pose[3 * o] = b.rot; pose[3 * o + 1] = b.x; pose[3 * o + 2] = b.y;
            prm[2 * o] = b.p0; prm[2 * o + 1] = b.p1;
        }
    const DssSdf2dGrids G = T.c();
    std::vector<double> out((size_t)P * cap * 7), tpar((size_t)P * cap);
    std::vector<int> count(P), st(P), tag((size_t)P * cap * 2);
    int rc = dss_sdf2d_contacts_forward(P, cap, kind.data(), pose.data(), prm.data(), scale.data(), gid.data(), &G, 0.1, out.data(), count.data(),
                                        st.data(), tag.data(), tpar.data(), 0, nullptr, nullptr, nullptr, nullptr);
    ++launches;
    if (rc != 0) { printf("forward status %d\n", rc); return 1; }
    counts = count; status = st;
    std::vector<double> gout((size_t)P * cap * 7);
    // (a row's upstream gradient depends on its place within its pair only, so that a pair gets the same one in any launch of this cap)
    for (size_t k = 0; k < gout.size(); ++k) gout[k] = 0.25 + 0.125 * (double)(k % ((size_t)cap * 7) % 11);
    std::vector<double> keep[3];
    for (int call = 0; call < 2; ++call) {
        std::vector<double> g_pose = dbl(6 * (size_t)P, 3.0), g_prm = dbl(4 * (size_t)P, 3.0), g_scale = dbl(2 * (size_t)P, 3.0);
        std::vector<double> g_vals = dbl(T.vals.size(), 0.0), g_grads = dbl(T.grads.size(), 0.0), g_verts = dbl(T.verts.size(), 0.0);
        rc = dss_sdf2d_contacts_backward_grids(P, cap, kind.data(), pose.data(), prm.data(), scale.data(), gid.data(), &G, count.data(), tag.data(),
                                               tpar.data(), gout.data(), g_pose.data(), g_prm.data(), g_scale.data(), g_vals.data(),
                                               g_grads.data(), g_verts.data(), nullptr);
        ++launches;
        if (rc != 0 || g_pose.back() != GUARD || g_prm.back() != GUARD || g_scale.back() != GUARD || g_vals.back() != GUARD ||
            g_grads.back() != GUARD || g_verts.back() != GUARD) { printf("backward_grids status %d or a guard word written\n", rc); return 1; }
        std::vector<double> o_pose = dbl(6 * (size_t)P, 3.0), o_prm = dbl(4 * (size_t)P, 3.0), o_scale = dbl(2 * (size_t)P, 3.0);
        rc = dss_sdf2d_contacts_backward(P, cap, kind.data(), pose.data(), prm.data(), scale.data(), gid.data(), &G, count.data(), tag.data(),
                                         tpar.data(), gout.data(), o_pose.data(), o_prm.data(), o_scale.data(), nullptr);
        if (rc != 0 || std::memcmp(o_pose.data(), g_pose.data(), o_pose.size() * 8) || std::memcmp(o_prm.data(), g_prm.data(), o_prm.size() * 8) ||
            std::memcmp(o_scale.data(), g_scale.data(), o_scale.size() * 8)) { printf("pose gradients differ from the old entry's bits\n"); return 1; }
        std::vector<double> *now[3] = {&g_vals, &g_grads, &g_verts};
        for (int a = 0; a < 3; ++a) {
            for (double v : *now[a]) if (v != v) { printf("a table gradient is not a number\n"); return 1; }
            if (call == 0) keep[a] = *now[a];
            else if (!shared && std::memcmp(keep[a].data(), now[a]->data(), keep[a].size() * 8)) { printf("two calls differ in their bits (array %d)\n", a); return 1; }
            else if (shared)
                for (size_t k = 0; k < keep[a].size(); ++k)
                    if (std::fabs(keep[a][k] - (*now[a])[k]) > 1e-12 * (1.0 + std::fabs(keep[a][k]))) { printf("two calls differ beyond round-off\n"); return 1; }
        }
    }
    if (table_grad) { table_grad->clear(); for (int a = 0; a < 3; ++a) table_grad->insert(table_grad->end(), keep[a].begin(), keep[a].end() - 1); }
    for (int a = 0; a < 3; ++a)
        for (size_t k = 0; k + 1 < keep[a].size(); ++k) entries += keep[a][k] != 0.0;
    return 0;
}

static bool all_zero(const std::vector<double> &v) { for (double x : v) if (x != 0.0) return false; return true; }

int main()
{
    const Side floor_b{1, 0.0, 0.3, 4.95, 12.0, 4.0, 18.0, 0}, floor_far{1, 0.0, 0.3, 9.0, 12.0, 4.0, 18.0, 0};
    auto grid = [](double rot, double x, double y, int g) { return Side{3, rot, x, y, 0.0, 0.0, 10.0, g}; };
    std::vector<int> n, st;
    std::vector<double> tg;
    {   // 2 x 2: the slab's edge crosses the grid's box, where the query has no gradient
        Table T; T.add_corner();
        if (launch({{grid(0.0, 0.0, 0.0, 0), floor_b}}, T, 8, false, n, st, &tg)) return 1;
        if (n[0] != 0 || st[0] != 0 || !all_zero(tg)) { printf("2 x 2: count %d status %d\n", n[0], st[0]); return 1; }
    }
    {   // 3 x 3 and 5 x 9, the grid as body 1 and as body 2
        for (int shape = 0; shape < 2; ++shape) {
            Table T; if (shape) T.add_disc(5, 9, 24); else T.add_disc(3, 3, 12);
            if (launch({{grid(0.2, 0.0, 0.0, 0), floor_b}, {floor_b, grid(1.3, 0.1, 0.0, 0)}}, T, 16, true, n, st, &tg)) return 1;
            if (n[0] < 1 || n[1] < 1 || all_zero(tg)) { printf("shape %d: counts %d %d\n", shape, n[0], n[1]); return 1; }
        }
    }
    {   // two grids; no grid in two pairs
        Table T; T.add_disc(5, 9, 24); T.add_disc(17, 17, 76);
        if (launch({{grid(0.2, 0.0, 0.0, 1), floor_b}, {floor_b, grid(1.3, 0.1, 0.0, 0)}}, T, 16, false, n, st, &tg)) return 1;
        if (n[0] < 1 || n[1] < 1) { printf("two grids: counts %d %d\n", n[0], n[1]); return 1; }
        // both in one pair, and the second grid against itself
        if (launch({{grid(0.4, 0.0, 0.0, 1), grid(1.1, 5.7, 0.3, 0)}, {grid(0.4, 0.0, 10.0, 1), grid(1.1, 5.7, 10.3, 1)}}, T, 32, true, n, st, &tg)) return 1;
        if (n[0] < 1 || n[1] < 1) { printf("grid pairs: counts %d %d\n", n[0], n[1]); return 1; }
        const size_t nv0 = 45, nv1 = 289;
        bool first = false, second = false;
        for (size_t k = 0; k < nv0; ++k) first |= tg[k] != 0.0;
        for (size_t k = nv0; k < nv0 + nv1; ++k) second |= tg[k] != 0.0;
        if (!first || !second) { printf("a grid of the pair got no gradient on its samples\n"); return 1; }
    }
    {   // one grid shared by three pairs, a pair with count 0 beside them: the sum of the three pairs run alone, to round-off
        Table T; T.add_disc(17, 17, 76);
        const std::vector<Pair> three = {{grid(0.2, 0.0, 0.0, 0), floor_b}, {floor_b, grid(0.25, 0.0, 0.0, 0)}, {grid(0.3, 0.0, 0.0, 0), floor_b}};
        const Pair apart = {grid(0.2, 0.0, 0.0, 0), floor_far};
        std::vector<Pair> four = three;
        four.push_back(apart);
        if (launch(four, T, 16, true, n, st, &tg)) return 1;
        if (n[0] < 1 || n[1] < 1 || n[2] < 1 || n[3] != 0 || all_zero(tg)) { printf("shared grid: counts %d %d %d %d\n", n[0], n[1], n[2], n[3]); return 1; }
        std::vector<double> sum(tg.size(), 0.0), one;
        std::vector<int> n1, s1;
        for (int k = 0; k < 3; ++k) {
            if (launch({three[k]}, T, 16, false, n1, s1, &one)) return 1;
            if (n1[0] != n[k] || one.size() != sum.size()) { printf("pair %d alone: count %d, %d in the launch of four\n", k, n1[0], n[k]); return 1; }
            for (size_t e = 0; e < sum.size(); ++e) sum[e] += one[e];
        }
        double top = 0.0;
        for (double v : tg) top = std::fmax(top, std::fabs(v));
        for (size_t e = 0; e < sum.size(); ++e)
            if (std::fabs(sum[e] - tg[e]) > 1e-12 * top) { printf("shared grid: entry %zu is %g, the pairs alone sum to %g\n", e, tg[e], sum[e]); return 1; }
        // a pair flagged over cap contributes nothing: pair 0 needs more than one row
        std::vector<double> flagged;
        if (n[0] < 2) { printf("pair 0 has %d contacts, the cap seam needs two\n", n[0]); return 1; }
        if (launch({three[0], apart}, T, n[0] - 1, false, n1, s1, &flagged)) return 1;
        if (s1[0] != DSS_SDF2D_OVER_CAP || n1[0] != n[0] || !all_zero(flagged)) { printf("over cap: status %d count %d\n", s1[0], n1[0]); return 1; }
    }
    {   // a null output with a grid in the table
        Table T; T.add_disc(3, 3, 12);
        const DssSdf2dGrids G = T.c();
        int kind[2] = {3, 1}, gid[2] = {0, 0}, cnt[1] = {0}, tag[2] = {0, 0};
        double pose[6] = {0, 0, 0, 0, 0, 5}, prm[4] = {0, 0, 4, 4}, scale[2] = {10, 6}, z[64] = {0};
        for (int k = 0; k < 3; ++k) {
            double *t[3] = {z, z, z};
            t[k] = nullptr;
            if (dss_sdf2d_contacts_backward_grids(1, 1, kind, pose, prm, scale, gid, &G, cnt, tag, z, z, z, z, z, t[0], t[1], t[2], nullptr) != DSS_E_BADARG) {
                printf("a null table output was accepted\n");
                return 1;
            }
        }
        // (without a table the three outputs may be null: a grid body is then a malformed pair and contributes nothing)
        if (dss_sdf2d_contacts_backward_grids(1, 1, kind, pose, prm, scale, gid, nullptr, cnt, tag, z, z, z, z, z, nullptr, nullptr, nullptr, nullptr) != DSS_OK) {
            printf("null table outputs without a table were refused\n");
            return 1;
        }
    }
    printf("%ld launches %ld table entries with a gradient\n", launches, entries);
    return 0;
}
