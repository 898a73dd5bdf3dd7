// Test harness (CPU, test infrastructure): csrc/sdf2d_contacts.hip through the fiber emulator as a program of its own, so that it
// can be built with the address and undefined-behaviour sanitizers.  Every output array is a heap block of exactly the size the
// ABI asks for plus one guard word that must come back untouched (a write further out ends the run under the sanitizer).
// Walked: outlines of 4, 64, 76 and 150 edges (rect, circle and bowl, two grid discs whose outlines are regular polygons over
// disc samples); `cap` at, one below and one above the number of contacts a launch needs, with a pair that fits beside the one
// that does not; cand_cap at 0, below and above the number of contacts before thinning; two 150-edge outlines on top of each
// other under a wide eps (more than DSS_SDF2D_MAXCAND contacts before thinning); the backward pass after each forward.
// Prints "<launches> launches <contacts> contacts most <n> per pair"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../diffsdfsim_amd/csrc/sdf2d_contacts.hip"

static const double GUARD = -7.25;
static const int IGUARD = -77;
static long launches = 0, contacts = 0;
static int most = 0;

struct Table {
    std::vector<int> dims, val_off, vert_off{0}, edge_off{0}, edges;
    std::vector<double> vals, grads, verts;
    // a disc of radius 0.3 sampled n x n over [-0.5, 0.5]^2, its outline a regular polygon of ne edges
    void add_disc(int n, int ne)
    {
        dims.push_back(n); dims.push_back(n);
        val_off.push_back((int)vals.size());
        const size_t base = vals.size();
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double x = -0.5 + (double)i / (n - 1), y = -0.5 + (double)j / (n - 1);
                vals.push_back(std::sqrt(x * x + y * y) - 0.3);
            }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                grads.push_back(i == 0 || i == n - 1 ? 0.0 : (vals[base + (size_t)(i + 1) * n + j] - vals[base + (size_t)(i - 1) * n + j]) / 2.0);
                grads.push_back(j == 0 || j == n - 1 ? 0.0 : (vals[base + (size_t)i * n + j + 1] - vals[base + (size_t)i * n + j - 1]) / 2.0);
            }
        for (int k = 0; k < ne; ++k) {
            verts.push_back(0.3 * std::cos(2.0 * M_PI * k / ne)); verts.push_back(0.3 * std::sin(2.0 * M_PI * k / ne));
            edges.push_back(k); edges.push_back((k + 1) % ne);
        }
        vert_off.push_back(vert_off.back() + ne); edge_off.push_back(edge_off.back() + ne);
    }
    DssSdf2dGrids c() const
    {
        return DssSdf2dGrids{(int)dims.size() / 2, dims.data(), val_off.data(), vert_off.data(), edge_off.data(), edges.data(), vals.data(),
                             grads.data(), verts.data()};
    }
};

struct Side { int kind; double rot, x, y, p0, p1, scale; int grid; };
struct Pair { Side a, b; };
struct Result { std::vector<int> count, status, ncand; };

static std::vector<double> dbl(size_t n) { std::vector<double> v(n + 1, GUARD); return v; }
static std::vector<int> ints(size_t n) { std::vector<int> v(n + 1, IGUARD); return v; }

// one forward launch and the backward after it; every buffer exact plus its guard word.  0: fine
static int launch(const std::vector<Pair> &pairs, const Table &T, double eps, int cap, int cand_cap, Result &R)
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
    std::vector<double> out = dbl((size_t)P * cap * 7), tpar = dbl((size_t)P * cap), cand = dbl((size_t)P * cand_cap * 7);
    std::vector<int> count = ints(P), status = ints(P), tag = ints((size_t)P * cap * 2), ncand = ints(P), ctag = ints((size_t)P * cand_cap * 2);
    int rc = dss_sdf2d_contacts_forward(P, cap, kind.data(), pose.data(), prm.data(), scale.data(), gid.data(), &G, eps, out.data(), count.data(),
                                        status.data(), tag.data(), tpar.data(), cand_cap, cand_cap ? ncand.data() : nullptr,
                                        cand_cap ? cand.data() : nullptr, cand_cap ? ctag.data() : nullptr, nullptr);
    ++launches;
    if (rc != 0) { printf("forward status %d\n", rc); return 1; }
    if (out.back() != GUARD || tpar.back() != GUARD || cand.back() != GUARD || count.back() != IGUARD || status.back() != IGUARD ||
        tag.back() != IGUARD || ncand.back() != IGUARD || ctag.back() != IGUARD) { printf("a guard word was written (cap %d, cand_cap %d)\n", cap, cand_cap); return 1; }
    for (int p = 0; p < P; ++p) {
        const int n = status[p] ? 0 : count[p];
        if (n > cap) { printf("pair %d: count %d above cap %d without a status\n", p, n, cap); return 1; }
        for (int q = 0; q < cap; ++q) {
            const double *row = &out[((size_t)p * cap + q) * 7];
            const double nn = row[0] * row[0] + row[1] * row[1];
            if (q < n ? std::fabs(nn - 1.0) > 1e-12 || !(-row[6] <= eps) : nn != 0.0) { printf("pair %d row %d of %d: normal^2 %g pen %g\n", p, q, n, nn, row[6]); return 1; }
            const int d = tag[((size_t)p * cap + q) * 2], e = tag[((size_t)p * cap + q) * 2 + 1];
            if (d < 0 || d > 1 || e < 0 || tpar[(size_t)p * cap + q] < 0.0 || tpar[(size_t)p * cap + q] > 1.0) { printf("pair %d row %d: tag %d %d\n", p, q, d, e); return 1; }
        }
        if (cand_cap && !status[p] && ncand[p] < n) { printf("pair %d: %d contacts of %d before thinning\n", p, n, ncand[p]); return 1; }
        contacts += n;
        if (n > most) most = n;
    }
    std::vector<double> gout((size_t)P * cap * 7, 0.5), g_pose = dbl(6 * (size_t)P), g_prm = dbl(4 * (size_t)P), g_scale = dbl(2 * (size_t)P);
    rc = dss_sdf2d_contacts_backward(P, cap, kind.data(), pose.data(), prm.data(), scale.data(), gid.data(), &G, count.data(), tag.data(), tpar.data(),
                                     gout.data(), g_pose.data(), g_prm.data(), g_scale.data(), nullptr);
    ++launches;
    if (rc != 0 || g_pose.back() != GUARD || g_prm.back() != GUARD || g_scale.back() != GUARD) { printf("backward status %d or a guard word written\n", rc); return 1; }
    for (int p = 0; p < P; ++p) {
        double any = 0.0;
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) {
                const double v = g_pose[3 * ((size_t)s * P + p) + k];
                if (v == GUARD || v != v) { printf("pair %d: pose gradient not written or not a number\n", p); return 1; }
                any += std::fabs(v);
            }
        if ((status[p] == 0 && count[p] > 0) != (any > 0.0)) { printf("pair %d: %d contacts, status %d, |gradient| %g\n", p, count[p], status[p], any); return 1; }
    }
    R.count.assign(count.begin(), count.end() - 1); R.status.assign(status.begin(), status.end() - 1); R.ncand.assign(ncand.begin(), ncand.end() - 1);
    return 0;
}

int main()
{
    Table T;
    T.add_disc(33, 76);
    T.add_disc(65, 150);
    const Side rect_a{1, 0.0, 0.0, 0.0, 4.0, 2.0, 6.0, 0}, floor_a{1, 0.0, 0.5, 3.0, 6.0, 4.0, 9.0, 0};
    const Side ball{0, 0.3, 0.013, 1.47, 2.55, 0.0, 2.55 * 2 * 1.3333, 0}, bowl{2, 0.0, 0.0, 0.0, 3.0, 0.4, 3.4 * 2 * 1.3333, 0};
    const Side circ_a{0, 0.1, 0.0, 0.0, 1.5, 0.0, 1.5 * 2 * 1.3333, 0}, circ_b{0, 0.7, 2.95, 0.2, 1.5, 0.0, 1.5 * 2 * 1.3333, 0};
    const Side disc{3, 0.2, 0.0, 0.0, 0.0, 0.0, 10.0, 0}, floor_b{1, 0.0, 0.3, 4.95, 12.0, 4.0, 18.0, 0};
    const Side big1{3, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0, 1}, big2{3, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0, 1};
    const std::vector<Pair> pairs = {{rect_a, floor_a}, {ball, bowl}, {circ_a, circ_b}, {disc, floor_b}, {bowl, disc}};
    Result R;
    if (launch(pairs, T, 0.1, 64, 200, R)) return 1;
    int need = 0, hold = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (R.status[p] != 0) { printf("pair %zu: status %d under a roomy cap\n", p, R.status[p]); return 1; }
        if (R.count[p] > need) need = R.count[p];
        if (R.ncand[p] > hold) hold = R.ncand[p];
    }
    if (R.count[0] != 2 || R.count[1] < 17 || R.count[2] < 1 || R.count[3] < 1) { printf("counts %d %d %d %d\n", R.count[0], R.count[1], R.count[2], R.count[3]); return 1; }
    const std::vector<int> roomy = R.count;
    for (int cap : {need, need + 1, need - 1, 1})
        for (int cand_cap : {0, hold - 1, hold, hold + 1}) {
            if (launch(pairs, T, 0.1, cap, cand_cap, R)) return 1;
            for (size_t p = 0; p < pairs.size(); ++p) {
                const bool over = roomy[p] > cap;
                if (R.status[p] != (over ? DSS_SDF2D_OVER_CAP : 0) || R.count[p] != roomy[p]) {
                    printf("cap %d pair %zu: status %d count %d, want %d contacts\n", cap, p, R.status[p], R.count[p], roomy[p]);
                    return 1;
                }
            }
        }
    // more contacts before thinning than the kernel holds, beside a pair that fits
    if (launch({{big1, big2}, {rect_a, floor_a}}, T, 0.5, 8, 4, R)) return 1;
    if (R.status[0] != DSS_SDF2D_OVER_CAND || R.count[0] != 0 || R.status[1] != 0 || R.count[1] != 2) {
        printf("candidate bound: status %d %d count %d %d\n", R.status[0], R.status[1], R.count[0], R.count[1]);
        return 1;
    }
    // an unknown kind, a grid outside the table
    Side odd = rect_a, lost = disc;
    odd.kind = 9; lost.grid = 5;
    if (launch({{odd, floor_a}, {rect_a, floor_a}, {lost, floor_b}}, T, 0.1, 4, 2, R)) return 1;
    if (R.status[0] != DSS_SDF2D_MALFORMED || R.status[1] != 0 || R.status[2] != DSS_SDF2D_MALFORMED || R.count[1] != 2) { printf("malformed pairs\n"); return 1; }
    printf("%ld launches %ld contacts most %d per pair\n", launches, contacts, most);
    return 0;
}
