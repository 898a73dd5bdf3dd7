// Test harness (CPU, test infrastructure): csrc/chamfer.hip through the fiber emulator as a program of its own, so that it can be
// built with the address and undefined-behaviour sanitizers: every array is a heap block of exactly the size the ABI asks for, and
// a read or a write outside one ends the run.  The calls are those of tests/test_emu_chamfer.py (drawn here by a generator of this
// file): nine unequal segments across the wavefront, query-block and tile boundaries with an empty query segment, an empty
// reference segment and a one-point pair, on the direct and on the split path, at the origin and shifted by (1e3, -2e3, 5e2); five
// queries against 3 tiles + 1; the integer lattice on both paths.  Checked against a plain double loop over the pairs in the
// direct form: idx equal (the first minimum), d2 within 2^-48 relative, equal on the lattice.
// Prints "<calls> calls <queries> queries worst <error / bound>"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../../diffsdfsim_amd/csrc/chamfer.hip"

static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (state >> 11) / 9007199254740992.0; }

static double worst = 0.0;
static long nquery = 0;

// lens [nseg][2]: query and reference points per segment; lattice: integer coordinates in [-3, 3]; want_split: the path expected
static int run(const std::vector<std::pair<int, int>> &lens, bool shifted, bool lattice, bool want_split)
{
    const int nseg = (int)lens.size();
    std::vector<int> qo(nseg + 1, 0), ro(nseg + 1, 0);
    int max_q = 0, max_r = 0;
    for (int s = 0; s < nseg; ++s) {
        qo[s + 1] = qo[s] + lens[s].first; ro[s + 1] = ro[s] + lens[s].second;
        if (lens[s].first > max_q) max_q = lens[s].first;
        if (lens[s].second > max_r) max_r = lens[s].second;
    }
    const double shift[3] = {1e3, -2e3, 5e2};
    auto draw = [&](std::vector<double> &v) {
        for (size_t i = 0; i < v.size(); ++i) v[i] = lattice ? std::floor(7.0 * rnd()) - 3.0 : 2.0 * rnd() - 1.0 + (shifted ? shift[i % 3] : 0.0);
    };
    std::vector<double> q(3 * (size_t)qo[nseg]), r(3 * (size_t)ro[nseg]);
    draw(q); draw(r);
    const size_t nbytes = dss_chamfer_nn_workspace_bytes(nseg, max_q, max_r);
    if ((nbytes > 0) != want_split) { printf("path: workspace %zu bytes\n", nbytes); return 1; }
    std::vector<char> ws(nbytes);
    std::vector<double> d2(qo[nseg], -7.0);
    std::vector<int> idx(qo[nseg], -7);
    if (dss_chamfer_nn(nseg, max_q, max_r, qo.data(), q.data(), ro.data(), r.data(), d2.data(), idx.data(), nbytes ? ws.data() : nullptr, nbytes,
                       nullptr) != 0) { printf("status\n"); return 1; }
    for (int s = 0; s < nseg; ++s)
        for (int i = qo[s]; i < qo[s + 1]; ++i, ++nquery) {
            double best = std::numeric_limits<double>::infinity();
            int at = -1;
            for (int j = ro[s]; j < ro[s + 1]; ++j) {
                const double dx = q[3 * (size_t)i] - r[3 * (size_t)j], dy = q[3 * (size_t)i + 1] - r[3 * (size_t)j + 1], dz = q[3 * (size_t)i + 2] - r[3 * (size_t)j + 2];
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < best) { best = d; at = j; }
            }
            const double err = std::isinf(best) ? (d2[i] == best ? 0.0 : 1.0) : std::fabs(d2[i] - best), bound = lattice ? 0.0 : 0x1p-48 * best;
            if (idx[i] != at || err > bound) { printf("segment %d query %d: d2 %.17g idx %d, want %.17g %d\n", s, i, d2[i], idx[i], best, at); return 1; }
            if (bound > 0 && err / bound > worst) worst = err / bound;
        }
    return 0;
}

int main()
{
    const int Q = DSS_CHAMFER_QUERIES, T = DSS_CHAMFER_TILE;
    const std::vector<std::pair<int, int>> direct = {{1, 65}, {63, T - 1}, {64, T}, {0, 64}, {1, 1}, {65, 0}, {Q - 1, T + 1}, {Q, 2 * T}, {Q + 1, 63}};
    std::vector<std::pair<int, int>> split = direct;
    split[2].second = 3 * T + 1; split[7].second = 2 * T + 3;
    int ncall = 0;
    for (int shifted = 0; shifted < 2; ++shifted) {
        if (run(direct, shifted, false, false)) return 1;
        if (run(split, shifted, false, true)) return 1;
        ncall += 2;
    }
    if (run({{5, 3 * T + 1}}, false, false, true)) return 1;
    if (run({{Q + 65, 2 * T}}, false, true, false)) return 1;
    if (run({{Q + 65, 5 * T + 1}}, false, true, true)) return 1;
    ncall += 3;
    printf("%d calls %ld queries worst %.3f\n", ncall, nquery, worst);
    return 0;
}
