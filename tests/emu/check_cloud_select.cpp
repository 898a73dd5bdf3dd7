// Test harness (CPU, test infrastructure): csrc/cloud_select.hip through the fiber emulator as a program of its own, so that it
// can be built with the address and undefined-behaviour sanitizers: every array is a heap block of exactly the size the ABI
// asks for, and a read or a write outside one ends the run.  The select cases are the shapes and kinds of
// tests/cloud_select_ref.py (drawn here by a generator of this file), checked against a plain loop over the pixels; the
// statistics run on segments of 0, 1, 63, 64, 65 and 2 049 points against long double sums (count, min, max exact; a sum within
// n 2^-52 sum|x|, the bound for any order of n terms).
// Prints "<select cases> select <segments> segments worst <error / bound>"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../../diffsdfsim_amd/csrc/cloud_select.hip"

static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (state >> 11) / 9007199254740992.0; }

static int run_select(int W, int H, int kind)
{
    const int nframe = 3, label = 4;
    const size_t npx = (size_t)nframe * H * W;
    std::vector<double> pcs(3 * npx);
    std::vector<int> segs(npx);
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    for (size_t i = 0; i < npx; ++i) {
        for (int k = 0; k < 3; ++k) pcs[3 * i + k] = 6.0 * rnd() - 3.0;
        const int frame = (int)(i / ((size_t)H * W));
        segs[i] = kind == 2 ? label : (rnd() < 0.4 ? label : (int)(7.0 * rnd()) - 1);
        if (kind == 1 && segs[i] == label) segs[i] = 2;                       // the label occurs nowhere
        if (frame == 1 && segs[i] == label) segs[i] = 0;                      // the middle frame holds no pixel of it
        if (rnd() < 0.15 && !(kind == 2 && frame == 2)) pcs[3 * i + (int)(3.0 * rnd())] = bad[(int)(3.0 * rnd())];
    }
    std::vector<double> want;
    std::vector<int> want_rows((size_t)nframe * H, 0);
    for (size_t i = 0; i < npx; ++i)
        if (segs[i] == label && std::isfinite(pcs[3 * i]) && std::isfinite(pcs[3 * i + 1]) && std::isfinite(pcs[3 * i + 2])) {
            want.insert(want.end(), pcs.begin() + 3 * i, pcs.begin() + 3 * i + 3);
            ++want_rows[i / W];
        }
    std::vector<int> rows((size_t)nframe * H, -5), off((size_t)nframe * H);
    if (dss_cloud_select_count(nframe, H, W, label, pcs.data(), segs.data(), rows.data(), nullptr) != 0 || rows != want_rows) return 1;
    int n = 0;
    for (size_t r = 0; r < rows.size(); ++r) { off[r] = n; n += rows[r]; }
    if ((size_t)n * 3 != want.size() || (kind == 1) != (n == 0) || (kind == 2 && rows[2 * H] != W)) return 1;
    std::vector<double> pts(3 * (size_t)n, 7.5);
    if (dss_cloud_select_emit(nframe, H, W, label, pcs.data(), segs.data(), off.data(), n ? pts.data() : nullptr, nullptr) != 0) return 1;
    return pts == want ? 0 : 1;
}

int main()
{
    const int shapes[6][2] = {{1, 3}, {63, 2}, {64, 2}, {65, 3}, {130, 7}, {3, 1}};
    int ncase = 0;
    for (auto &s : shapes)
        for (int kind = 0; kind < 3; ++kind, ++ncase)
            if (run_select(s[0], s[1], kind)) { printf("select W %d H %d kind %d differs\n", s[0], s[1], kind); return 1; }

    const int lens[6] = {0, 1, 63, 64, 65, 2049}, nseg = 6;
    std::vector<int> off(nseg + 1, 0);
    int max_len = 0;
    for (int s = 0; s < nseg; ++s) { off[s + 1] = off[s] + lens[s]; if (lens[s] > max_len) max_len = lens[s]; }
    std::vector<double> pts(3 * (size_t)off[nseg]);
    for (size_t i = 0; i < pts.size(); ++i) pts[i] = (2.0 * rnd() - 1.0) * std::pow(10.0, (int)(7.0 * rnd()) - 3) + (i % 3 == 2 ? -1e3 : 0.0);
    const size_t nbytes = dss_cloud_stats_workspace_bytes(nseg, max_len);
    std::vector<double> ws(nbytes / sizeof(double)), out((size_t)nseg * 10, -7.0);
    if (dss_cloud_stats(nseg, max_len, off.data(), pts.data(), out.data(), ws.data(), nbytes, nullptr) != 0) { printf("stats: status\n"); return 1; }
    double worst = 0.0;
    for (int s = 0; s < nseg; ++s) {
        const double *o = &out[(size_t)s * 10];
        if (o[0] != lens[s]) { printf("segment %d: count %g\n", s, o[0]); return 1; }
        for (int k = 0; k < 3; ++k) {
            long double sum = 0, abs_sum = 0;
            double mn = std::numeric_limits<double>::infinity(), mx = -mn;
            for (int i = off[s]; i < off[s + 1]; ++i) {
                const double v = pts[3 * (size_t)i + k];
                sum += v; abs_sum += std::fabs(v);
                if (v < mn) mn = v;
                if (v > mx) mx = v;
            }
            if (o[4 + k] != mn || o[7 + k] != mx) { printf("segment %d axis %d: min %g max %g\n", s, k, o[4 + k], o[7 + k]); return 1; }
            const long double err = fabsl(o[1 + k] - sum), bound = lens[s] * 0x1p-52L * abs_sum;
            if (err > bound) { printf("segment %d axis %d: sum %.17g vs %.17Lg\n", s, k, o[1 + k], sum); return 1; }
            if (bound > 0 && (double)(err / bound) > worst) worst = (double)(err / bound);
        }
    }
    printf("%d select %d segments worst %.3f\n", ncase, nseg, worst);
    return 0;
}
