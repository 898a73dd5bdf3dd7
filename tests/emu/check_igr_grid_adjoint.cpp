// Test harness (CPU, test infrastructure): csrc/igr_grid_adjoint.hip, with csrc/igr_mlp.hip behind it, through the fiber emulator as
// a program of its own, so that it can be built with the address and undefined-behaviour sanitizers: every array is a heap block of
// exactly the size the ABI asks for -- g_latent of nlat * 4 doubles, n_nodes of one int, the workspace of exactly
// dss_igr_grid_adjoint_workspace_bytes -- and a read or a write outside one ends the run.  The seams of
// tests/test_emu_igr_grid_adjoint.py part 2:
//   grids of 5^3 (under one chunk), 13^3 (one chunk and a ragged one) and (3, 4, 17) samples; no node, one node, every node (5^3),
//   3, 4 and 5 nodes (the network's tangent tile is 4 points) on both sides of the 13^3 grid's chunk boundary;
//   two grids sharing a latent row, a grid with lat_idx -1 whose adjoint is all NaN, a NaN code that nobody names;
//   the capacity at the need and one below (DSS_E_WORKSPACE, n_nodes right, g_latent untouched); two calls bit-equal; refused inputs.
// (The emulated network under the sanitizers takes a fifth of a second per point: the lists are short.)
// Checked: the return code, n_nodes against the host's own count, the named rows finite and not the sentinel, exact zeros in the
// slots >= L and in the rows nobody names.  Prints "<calls> calls <nodes> compacted"; exit code 1 on any mismatch.
#ifndef DSS_EMU
#define DSS_EMU 1
#endif
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../../diffsdfsim_amd/csrc/igr_mlp.hip"
#include "../../diffsdfsim_amd/csrc/igr_grid_adjoint.hip"

static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (state >> 11) / 9007199254740992.0; }

static long compacted = 0;
static int ncall = 0;
static const double SENT = -7.25, QNAN = std::numeric_limits<double>::quiet_NaN();

struct Grid { int n[3]; int row; std::vector<double> g; };

static Grid make(int n0, int n1, int n2, int row, const std::vector<int> &idx, bool all = false, bool nan = false)
{
    Grid G{{n0, n1, n2}, row, std::vector<double>((size_t)n0 * n1 * n2, nan ? QNAN : 0.0)};
    if (all) for (double &v : G.g) v = 2.0 * rnd() - 1.0 + 1e-3;
    for (int i : idx) G.g[i] = 0.5 + rnd();
    return G;
}

// -> 0 when the call returned `want_rc` and left what it should; out (if given) receives g_latent
static int run(const std::vector<Grid> &grids, const DssIgrNet &net, const std::vector<double> &latents, int stride, int nlat, int cap, int want_rc,
               std::vector<double> *keep = nullptr)
{
    const int ngrid = (int)grids.size();
    std::vector<int> off(ngrid), dims(3 * (size_t)ngrid), rows(ngrid);
    std::vector<double> g;
    std::vector<char> named(nlat, 0);
    int need = 0;
    for (int k = 0; k < ngrid; ++k) {
        off[k] = (int)g.size();
        for (int d = 0; d < 3; ++d) dims[3 * k + d] = grids[k].n[d];
        rows[k] = grids[k].row;
        g.insert(g.end(), grids[k].g.begin(), grids[k].g.end());
        if (rows[k] < 0) continue;
        int live = 0;
        for (double v : grids[k].g) live += !(v == 0.0);
        if (live) named[rows[k]] = 1;
        need += live;
    }
    if (cap < 0) cap = need > 0 ? need : 1;
    const size_t nbytes = dss_igr_grid_adjoint_workspace_bytes((int)g.size(), cap, nlat);
    std::vector<char> ws(nbytes);
    std::vector<double> out((size_t)nlat * DSS_IGR_LATENT_MAX, SENT);
    std::vector<int> nn(1, -77);
    const int rc = dss_igr_grid_adjoint(&net, ngrid, off.data(), dims.data(), rows.data(), latents.data(), stride, nlat, g.data(), cap, out.data(),
                                        nn.data(), ws.data(), nbytes, nullptr);
    ++ncall;
    if (rc != want_rc) { printf("call %d: status %d, want %d\n", ncall, rc, want_rc); return 1; }
    if (rc == DSS_E_WORKSPACE) {
        if (nn[0] != need) { printf("call %d: n_nodes %d, want %d\n", ncall, nn[0], need); return 1; }
        for (double v : out) if (v != SENT) { printf("call %d: g_latent written on a refusal\n", ncall); return 1; }
        return 0;
    }
    if (nn[0] != need) { printf("call %d: n_nodes %d, want %d\n", ncall, nn[0], need); return 1; }
    const int L = net.latent;
    for (int r = 0; r < nlat; ++r)
        for (int k = 0; k < DSS_IGR_LATENT_MAX; ++k) {
            const double v = out[(size_t)r * DSS_IGR_LATENT_MAX + k];
            const bool zero = k >= L || !named[r];
            if (zero ? v != 0.0 : (!std::isfinite(v) || v == SENT || v == 0.0)) { printf("call %d: row %d slot %d: %.17g\n", ncall, r, k, v); return 1; }
        }
    compacted += need;
    if (keep) *keep = out;
    return 0;
}

int main()
{
    // the 128-wide network with two latent numbers: any finite weights serve (the values are the subject of the Python tests)
    const int H = 128, DIN = 5;
    std::vector<double> W0(H * DIN), b0(H), Wp(dss_igr_packed_doubles()), bh(7 * H), W8(H), b8(1, -0.5);
    for (double &v : W0) v = 0.6 * rnd() - 0.3;
    for (double &v : b0) v = 0.02 * rnd() - 0.01;
    for (double &v : Wp) v = 0.3 * rnd() - 0.15;
    for (double &v : bh) v = 0.02 * rnd() - 0.01;
    for (double &v : W8) v = 0.3 * rnd();
    const DssIgrNet net{W0.data(), b0.data(), Wp.data(), bh.data(), W8.data(), b8.data(), H, 2};
    const int stride = 3, nlat = 3;
    const std::vector<double> latents = {0.05, -0.1, QNAN, QNAN, QNAN, QNAN, -0.08, 0.02, QNAN};      // row 1: a NaN code nobody names

    if (run({make(5, 5, 5, 0, {})}, net, latents, stride, nlat, -1, DSS_OK)) return 1;                        // no node
    if (run({make(5, 5, 5, 2, {124})}, net, latents, stride, nlat, -1, DSS_OK)) return 1;                     // one node, the grid's last
    if (run({make(3, 4, 17, 0, {0, 203})}, net, latents, stride, nlat, -1, DSS_OK)) return 1;
    if (run({make(5, 5, 5, 0, {}, true)}, net, latents, stride, nlat, -1, DSS_OK)) return 1;                  // every node
    const std::vector<int> seam = {2196, 2047, 2048, 0, 2049};
    for (int n = 3; n <= 5; ++n)                                                                                // the tile and one off, both chunks
        if (run({make(13, 13, 13, 0, std::vector<int>(seam.begin(), seam.begin() + n))}, net, latents, stride, nlat, -1, DSS_OK)) return 1;
    // shared rows, a grid that is not a neural one with an all-NaN adjoint, twice: the same bits
    const std::vector<Grid> combo = {make(5, 5, 5, 0, {3, 77}), make(3, 4, 17, -1, {}, false, true), make(13, 13, 13, 0, {5, 2047, 2048}),
                                     make(5, 5, 5, 2, {0, 62})};
    std::vector<double> a, b;
    if (run(combo, net, latents, stride, nlat, -1, DSS_OK, &a) || run(combo, net, latents, stride, nlat, 64, DSS_OK, &b)) return 1;
    if (memcmp(a.data(), b.data(), a.size() * sizeof(double)) != 0) { printf("two calls differ\n"); return 1; }
    // the capacity one below the need
    if (run(combo, net, latents, stride, nlat, 6, DSS_E_WORKSPACE)) return 1;
    // refused inputs: a dim of 1, a latent row past the table, a stride below L, a network shape that is not built
    std::vector<Grid> bad = combo;
    bad[2].n[1] = 1; bad[2].g.resize(13 * 13);
    DssIgrNet odd = net;
    odd.width = 192;
    std::vector<Grid> far = combo;
    far[3].row = 3;
    // (a refusal returns before anything is compared: run() checks the status and that nothing was written)
    struct { const std::vector<Grid> *g; const DssIgrNet *n; int stride, want; } refusals[] = {
        {&bad, &net, stride, DSS_E_BADARG}, {&far, &net, stride, DSS_E_BADARG}, {&combo, &net, 1, DSS_E_BADARG}, {&combo, &odd, stride, DSS_E_UNSUPPORTED}};
    for (auto &r : refusals) {
        const int ngrid = (int)r.g->size();
        std::vector<int> off(ngrid), dims(3 * (size_t)ngrid), rows(ngrid);
        std::vector<double> g;
        for (int k = 0; k < ngrid; ++k) {
            off[k] = (int)g.size();
            for (int d = 0; d < 3; ++d) dims[3 * k + d] = (*r.g)[k].n[d];
            rows[k] = (*r.g)[k].row;
            g.insert(g.end(), (*r.g)[k].g.begin(), (*r.g)[k].g.end());
        }
        const size_t nbytes = dss_igr_grid_adjoint_workspace_bytes((int)g.size(), 16, nlat);
        std::vector<char> ws(nbytes, 0x5a);
        std::vector<double> out((size_t)nlat * DSS_IGR_LATENT_MAX, SENT);
        std::vector<int> nn(1, -77);
        const int rc = dss_igr_grid_adjoint(r.n, ngrid, off.data(), dims.data(), rows.data(), latents.data(), r.stride, nlat, g.data(), 16, out.data(),
                                            nn.data(), ws.data(), nbytes, nullptr);
        ++ncall;
        bool clean = rc == r.want && nn[0] == -77;
        for (double v : out) clean = clean && v == SENT;
        for (char c : ws) clean = clean && c == 0x5a;
        if (!clean) { printf("call %d: a refusal returned %d (want %d) or wrote something\n", ncall, rc, r.want); return 1; }
    }
    printf("%d calls %ld compacted\n", ncall, compacted);
    return 0;
}
