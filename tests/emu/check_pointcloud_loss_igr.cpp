// Test harness (CPU, test infrastructure): csrc/pointcloud_loss_igr.hip, with csrc/igr_mlp.hip behind it, through the fiber emulator
// as a program of its own, so that it can be built with the address and undefined-behaviour sanitizers: every array is a heap block
// of exactly the size the ABI asks for -- the workspace of exactly dss_pointcloud_loss_igr_workspace_bytes -- and a read or a write
// outside one ends the run.  The compaction offsets are where an overrun would hide, so the calls are shaped around them:
//   1  three segments: 4133 points (three chunks, 7 + 6 + 5 inside: non-zero chunk offsets, a count that is no multiple of 16),
//      an empty segment, and 300 points of which every thirtieth is inside, with another latent row
//      (few points inside: the emulated network under the sanitizers takes a fifth of a second per point)
//   2  the same points with every pose moved away: nothing inside, the network walks a list of length 0
//   3  one segment of 20 points, all inside: the list fills its capacity to the last slot
// Checked: the return code, every count against the host's own inside test, the other outputs finite and the sentinel gone.
// Prints "<calls> calls <points> compacted"; exit code 1 on any mismatch.
#ifndef DSS_EMU
#define DSS_EMU 1
#endif
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../diffsdfsim_amd/csrc/igr_mlp.hip"
#include "../../diffsdfsim_amd/csrc/pointcloud_loss_igr.hip"

static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (state >> 11) / 9007199254740992.0; }

static long compacted = 0;

struct Seg { int n; std::vector<char> inside; double scale; int row; };

static int run(const std::vector<Seg> &segs, bool away, const DssIgrNet &net, const std::vector<double> &latents, int stride)
{
    const int nseg = (int)segs.size();
    std::vector<int> off(nseg + 1, 0), rows(nseg);
    std::vector<double> pose(7 * (size_t)nseg), scale(nseg);
    int max_len = 0;
    for (int s = 0; s < nseg; ++s) {
        off[s + 1] = off[s] + segs[s].n;
        if (segs[s].n > max_len) max_len = segs[s].n;
        rows[s] = segs[s].row; scale[s] = segs[s].scale;
        double *p = &pose[7 * (size_t)s];
        for (int i = 0; i < 4; ++i) p[i] = 2.0 * rnd() - 1.0;      // (a raw quaternion, not normalised)
        for (int i = 0; i < 3; ++i) p[4 + i] = 4.0 * rnd() - 2.0;
    }
    const int n_pts = off[nseg];
    std::vector<double> pts(3 * (size_t)n_pts);
    std::vector<int> want(nseg, 0);
    for (int s = 0; s < nseg; ++s) {
        double R[9];
        dss::quat_to_mat(&pose[7 * (size_t)s], R);
        for (int i = 0; i < segs[s].n; ++i) {
            double p[3];
            for (int k = 0; k < 3; ++k) p[k] = (1.9 * rnd() - 0.95) * scale[s];
            if (!segs[s].inside[i]) p[(int)(3.0 * rnd())] = (rnd() < 0.5 ? -1.0 : 1.0) * scale[s] * (1.05 + rnd());
            else ++want[s];
            for (int k = 0; k < 3; ++k)
                pts[3 * (size_t)(off[s] + i) + k] = R[3 * k] * p[0] + R[3 * k + 1] * p[1] + R[3 * k + 2] * p[2] + pose[7 * (size_t)s + 4 + k];
        }
        if (away) { pose[7 * (size_t)s + 4] += 50.0; want[s] = 0; }
    }
    const size_t nbytes = dss_pointcloud_loss_igr_workspace_bytes(nseg, max_len, n_pts);
    std::vector<char> ws(nbytes);
    std::vector<double> out((size_t)nseg * DSS_PC_IGR_OUT, -7.25);
    const int rc = dss_pointcloud_loss_igr(&net, nseg, max_len, off.data(), pts.data(), pose.data(), scale.data(), rows.data(), latents.data(),
                                           stride, n_pts, out.data(), nbytes ? ws.data() : nullptr, nbytes, nullptr);
    if (rc != 0) { printf("status %d\n", rc); return 1; }
    for (int s = 0; s < nseg; ++s) {
        const double *o = &out[(size_t)s * DSS_PC_IGR_OUT];
        if (o[1] != (double)want[s]) { printf("segment %d: count %.17g, want %d\n", s, o[1], want[s]); return 1; }
        for (int k = 0; k < DSS_PC_IGR_OUT; ++k)
            if (!std::isfinite(o[k]) || o[k] == -7.25 || (want[s] == 0 && o[k] != 0.0) || (k >= 11 && o[k] != 0.0)) {
                printf("segment %d output %d: %.17g\n", s, k, o[k]);
                return 1;
            }
        if (want[s] > 0 && !(o[0] > 0.0)) { printf("segment %d: sum %.17g\n", s, o[0]); return 1; }
        compacted += want[s];
    }
    return 0;
}

int main()
{
    // the 128-wide network with two latent numbers: any finite weights serve (the values are the subject of the golden tests)
    const int H = 128, DIN = 5;
    std::vector<double> W0(H * DIN), b0(H), Wp(dss_igr_packed_doubles()), bh(7 * H), W8(H), b8(1, -0.5);
    for (double &v : W0) v = 0.6 * rnd() - 0.3;
    for (double &v : b0) v = 0.02 * rnd() - 0.01;
    for (double &v : Wp) v = 0.3 * rnd() - 0.15;
    for (double &v : bh) v = 0.02 * rnd() - 0.01;
    for (double &v : W8) v = 0.3 * rnd();
    const DssIgrNet net{W0.data(), b0.data(), Wp.data(), bh.data(), W8.data(), b8.data(), H, 2};
    const int stride = 3;
    std::vector<double> latents = {0.05, -0.1, 1e300, -0.08, 0.02, 1e300};

    Seg sparse{4096 + 37, std::vector<char>(4096 + 37, 0), 1.2, 0};
    const int lo[3] = {0, 2048, 4096}, len[3] = {2048, 2048, 37}, k[3] = {7, 6, 5};
    for (int c = 0; c < 3; ++c)
        for (int placed = 0; placed < k[c];) {
            const int i = lo[c] + (int)(len[c] * rnd());
            if (!sparse.inside[i]) { sparse.inside[i] = 1; ++placed; }
        }
    Seg empty{0, {}, 1.0, 1}, third{300, std::vector<char>(300, 0), 0.7, 1};
    for (int i = 0; i < 300; i += 30) third.inside[i] = 1;
    Seg dense{20, std::vector<char>(20, 1), 0.9, 1};
    int ncall = 0;
    if (run({sparse, empty, third}, false, net, latents, stride)) return 1;
    ++ncall;
    if (run({sparse, empty, third}, true, net, latents, stride)) return 1;
    ++ncall;
    if (run({dense}, false, net, latents, stride)) return 1;
    ++ncall;
    printf("%d calls %ld compacted\n", ncall, compacted);
    return 0;
}
