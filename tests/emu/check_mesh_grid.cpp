// Test harness (CPU, test infrastructure): csrc/mesh_grid.hip through the fiber emulator as a program of its own, so that it can
// be built with the address and undefined-behaviour sanitizers: every array is a heap block of exactly the size the ABI asks for,
// and a read or a write outside one ends the run.  The calls are the seams of tests/test_emu_mesh_grid.py with meshes drawn here:
// disjoint rotated boxes (12 faces), tetrahedra (4) and one triangular bipyramid (6) on a lattice inside the cube, so that a mesh
// has exactly T - 2, T, T + 2, 3 T + 6 or 4 faces (T = DSS_MESH_GRID_TILE), each on the grids 2^3, 8^3, 9^3 and 7 x 9 x 11; a batch
// of two meshes with different grids; a face index of nv and one of -1 (status word set, nothing outside the blocks touched); the
// return codes.  Checked against a plain double loop in another form -- the foot on the triangle's plane where it lies inside,
// else the least of the three segment distances; the same solid-angle sum -- at every sample: the sign, and the value to
// 1e-12 scale, after the reference alone has shown |phi| >= 1e-6 scale and |w - round(w)| <= 1e-6 there.
// Prints "<calls> calls <samples> samples worst <error / bound>"; exit code 1 on any mismatch.
#define DSS_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../diffsdfsim_amd/csrc/mesh_grid.hip"

struct V3 { double x, y, z; };
static V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double norm(V3 a) { return std::sqrt(dot(a, a)); }

struct Mesh { std::vector<double> v; std::vector<int> f; int nv() const { return (int)v.size() / 3; } int nf() const { return (int)f.size() / 3; } };

static V3 rotated(V3 p)      // by the quaternion (0.9, 0.3, -0.2, 0.1) normalised
{
    const double n = std::sqrt(0.95), w = 0.9 / n, x = 0.3 / n, y = -0.2 / n, z = 0.1 / n;
    return {(1 - 2 * (y * y + z * z)) * p.x + 2 * (x * y - z * w) * p.y + 2 * (x * z + y * w) * p.z,
            2 * (x * y + z * w) * p.x + (1 - 2 * (x * x + z * z)) * p.y + 2 * (y * z - x * w) * p.z,
            2 * (x * z - y * w) * p.x + 2 * (y * z + x * w) * p.y + (1 - 2 * (x * x + y * y)) * p.z};
}

static void add(Mesh &m, const std::vector<V3> &v, const std::vector<int> &f, V3 at)
{
    const int base = m.nv();
    for (V3 p : v) { p = rotated(p) + at; m.v.push_back(p.x); m.v.push_back(p.y); m.v.push_back(p.z); }
    for (int i : f) m.f.push_back(base + i);
}

// a closed mesh of exactly nf faces (even, >= 4): components of radius r on the 5^3 lattice of pitch 0.3 scale
static Mesh mesh_of(int nf, double scale)
{
    Mesh m;
    const double r = 0.1 * scale;
    int spot = 0, left = nf;
    auto at = [&]() { const int s = spot++; return V3{0.3 * scale * (s % 5 - 2), 0.3 * scale * (s / 5 % 5 - 2), 0.3 * scale * (s / 25 - 2)}; };
    if (left % 4 == 2) {
        const double c = 0.5, s = std::sqrt(0.75);
        add(m, {{r, 0, 0}, {-c * r, s * r, 0}, {-c * r, -s * r, 0}, {0, 0, 0.8 * r}, {0, 0, -0.8 * r}},
            {0, 1, 3, 1, 2, 3, 2, 0, 3, 1, 0, 4, 2, 1, 4, 0, 2, 4}, at());
        left -= 6;
    }
    while (left >= 12 && (left - 12) % 4 == 0 && spot < 100) {
        std::vector<V3> v;
        for (int i = 0; i < 8; ++i) v.push_back({(i & 4 ? 0.8 : -0.8) * r, (i & 2 ? 0.6 : -0.6) * r, (i & 1 ? 0.45 : -0.45) * r});
        add(m, v, {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3}, at());
        left -= 12;
    }
    for (; left > 0; left -= 4) {
        const double t = r / std::sqrt(3.0);
        add(m, {{t, t, t}, {t, -t, -t}, {-t, t, -t}, {-t, -t, t}}, {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2}, at());
    }
    if (m.nf() != nf || spot > 125) { printf("mesh_of(%d): %d faces, %d spots\n", nf, m.nf(), spot); exit(1); }
    return m;
}

static double segment(V3 p, V3 a, V3 b)
{
    const V3 e = b - a;
    double t = dot(p - a, e) / dot(e, e);
    t = t < 0 ? 0 : (t > 1 ? 1 : t);
    return norm(p - a - t * e);
}

// -> phi; *w: the winding number
static double reference(const Mesh &m, V3 p, double *w)
{
    double best = HUGE_VAL, sum = 0;
    for (int t = 0; t < m.nf(); ++t) {
        V3 c[3];
        for (int k = 0; k < 3; ++k) { const double *q = &m.v[3 * (size_t)m.f[3 * t + k]]; c[k] = {q[0], q[1], q[2]}; }
        const V3 n = cross(c[1] - c[0], c[2] - c[0]);
        const double nn = dot(n, n), h = dot(p - c[0], n) / nn;
        const V3 foot = p - h * n;
        double d;
        if (dot(cross(c[1] - c[0], foot - c[0]), n) >= 0 && dot(cross(c[2] - c[1], foot - c[1]), n) >= 0 && dot(cross(c[0] - c[2], foot - c[2]), n) >= 0)
            d = std::fabs(dot(p - c[0], n)) / std::sqrt(nn);
        else
            d = std::fmin(std::fmin(segment(p, c[0], c[1]), segment(p, c[1], c[2])), segment(p, c[2], c[0]));
        best = std::fmin(best, d);
        const V3 a = c[0] - p, b = c[1] - p, cc = c[2] - p;
        const double la = norm(a), lb = norm(b), lc = norm(cc);
        sum += 2.0 * std::atan2(dot(a, cross(b, cc)), la * lb * lc + dot(a, b) * lc + dot(b, cc) * la + dot(cc, a) * lb);
    }
    *w = sum / (4.0 * M_PI);
    return *w > 0.5 ? -best : best;
}

static double worst = 0.0;
static long nsample = 0;

struct Grid { int n[3]; double scale; };

// bad: a face index to plant in mesh 0 (0 = none; the face is left out of the reference): the status word has to say so
static int run(std::vector<Mesh> meshes, const std::vector<Grid> &grids, int bad)
{
    const int nm = (int)meshes.size();
    std::vector<int> voff(nm + 1, 0), foff(nm + 1, 0), dims(3 * nm), goff(nm), want_status(nm, 0);
    std::vector<double> scale(nm);
    int total = 0, max_samples = 0, max_faces = 0;
    for (int m = 0; m < nm; ++m) {
        voff[m + 1] = voff[m] + meshes[m].nv(); foff[m + 1] = foff[m] + meshes[m].nf();
        const int n = grids[m].n[0] * grids[m].n[1] * grids[m].n[2];
        for (int d = 0; d < 3; ++d) dims[3 * m + d] = grids[m].n[d];
        goff[m] = total; total += n; scale[m] = grids[m].scale;
        if (n > max_samples) max_samples = n;
        if (meshes[m].nf() > max_faces) max_faces = meshes[m].nf();
    }
    std::vector<double> verts;
    std::vector<int> faces;
    for (int m = 0; m < nm; ++m) {
        verts.insert(verts.end(), meshes[m].v.begin(), meshes[m].v.end());
        faces.insert(faces.end(), meshes[m].f.begin(), meshes[m].f.end());
    }
    if (bad) {      // the last face of mesh 0: in the pooled array it names a vertex of the next mesh, or the end of the block
        faces[3 * (size_t)foff[1] - 1] = bad;
        meshes[0].f.resize(meshes[0].f.size() - 3);
        want_status[0] = DSS_MESH_GRID_MALFORMED;
    }
    std::vector<double> out(total, -7.0);
    std::vector<int> status(nm, -7);
    if (dss_mesh_grid_sdf(nm, verts.data(), faces.data(), voff.data(), foff.data(), dims.data(), goff.data(), scale.data(), max_samples, max_faces,
                          out.data(), status.data(), nullptr) != 0) { printf("return code\n"); return 1; }
    for (int m = 0; m < nm; ++m) {
        if (status[m] != want_status[m]) { printf("mesh %d: status %d, want %d\n", m, status[m], want_status[m]); return 1; }
        const Grid &g = grids[m];
        for (int i = 0; i < g.n[0]; ++i)
            for (int j = 0; j < g.n[1]; ++j)
                for (int k = 0; k < g.n[2]; ++k, ++nsample) {
                    const V3 p = {g.scale * (-1.0 + 2.0 * i / (g.n[0] - 1)), g.scale * (-1.0 + 2.0 * j / (g.n[1] - 1)), g.scale * (-1.0 + 2.0 * k / (g.n[2] - 1))};
                    double w;
                    const double phi = reference(meshes[m], p, &w), got = out[goff[m] + (i * g.n[1] + j) * g.n[2] + k] * g.scale;
                    // (a mesh whose bad face was left out is open: its winding number is no integer, only its distance is held)
                    const bool open = want_status[m] != 0;
                    if (!open && (std::fabs(phi) < 1e-6 * g.scale || std::fabs(w - std::round(w)) > 1e-6)) { printf("input condition: phi %g w %.9f\n", phi, w); return 1; }
                    const double err = open ? std::fabs(std::fabs(got) - std::fabs(phi)) : std::fabs(got - phi), bound = 1e-12 * g.scale;
                    if (!(err <= bound) || (!open && (got < 0) != (phi < 0))) {
                        printf("mesh %d sample (%d, %d, %d): %.17g, want %.17g\n", m, i, j, k, got, phi);
                        return 1;
                    }
                    if (err / bound > worst) worst = err / bound;
                }
    }
    return 0;
}

int main()
{
    const int T = DSS_MESH_GRID_TILE;
    const Grid grids[4] = {{{2, 2, 2}, 1.0}, {{8, 8, 8}, 1.0}, {{9, 9, 9}, 1.0}, {{7, 9, 11}, 1.0}};
    int ncall = 0;
    for (int nf : {T - 2, T, T + 2, 3 * T + 6, 4})
        for (const Grid &g : grids) {
            if (run({mesh_of(nf, 1.0)}, {g}, 0)) return 1;
            ++ncall;
        }
    if (run({mesh_of(T + 2, 0.8), mesh_of(30, 1.0)}, {{{7, 9, 11}, 0.8}, {{9, 9, 9}, 1.0}}, 0)) return 1;
    const Mesh one = mesh_of(T + 2, 1.0);
    if (run({one, mesh_of(4, 1.0)}, {grids[2], grids[1]}, one.nv())) return 1;      // index nv: a vertex of the next mesh
    if (run({one}, {grids[2]}, one.nv())) return 1;                                 // index nv: the end of the vertex block
    if (run({one}, {grids[2]}, -1)) return 1;                                       // index -1: before it
    ncall += 4;
    // the return codes write nothing: null outputs would be dereferenced otherwise
    int i1[2] = {0, 1};
    double d1[3] = {0, 0, 0};
    if (dss_mesh_grid_sdf(0, d1, i1, i1, i1, i1, i1, d1, 8, 1, d1, i1, nullptr) != DSS_E_BADARG ||
        dss_mesh_grid_sdf(1, d1, i1, i1, i1, i1, i1, d1, 8, 1, nullptr, i1, nullptr) != DSS_E_BADARG ||
        dss_mesh_grid_sdf(1, d1, i1, i1, i1, i1, i1, d1, 8, 1, d1, nullptr, nullptr) != DSS_E_BADARG ||
        dss_mesh_grid_sdf(1 << 23, d1, i1, i1, i1, i1, i1, d1, 256, 1, d1, i1, nullptr) != DSS_E_UNSUPPORTED ||
        dss_mesh_grid_sdf(1, d1, i1, i1, i1, i1, i1, d1, 0x7fffffff, 1, d1, i1, nullptr) != DSS_E_UNSUPPORTED) { printf("return codes\n"); return 1; }
    printf("%d calls %ld samples worst %.3f\n", ncall, nsample, worst);
    return 0;
}
