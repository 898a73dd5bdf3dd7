// sdf2d_contacts.hip -- contacts between 2-D SDF bodies: the reference's SDFContactHandler (sdf_physics/physics/contacts.py:
// 31-141) with the bodies of sdf_physics/physics/bodies.py (circle, rect, bowl, grid), for a batch of body pairs.
//
// One 64-lane workgroup (one wavefront) per pair, lanes over the edges of an outline in strides of 64.  For every edge of
// body 1's outline a Frank-Wolfe search over the edge minimises body 2's SDF (start at the midpoint, cull, 32 steps towards
// the end point the gradient prefers, a tie taking the first), then the same with the bodies exchanged; what ends at
// phi <= eps is a contact.  The contacts of both directions are compacted into LDS in candidate order by wavefront ballots
// and thinned as the reference thins them: singular values of the centred p1's (closed-form 2 x 2 eigenproblem; which are
// above 1e-5 gives the dimension), then hull vertices (dimension 2; the gift wrap and collinearity measure of wrap2d.h),
// the two extremes along the principal direction (1) or the first contact (0).  The thinning runs on lane 0: a few dozen
// points, and a serial wrap keeps its order free of reduction trees.
//
// The analytic outlines (4, 64, 64 vertices) are generated from the shape parameters, a grid's comes from the pooled table.
// The same templated query and outline code serves the forward (T = double) and the vector-Jacobian product (T = Dual<NS>):
// to autograd the search is a constant convex combination x = (1 - t) a + t b of the edge's end points, so the backward
// kernel rebuilds every kept contact from its saved (direction, edge, t), a few seeds per pass, and sums per pair in a fixed
// order.  Branch decisions read values only and repeat those of the reference; this file includes geom.h, which switches
// FMA contraction off, so the comparisons that decide them are evaluated in the reference's order.
#include <math.h>

#include "../../include/diffsdfsim_hip.h"
#include "geom.h"
#include "../../include/sdf2d_contacts.h"
#include "wrap2d.h"

namespace {
using namespace dss;

constexpr int MAXCAND = DSS_SDF2D_MAXCAND, NITER = 32, NCOORD = 12;

__host__ __device__ inline double t_min0(double a) { return a < 0.0 ? a : 0.0; }
// torch.min(x, tensor(0)): at an exact tie autograd gives each argument half the gradient
template <int N> __host__ __device__ inline Dual<N> t_min0(const Dual<N> &a)
{
    if (a.v < 0.0) return a;
    if (a.v > 0.0) return Dual<N>(0.0);
    return a * 0.5;
}
__host__ __device__ inline double sign0(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

template <class T> struct Body {
    int kind;
    T rot, pos[2], prm[2], scale, c, s;
    // grid bodies: samples, central differences, outline (unit scale) and its edges
    const double *vals, *grads, *gverts;
    const int *gedges;
    int n0, n1, nv, ne;
    // backward with respect to the table (dss_sdf2d_contacts_backward_grids): where the grid starts in the pooled arrays, and
    // which of its entries carry the tangents of this pass (0 none, 1 the cell's four samples, 2 / 3 the first / second
    // component of their central differences, 4 the two vertices sv[0], sv[1] of an edge)
    int val_base, vert_base, lseed, sv[2];
};

struct Args {
    int P, cap, cand_cap;
    const int *kind, *grid_id;
    const double *pose, *prm, *scale;
    DssSdf2dGrids G;
    double eps;
};

// false: the pair is malformed (unknown kind, grid id outside the table)
template <class T> __host__ __device__ inline bool load_body(const Args &A, int p, int s, Body<T> &b)
{
    const size_t o = (size_t)s * A.P + p;
    b.kind = A.kind[o];
    b.rot = T(A.pose[3 * o]); b.pos[0] = T(A.pose[3 * o + 1]); b.pos[1] = T(A.pose[3 * o + 2]);
    b.prm[0] = T(A.prm[2 * o]); b.prm[1] = T(A.prm[2 * o + 1]);
    b.scale = T(A.scale[o]);
    b.vals = b.grads = b.gverts = nullptr; b.gedges = nullptr;
    b.n0 = b.n1 = b.nv = 0;
    b.val_base = b.vert_base = b.lseed = 0; b.sv[0] = b.sv[1] = -1;
    if (b.kind == DSS_SDF2D_RECT) b.ne = 4;
    else if (b.kind == DSS_SDF2D_CIRCLE || b.kind == DSS_SDF2D_BOWL) b.ne = 64;
    else if (b.kind == DSS_SDF2D_GRID) {
        const int g = A.grid_id[o];
        if (g < 0 || g >= A.G.ngrids) return false;
        b.n0 = A.G.dims[2 * g]; b.n1 = A.G.dims[2 * g + 1];
        if (b.n0 < 2 || b.n1 < 2) return false;
        b.vals = A.G.vals + A.G.val_off[g];
        b.grads = A.G.grads + 2 * (size_t)A.G.val_off[g];
        b.gverts = A.G.verts + 2 * (size_t)A.G.vert_off[g];
        b.gedges = A.G.edges + 2 * (size_t)A.G.edge_off[g];
        b.val_base = A.G.val_off[g]; b.vert_base = A.G.vert_off[g];
        b.nv = A.G.vert_off[g + 1] - A.G.vert_off[g];
        b.ne = A.G.edge_off[g + 1] - A.G.edge_off[g];
        if (b.nv < 0 || b.ne < 0) return false;
    } else return false;
    return true;
}
template <class T> __host__ __device__ inline void finish_body(Body<T> &b) { b.c = t_cos(b.rot); b.s = t_sin(b.rot); }

// torch.linspace(start, end, steps)[i] as the CPU kernel evaluates it: from the start in the first half, from the end after
__host__ __device__ inline double linspace_at(double start, double end, int steps, int i)
{
    const double step = (end - start) / (double)(steps - 1);
    return i < steps / 2 ? start + step * (double)i : end - step * (double)(steps - 1 - i);
}

// a table entry as a T, with tangent `slot` set where T carries tangents
template <class T> struct Seeded { __host__ __device__ static T at(double x, int) { return T(x); } };
template <int N> struct Seeded<Dual<N>> {
    __host__ __device__ static Dual<N> at(double x, int slot) { Dual<N> r(x); r.d[slot] = 1.0; return r; }
};

// vertex i of the outline in world coordinates (get_surface: verts_loc @ R^T + pos)
template <class T> __host__ __device__ inline void outline_vertex(const Body<T> &B, int i, T *w)
{
    T l[2];
    if (B.kind == DSS_SDF2D_RECT) {
        const T h0 = B.prm[0] / 2.0, h1 = B.prm[1] / 2.0;
        l[0] = (i == 0 || i == 3) ? h0 : -h0;
        l[1] = (i == 0 || i == 1) ? h1 : -h1;
    } else if (B.kind == DSS_SDF2D_CIRCLE) {
        const double a = linspace_at(0.0, (2.0 * M_PI / 64.0) * 63.0, 64, i);
        l[0] = cos(a) * B.prm[0]; l[1] = sin(a) * B.prm[0];
    } else if (B.kind == DSS_SDF2D_BOWL) {
        const double a = linspace_at(-M_PI, 0.0, 32, i < 32 ? i : 63 - i);
        const T rr = i < 32 ? B.prm[0] - B.prm[1] : B.prm[0] + B.prm[1];
        l[0] = cos(a) * rr; l[1] = sin(a) * rr + B.prm[0] / 2.0;
    } else if (B.lseed == 4 && (i == B.sv[0] || i == B.sv[1])) {      // tangents 0, 1 on the edge's first vertex, 2, 3 on its second
        const int s0 = i == B.sv[0] ? 0 : 2;
        l[0] = Seeded<T>::at(B.gverts[2 * i], s0) * B.scale; l[1] = Seeded<T>::at(B.gverts[2 * i + 1], s0 + 1) * B.scale;
    } else {
        l[0] = B.gverts[2 * i] * B.scale; l[1] = B.gverts[2 * i + 1] * B.scale;
    }
    w[0] = l[0] * B.c + l[1] * (-B.s) + B.pos[0];
    w[1] = l[0] * B.s + l[1] * B.c + B.pos[1];
}
// end points of edge e; false: an index outside the outline (grids only: the table is device memory)
template <class T> __host__ __device__ inline bool edge_ends(const Body<T> &B, int e, int &i0, int &i1)
{
    if (B.kind != DSS_SDF2D_GRID) { i0 = e; i1 = (e + 1) % B.ne; return true; }
    i0 = B.gedges[2 * e]; i1 = B.gedges[2 * e + 1];
    return i0 >= 0 && i0 < B.nv && i1 >= 0 && i1 < B.nv;
}

// query_sdfs of one point: value (world units) and unit gradient (world frame).  corners: where a grid was interpolated, the
// numbers of the cell's four samples within the grid (left as they are otherwise)
template <class T> __host__ __device__ inline void query(const Body<T> &B, const T *pt, T &phi, T *g, size_t *corners = nullptr)
{
    const T dx = pt[0] - B.pos[0], dy = pt[1] - B.pos[1];
    const T lx = dx * B.c + dy * B.s, ly = dx * (-B.s) + dy * B.c;
    const double half = val(B.scale) / 2.0;
    if (!(fabs(val(lx)) < half && fabs(val(ly)) < half)) {     // outside the body's box: the scale, no gradient
        phi = B.scale;
        g[0] = T(0.0); g[1] = T(0.0);
        return;
    }
    T gl[2];
    if (B.kind == DSS_SDF2D_CIRCLE) {
        const T n = t_sqrt(lx * lx + ly * ly);
        phi = n - B.prm[0];
        gl[0] = lx / n; gl[1] = ly / n;
    } else if (B.kind == DSS_SDF2D_RECT) {
        const T d0 = t_abs(lx) - B.prm[0] / 2.0, d1 = t_abs(ly) - B.prm[1] / 2.0;
        const bool outer = val(d0) > 0.0 || val(d1) > 0.0;
        const double s0 = val(lx) < 0.0 ? -1.0 : 1.0, s1 = val(ly) < 0.0 ? -1.0 : 1.0;
        const int ind = val(d1) > val(d0) ? 1 : 0;      // torch.max(dim): the first of equal
        const T md = ind ? d1 : d0;
        const T q0 = t_maximum(d0, T(0.0)), q1 = t_maximum(d1, T(0.0));
        phi = t_sqrt(q0 * q0 + q1 * q1) + t_min0(md);
        T go[2];
        if (outer) { go[0] = q0 * s0; go[1] = q1 * s1; }
        else { go[0] = T(ind == 0 ? s0 : 0.0); go[1] = T(ind == 1 ? s1 : 0.0); }
        const T n = t_sqrt(go[0] * go[0] + go[1] * go[1]);
        gl[0] = go[0] / n; gl[1] = go[1] / n;
    } else if (B.kind == DSS_SDF2D_BOWL) {
        const T r = B.prm[0], d = B.prm[1];
        const T px = lx, py = ly - r / 2.0;
        const T ax = t_abs(px), pn = t_sqrt(ax * ax + py * py);
        T a = val(py) < 0.0 ? pn : ax;
        a = t_abs(a - r) - d;
        const T m0 = t_maximum(a, T(0.0)), m1 = t_maximum(py, T(0.0));
        phi = t_sqrt(m0 * m0 + m1 * m1) + t_min0(t_max(a, py));
        T go[2];
        if (val(py) >= 0.0) {
            go[0] = m0 * (sign0(val(px)) * sign0(fabs(val(px)) - val(r)));
            go[1] = m1;
        } else {
            const double sg = sign0(val(pn) - val(r));
            go[0] = px * sg; go[1] = py * sg;
        }
        const T n = t_sqrt(go[0] * go[0] + go[1] * go[1]);
        gl[0] = go[0] / n; gl[1] = go[1] / n;
    } else {
        // bilinear interpolation of the samples and of their central differences at index position (l / scale + 0.5)(n - 1)
        const T ix = (lx / B.scale + 0.5) * (double)(B.n0 - 1), iy = (ly / B.scale + 0.5) * (double)(B.n1 - 1);
        int x0 = (int)floor(val(ix)), y0 = (int)floor(val(iy)), x1 = x0 + 1, y1 = y0 + 1;
        x0 = x0 < 0 ? 0 : (x0 > B.n0 - 1 ? B.n0 - 1 : x0); x1 = x1 < 0 ? 0 : (x1 > B.n0 - 1 ? B.n0 - 1 : x1);
        y0 = y0 < 0 ? 0 : (y0 > B.n1 - 1 ? B.n1 - 1 : y0); y1 = y1 < 0 ? 0 : (y1 > B.n1 - 1 ? B.n1 - 1 : y1);
        const T ux = (double)x1 - ix, vx = ix - (double)x0, uy = (double)y1 - iy, vy = iy - (double)y0;
        const T wa = ux * uy, wb = ux * vy, wc = vx * uy, wd = vx * vy;
        const size_t ia = (size_t)x0 * B.n1 + y0, ib = (size_t)x0 * B.n1 + y1, ic = (size_t)x1 * B.n1 + y0, id = (size_t)x1 * B.n1 + y1;
        if (corners) { corners[0] = ia; corners[1] = ib; corners[2] = ic; corners[3] = id; }
        T v, go[2];
        if (B.lseed >= 1 && B.lseed <= 3) {      // the same sums over table entries that carry tangent c at corner c
            const size_t at[4] = {ia, ib, ic, id};
            const T w[4] = {wa, wb, wc, wd};
            T c[4], d[4][2];
            for (int k = 0; k < 4; ++k) {
                c[k] = B.lseed == 1 ? Seeded<T>::at(B.vals[at[k]], k) : T(B.vals[at[k]]);
                for (int j = 0; j < 2; ++j) d[k][j] = B.lseed == 2 + j ? Seeded<T>::at(B.grads[2 * at[k] + j], k) : T(B.grads[2 * at[k] + j]);
            }
            v = w[0] * c[0] + w[1] * c[1] + w[2] * c[2] + w[3] * c[3];
            for (int j = 0; j < 2; ++j) go[j] = w[0] * d[0][j] + w[1] * d[1][j] + w[2] * d[2][j] + w[3] * d[3][j];
        } else {
            v = wa * B.vals[ia] + wb * B.vals[ib] + wc * B.vals[ic] + wd * B.vals[id];
            for (int k = 0; k < 2; ++k)
                go[k] = wa * B.grads[2 * ia + k] + wb * B.grads[2 * ib + k] + wc * B.grads[2 * ic + k] + wd * B.grads[2 * id + k];
        }
        const T n = t_sqrt(go[0] * go[0] + go[1] * go[1]);
        if (val(n) != 0.0) { gl[0] = go[0] / n; gl[1] = go[1] / n; }
        else { gl[0] = go[0]; gl[1] = go[1]; }
        phi = v * B.scale;
    }
    g[0] = gl[0] * B.c + gl[1] * (-B.s);
    g[1] = gl[0] * B.s + gl[1] * B.c;
}

// the contact tuple of a point x with value phi and gradient g (contacts.py:62-79): the normal is g in direction 0 (body 1's
// edges against body 2) and -g in direction 1; both points are x less phi g, taken from the two positions
template <class T> __host__ __device__ inline void make_tuple(const T *x, const T &phi, const T *g, int dir, const T *pos1, const T *pos2, T *row)
{
    for (int k = 0; k < 2; ++k) {
        row[k] = dir ? -g[k] : g[k];
        row[2 + k] = (x[k] - pos1[k]) - phi * g[k];
        row[4 + k] = (x[k] - pos2[k]) - phi * g[k];
    }
    row[6] = -phi;
}

// Frank-Wolfe over edge e of O against the SDF of Q (_search_contacts, contacts.py:113-140).  true: a contact; row, t set
__host__ __device__ inline bool search_edge(const Body<double> &O, const Body<double> &Q, int e, double eps, int dir, const double *pos1,
                                            const double *pos2, double *row, double &t, bool &bad_edge)
{
    int i0, i1;
    if (!edge_ends(O, e, i0, i1)) { bad_edge = true; return false; }
    double a[2], b[2], x[2], phi, g[2];
    outline_vertex(O, i0, a);
    outline_vertex(O, i1, b);
    for (int k = 0; k < 2; ++k) x[k] = (a[k] + b[k]) / 2.0;
    query(Q, x, phi, g);
    const double ra = sqrt((x[0] - a[0]) * (x[0] - a[0]) + (x[1] - a[1]) * (x[1] - a[1]));
    const double rb = sqrt((x[0] - b[0]) * (x[0] - b[0]) + (x[1] - b[1]) * (x[1] - b[1]));
    if (!(phi < fmax(ra, rb)) || (g[0] == 0.0 && g[1] == 0.0)) return false;
    t = 0.5;
    for (int it = 0; it < NITER; ++it) {
        query(Q, x, phi, g);
        const double da = a[0] * g[0] + a[1] * g[1], db = b[0] * g[0] + b[1] * g[1];
        const bool second = db < da;                        // argmin over the two end points, the first on a tie
        const double gamma = 2.0 / ((double)it + 2.0);
        for (int k = 0; k < 2; ++k) x[k] = (1.0 - gamma) * x[k] + gamma * (second ? b[k] : a[k]);
        t = (1.0 - gamma) * t + gamma * (second ? 1.0 : 0.0);
    }
    query(Q, x, phi, g);
    if (!(phi <= eps)) return false;
    make_tuple(x, phi, g, dir, pos1, pos2, row);
    return true;
}

// Thinning of n contacts whose p1 are (px[k], py[k]) (contacts.py:89-106), on one lane.  keep[] receives the kept contacts'
// numbers in ascending order; returns how many.
__host__ __device__ inline int thin(const double *px, const double *py, int n, int *keep)
{
    if (n <= 1) { if (n == 1) keep[0] = 0; return n; }
    double mx = 0.0, my = 0.0, amax = 0.0;
    for (int k = 0; k < n; ++k) { mx += px[k]; my += py[k]; amax = fmax(amax, fmax(fabs(px[k]), fabs(py[k]))); }
    mx /= n; my /= n;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int k = 0; k < n; ++k) { const double dx = px[k] - mx, dy = py[k] - my; sxx += dx * dx; sxy += dx * dy; syy += dy * dy; }
    // principal axis of the scatter matrix in closed form; the singular values are the root sums of squares along it and
    // across it (summed as such: the small one would drown in the difference of the eigenvalue formula)
    const double th = 0.5 * atan2(2.0 * sxy, sxx - syy), ux = cos(th), uy = sin(th);
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < n; ++k) {
        const double dx = px[k] - mx, dy = py[k] - my, al = dx * ux + dy * uy, ac = dy * ux - dx * uy;
        s1 += al * al; s2 += ac * ac;
    }
    const int dim = (sqrt(s1) > 1e-5 ? 1 : 0) + (sqrt(s2) > 1e-5 ? 1 : 0);
    if (dim == 0) { keep[0] = 0; return 1; }
    if (dim == 1) {
        int lo = 0, hi = 0;
        double vlo = INFINITY, vhi = -INFINITY;
        for (int k = 0; k < n; ++k) {
            const double v = px[k] * ux + py[k] * uy;
            if (v < vlo) { vlo = v; lo = k; }
            if (v > vhi) { vhi = v; hi = k; }
        }
        if (lo == hi) { keep[0] = lo; return 1; }
        keep[0] = lo < hi ? lo : hi; keep[1] = lo < hi ? hi : lo;
        return 2;
    }
    // dimension 2: gift wrap from the lexicographic minimum (first coordinates equal to round-off count as equal)
    const double tolf = wrap2_tolf(amax), dtol = wrap2_dtol(amax), dtol2 = dtol * dtol;
    int i0 = 0;
    for (int k = 1; k < n; ++k) if (px[k] < px[i0]) i0 = k;
    int iS = -1;
    for (int k = 0; k < n; ++k) if (px[k] <= px[i0] + dtol && (iS < 0 || py[k] < py[iS])) iS = k;
    for (int k = 0; k < n; ++k) keep[k] = 0;      // (flags first, numbers after)
    int cur = iS;
    for (int step = 0; step < n; ++step) {
        keep[cur] = 1;
        int best = -1;
        double bx = 0.0, by = 0.0;
        for (int k = 0; k < n; ++k) {
            const double qx = px[k] - px[cur], qy = py[k] - py[cur];
            if (!(qx * qx + qy * qy > tolf * tolf)) continue;      // the current point or a duplicate of it
            if (best < 0 || wrap2_better(bx, by, qx, qy, dtol2)) { best = k; bx = qx; by = qy; }
        }
        if (best < 0 || best == iS || keep[best]) break;
        const double dx = px[best] - px[iS], dy = py[best] - py[iS];
        if (!(dx * dx + dy * dy > tolf * tolf)) break;             // coincident with the start: the loop is closed
        cur = best;
    }
    int m = 0;
    for (int k = 0; k < n; ++k) if (keep[k]) keep[m++] = k;
    return m;
}

__global__ void __launch_bounds__(64)
sdf2d_forward_kernel(Args A, double *out, int *count, int *status, int *tag, double *tpar, int *ncand, double *cand, int *cand_tag)
{
    __shared__ double c_row[7][MAXCAND], c_t[MAXCAND];
    __shared__ int c_tag[MAXCAND], keep[MAXCAND], sh_n;
    const int p = blockIdx.x, lane = threadIdx.x, cap = A.cap;
    Body<double> b[2];
    const bool ok = load_body(A, p, 0, b[0]) & load_body(A, p, 1, b[1]);
    int st = ok ? 0 : DSS_SDF2D_MALFORMED, n = 0;
    if (ok) {
        finish_body(b[0]);
        finish_body(b[1]);
        bool bad_edge = false;
        for (int dir = 0; dir < 2; ++dir) {
            const Body<double> &O = b[dir], &Q = b[1 - dir];
            for (int base = 0; base < O.ne; base += 64) {
                const int e = base + lane;
                double row[7], t = 0.0;
                const bool hit = e < O.ne && search_edge(O, Q, e, A.eps, dir, b[0].pos, b[1].pos, row, t, bad_edge);
                const unsigned long long mask = __ballot(hit ? 1 : 0);
                if (hit) {
                    const int slot = n + __popcll(lane ? mask & ((1ull << lane) - 1ull) : 0ull);
                    if (slot < MAXCAND) {
                        for (int k = 0; k < 7; ++k) c_row[k][slot] = row[k];
                        c_t[slot] = t;
                        c_tag[slot] = dir * (1 << 24) + e;
                    }
                }
                n += __popcll(mask);
            }
        }
        if (__ballot(bad_edge ? 1 : 0)) st |= DSS_SDF2D_MALFORMED;
        if (n > MAXCAND) st |= DSS_SDF2D_OVER_CAND;
    }
    __syncthreads();
    if (st) n = 0;
    if (lane == 0) sh_n = thin(c_row[2], c_row[3], n, keep);
    __syncthreads();
    int m = sh_n;
    if (m > cap) st |= DSS_SDF2D_OVER_CAP;
    if (lane == 0) { count[p] = (st & ~DSS_SDF2D_OVER_CAP) ? 0 : m; status[p] = st; }
    if (st) m = 0;
    for (int q = lane; q < cap; q += 64) {
        const size_t o = (size_t)p * cap + q;
        const int k = q < m ? keep[q] : -1;
        for (int j = 0; j < 7; ++j) out[o * 7 + j] = k >= 0 ? c_row[j][k] : 0.0;
        tag[2 * o] = k >= 0 ? c_tag[k] >> 24 : 0;
        tag[2 * o + 1] = k >= 0 ? c_tag[k] & ((1 << 24) - 1) : 0;
        tpar[o] = k >= 0 ? c_t[k] : 0.0;
    }
    if (ncand && lane == 0) ncand[p] = (st & (DSS_SDF2D_MALFORMED | DSS_SDF2D_OVER_CAND)) ? 0 : n;
    if (cand && cand_tag)
        for (int q = lane; q < A.cand_cap; q += 64) {
            const size_t o = (size_t)p * A.cand_cap + q;
            const bool on = q < n;
            for (int j = 0; j < 7; ++j) cand[o * 7 + j] = on ? c_row[j][q] : 0.0;
            cand_tag[2 * o] = on ? c_tag[q] >> 24 : 0;
            cand_tag[2 * o + 1] = on ? c_tag[q] & ((1 << 24) - 1) : 0;
        }
}

constexpr int NS = 4;      // seeds per pass of the vector-Jacobian product

// coordinate k of the pair: body k / 6, then angle, x, y, the two shape parameters, scale
__host__ __device__ inline void seed_coord(Body<Dual<NS>> *b, int k, int slot)
{
    Body<Dual<NS>> &B = b[k / 6];
    const int j = k % 6;
    if (j == 0) B.rot.d[slot] = 1.0;
    else if (j < 3) B.pos[j - 1].d[slot] = 1.0;
    else if (j < 5) B.prm[j - 3].d[slot] = 1.0;
    else B.scale.d[slot] = 1.0;
}

constexpr int NLOCAL = 16;      // table entries one contact reads with a tangent: 4 samples, 8 central differences, 2 x 2 vertex numbers

// The tuple of the kept contact (dir, e, t) of pair p on NS tangents: coordinates k0 .. k0 + NS - 1 of the pair (lpass 0), or
// table entries (lpass 1: the four samples of Q's cell, 2 / 3: the components of their central differences, 4: the two end
// vertices of O's edge).  false: nothing to rebuild (a malformed pair or edge; a pass over a table the body does not read).
// corners: numbers of the cell's samples within Q's grid ((size_t)-1 where none was interpolated); ends: O's two vertices
__host__ __device__ inline bool rebuild(const Args &A, int p, int dir, int e, double t, int k0, int lpass, Dual<NS> *row, size_t *corners,
                                        int *ends, int *val_base, int *vert_base)
{
    Body<Dual<NS>> b[2];
    if (!(load_body(A, p, 0, b[0]) & load_body(A, p, 1, b[1]))) return false;
    if (lpass == 0)
        for (int s = 0; s < NS; ++s) seed_coord(b, k0 + s, s);
    finish_body(b[0]);
    finish_body(b[1]);
    Body<Dual<NS>> &O = b[dir], &Q = b[1 - dir];
    int i0, i1;
    if (e >= O.ne || !edge_ends(O, e, i0, i1)) return false;
    if (lpass >= 1 && lpass <= 3) {
        if (Q.kind != DSS_SDF2D_GRID) return false;
        Q.lseed = lpass;
    } else if (lpass == 4) {
        if (O.kind != DSS_SDF2D_GRID) return false;
        O.lseed = 4; O.sv[0] = i0; O.sv[1] = i1;
    }
    Dual<NS> a[2], bb[2], x[2], phi, g[2];
    outline_vertex(O, i0, a);
    outline_vertex(O, i1, bb);
    for (int k = 0; k < 2; ++k) x[k] = a[k] * (1.0 - t) + bb[k] * t;
    if (corners) corners[0] = corners[1] = corners[2] = corners[3] = (size_t)-1;
    query(Q, x, phi, g, corners);
    make_tuple(x, phi, g, dir, b[0].pos, b[1].pos, row);
    if (ends) { ends[0] = i0; ends[1] = i1; *val_base = Q.val_base; *vert_base = O.vert_base; }
    return true;
}

// GRIDS: also the gradient with respect to the table (g_vals, g_grads, g_verts: pooled like the table, zeroed by the caller).
// Per block of 64 contacts every lane leaves its contact's NLOCAL contributions in LDS and lane 0 adds them to global memory
// in contact order, entry by entry: a fixed order within the pair; pairs that share a grid meet in the atomic adds.
template <bool GRIDS>
__global__ void __launch_bounds__(64)
sdf2d_backward_kernel(Args A, const int *count, const int *tag, const double *tpar, const double *gout, double *g_pose, double *g_prm,
                      double *g_scale, double *g_vals, double *g_grads, double *g_verts)
{
    __shared__ double part[64][NCOORD];
    __shared__ double loc_v[GRIDS ? 64 : 1][NLOCAL];
    __shared__ long long loc_at[GRIDS ? 64 : 1][NLOCAL];      // array (0 g_vals, 1 g_grads, 2 g_verts) * 2^48 + element, -1: none
    const int p = blockIdx.x, lane = threadIdx.x, cap = A.cap;
    int n = count[p];
    if (n < 0 || n > cap) n = 0;      // (a pair the forward flagged as over its capacity holds no rows)
    double acc[NCOORD];
    for (int k = 0; k < NCOORD; ++k) acc[k] = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int q = base + lane;
        if constexpr (GRIDS)
            for (int s = 0; s < NLOCAL; ++s) loc_at[lane][s] = -1;
        if (q < n) {
            const size_t o = (size_t)p * cap + q;
            const int dir = tag[2 * o], e = tag[2 * o + 1];
            const double t = tpar[o];
            if (!(dir < 0 || dir > 1 || e < 0)) {
                Dual<NS> row[7];
                for (int k0 = 0; k0 < NCOORD; k0 += NS) {
                    if (!rebuild(A, p, dir, e, t, k0, 0, row, nullptr, nullptr, nullptr, nullptr)) break;
                    for (int s = 0; s < NS; ++s) {
                        double v = 0.0;
                        for (int j = 0; j < 7; ++j) v += gout[o * 7 + j] * row[j].d[s];
                        acc[k0 + s] += v;
                    }
                }
                if constexpr (GRIDS)
                    for (int lpass = 1; lpass <= 4; ++lpass) {
                        size_t corners[4];
                        int ends[2], vb = 0, tb = 0;
                        if (!rebuild(A, p, dir, e, t, 0, lpass, row, corners, ends, &vb, &tb)) continue;
                        if (lpass < 4 && corners[0] == (size_t)-1) continue;      // outside the grid's box: the value is the scale
                        for (int s = 0; s < NS; ++s) {
                            double v = 0.0;
                            for (int j = 0; j < 7; ++j) v += gout[o * 7 + j] * row[j].d[s];
                            long long at;
                            if (lpass == 1) at = (long long)vb + (long long)corners[s];
                            else if (lpass < 4) at = (1ll << 48) + 2 * ((long long)vb + (long long)corners[s]) + (lpass - 2);
                            else at = (2ll << 48) + 2 * ((long long)tb + ends[s >> 1]) + (s & 1);
                            loc_v[lane][(lpass - 1) * NS + s] = v;
                            loc_at[lane][(lpass - 1) * NS + s] = at;
                        }
                    }
            }
        }
        if constexpr (GRIDS) {
            __syncthreads();
            if (lane == 0) {
                const int m = n - base < 64 ? n - base : 64;
                for (int l = 0; l < m; ++l)
                    for (int s = 0; s < NLOCAL; ++s) {
                        const long long at = loc_at[l][s];
                        if (at < 0) continue;
                        double *dst = (at >> 48) == 0 ? g_vals : ((at >> 48) == 1 ? g_grads : g_verts);
                        atomicAdd(dst + (at & ((1ll << 48) - 1)), loc_v[l][s]);
                    }
            }
            __syncthreads();
        }
    }
    for (int k = 0; k < NCOORD; ++k) part[lane][k] = acc[k];
    __syncthreads();
    if (lane < NCOORD) {
        double v = 0.0;
        for (int l = 0; l < 64; ++l) v += part[l][lane];      // lane order: two calls return the same bits
        const int body = lane / 6, j = lane % 6;
        const size_t o = (size_t)body * A.P + p;
        if (j < 3) g_pose[3 * o + j] = v;
        else if (j < 5) g_prm[2 * o + (j - 3)] = v;
        else g_scale[o] = v;
    }
}

bool make_args(Args &A, int npairs, int cap, int cand_cap, const int *kind, const double *pose, const double *prm, const double *scale,
               const int *grid_id, const DssSdf2dGrids *grids, double eps)
{
    if (npairs < 0 || cap < 1 || cand_cap < 0) return false;
    if (npairs > 0 && (!kind || !pose || !prm || !scale || !grid_id)) return false;
    DssSdf2dGrids G = {0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (grids) {
        G = *grids;
        if (G.ngrids < 0) return false;
        if (G.ngrids > 0 && (!G.dims || !G.val_off || !G.vert_off || !G.edge_off || !G.vals || !G.grads || !G.edges || !G.verts)) return false;
    }
    A = Args{npairs, cap, cand_cap, kind, grid_id, pose, prm, scale, G, eps};
    return true;
}
}  // namespace

extern "C" int dss_sdf2d_contacts_forward(int npairs, int cap, const int *kind, const double *pose, const double *prm, const double *scale,
                                          const int *grid_id, const DssSdf2dGrids *grids, double eps, double *out, int *count, int *status,
                                          int *tag, double *tpar, int cand_cap, int *ncand, double *cand, int *cand_tag, void *stream)
{
    Args A;
    if (!make_args(A, npairs, cap, cand_cap, kind, pose, prm, scale, grid_id, grids, eps)) return DSS_E_BADARG;
    if (npairs == 0) return DSS_OK;
    if (!out || !count || !status || !tag || !tpar) return DSS_E_BADARG;
    hipLaunchKernelGGL(sdf2d_forward_kernel, dim3(npairs), dim3(64), 0, (hipStream_t)stream, A, out, count, status, tag, tpar, ncand, cand,
                       cand_tag);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_BADARG;
}

extern "C" int dss_sdf2d_contacts_backward(int npairs, int cap, const int *kind, const double *pose, const double *prm, const double *scale,
                                           const int *grid_id, const DssSdf2dGrids *grids, const int *count, const int *tag,
                                           const double *tpar, const double *gout, double *g_pose, double *g_prm, double *g_scale,
                                           void *stream)
{
    Args A;
    if (!make_args(A, npairs, cap, 0, kind, pose, prm, scale, grid_id, grids, 0.0)) return DSS_E_BADARG;
    if (npairs == 0) return DSS_OK;
    if (!count || !tag || !tpar || !gout || !g_pose || !g_prm || !g_scale) return DSS_E_BADARG;
    hipLaunchKernelGGL(sdf2d_backward_kernel<false>, dim3(npairs), dim3(64), 0, (hipStream_t)stream, A, count, tag, tpar, gout, g_pose, g_prm,
                       g_scale, (double *)nullptr, (double *)nullptr, (double *)nullptr);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_BADARG;
}

extern "C" int dss_sdf2d_contacts_backward_grids(int npairs, int cap, const int *kind, const double *pose, const double *prm,
                                                 const double *scale, const int *grid_id, const DssSdf2dGrids *grids, const int *count,
                                                 const int *tag, const double *tpar, const double *gout, double *g_pose, double *g_prm,
                                                 double *g_scale, double *g_vals, double *g_grads, double *g_verts, void *stream)
{
    Args A;
    if (!make_args(A, npairs, cap, 0, kind, pose, prm, scale, grid_id, grids, 0.0)) return DSS_E_BADARG;
    if (A.G.ngrids > 0 && (!g_vals || !g_grads || !g_verts)) return DSS_E_BADARG;
    if (npairs == 0) return DSS_OK;
    if (!count || !tag || !tpar || !gout || !g_pose || !g_prm || !g_scale) return DSS_E_BADARG;
    hipLaunchKernelGGL(sdf2d_backward_kernel<true>, dim3(npairs), dim3(64), 0, (hipStream_t)stream, A, count, tag, tpar, gout, g_pose, g_prm,
                       g_scale, g_vals, g_grads, g_verts);
    return hipGetLastError() == hipSuccess ? DSS_OK : DSS_E_BADARG;
}
