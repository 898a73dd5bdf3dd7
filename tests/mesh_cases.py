"""Closed triangle meshes for the mesh-chain tests (marching cubes -> MeshSDF backward -> mesh inertia and its backward).

Plain numpy, deterministic from fixed seeds: the golden generator (oracle/gen/gen_mesh_chain_golden.py) and the tests
build the same meshes from here, so no mesh is stored.  Face counts straddle the launch boundaries of
csrc/sdf_mesh.hip: the 256-face stride of one workgroup (254 / 256 / 258) and the 32-workgroup cap of the backward,
past which its stride loop takes a second trip (8190 / 8192 / 8194).  A closed triangle mesh has an even face count.
"""
import fractions

import numpy as np

from diffsdfsim_amd import meshes

SHIFT = np.array([0.05, -0.02, 0.03])
FULL_GRAD_MAX_FACES = 1280      # the golden stores the whole vertex gradient up to here, 512 rows of it beyond
N_STORED = 512


def bipyramid(n, seed):
    """Irregular closed bipyramid over an n-gon: verts [n + 2, 3] (ring, top apex n, bottom apex n + 1),
    faces [2 n, 3] oriented outwards.  Each apex belongs to n faces."""
    r = np.random.default_rng(seed)
    th = np.sort(r.uniform(0.0, 2.0 * np.pi, n))
    rad = r.uniform(0.4, 0.9, n)
    z = r.uniform(-0.1, 0.1, n)
    ring = np.stack([rad * np.cos(th), rad * np.sin(th), z], 1)
    v = np.concatenate([ring, [[0.03, -0.02, 0.7]], [[-0.02, 0.04, -0.6]]]) + SHIFT
    i = np.arange(n); j = (i + 1) % n
    f = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)])
    return v, f.astype(np.int64)


def tetra():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.3, 0.8]]) + SHIFT
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)
    return v, f


def stretched_icosphere(sub):
    v, f = meshes.icosphere(sub)
    return v * np.array([0.7, 0.5, 0.9]) + SHIFT, f


def with_orphan(v, f):
    """The same mesh plus one vertex that no face uses (last row)."""
    return np.concatenate([v, [[0.3, 0.2, -0.1]]]), f


# name -> (builder, mass); masses are distinct
_CASES = {
    "tetra": (tetra, 0.9),
    "ico2": (lambda: stretched_icosphere(2), 1.7),
    "ico2_orphan": (lambda: with_orphan(*stretched_icosphere(2)), 1.3),
    "bipyr254": (lambda: bipyramid(127, 11), 2.1),
    "bipyr256": (lambda: bipyramid(128, 12), 2.3),
    "bipyr258": (lambda: bipyramid(129, 13), 2.9),
    "ico4": (lambda: meshes.icosphere(4), 3.1),
    "bipyr8190": (lambda: bipyramid(4095, 14), 3.7),
    "bipyr8192": (lambda: bipyramid(4096, 15), 4.1),
    "bipyr8194": (lambda: bipyramid(4097, 16), 4.3),
}
NAMES = list(_CASES)


def case(name):
    """-> verts [V,3] float64, faces [F,3] int64, mass, gJ [3,3] (seeded, non-symmetric)."""
    build, mass = _CASES[name]
    v, f = build()
    gJ = np.random.default_rng(1000 + NAMES.index(name)).standard_normal((3, 3))
    return np.ascontiguousarray(v), f, mass, gJ


def stored_rows(name, v, f):
    """Vertex rows at which the golden keeps the gradient: all of them for a small mesh; for a large one N_STORED
    seeded rows that always include the two apexes of a bipyramid (its last two vertices)."""
    if len(f) <= FULL_GRAD_MAX_FACES:
        return np.arange(len(v))
    r = np.random.default_rng(2000 + NAMES.index(name))
    idx = r.choice(len(v) - 2, N_STORED - 2, replace=False)
    return np.sort(np.concatenate([idx, [len(v) - 2, len(v) - 1]]))


def exact_volume(v, f):
    """Volume by signed tetrahedra against the origin, in exact rational arithmetic on the float64 coordinates,
    rounded once."""
    F = [[fractions.Fraction(float(x)) for x in row] for row in v]
    tot = fractions.Fraction(0)
    for a, b, c in f:
        A, B, C = F[a], F[b], F[c]
        tot += (A[0] * (B[1] * C[2] - B[2] * C[1]) - A[1] * (B[0] * C[2] - B[2] * C[0]) + A[2] * (B[0] * C[1] - B[1] * C[0]))
    return float(tot / 6)


# ---- MeshSDF backward -------------------------------------------------------------------------------------------------
SDF_TYPES = {"box": 0, "sphere": 1, "cylinder": 2, "rounded": 3, "brick": 4, "bowl": 5}
PREFIXES = (1, 255, 256, 257, 600)
N_SUBSET = 600
KINK_MARGIN = 1e-3


def kink_distance(name, unit_prm, v):
    """Distance of unit-frame points v [n,3] to the nearest kink of the type's SDF: the planes / cylinders on which
    the SDF or its normal switches branch (box edge planes |q_i| = |q_j| and q_i = 0 outside, cylinder rim, bowl lip)."""
    p = np.asarray(unit_prm, np.float64).reshape(-1)
    a = np.abs(v)
    inf = np.full(len(v), np.inf)
    if name == "sphere":
        return inf
    if name in ("box", "rounded"):
        hd = (p[:3] - (2.0 * p[3] if name == "rounded" else 0.0)) / 2.0
        q = a - hd
        return _box_kinks(q)
    if name == "cylinder":
        q = np.stack([np.hypot(v[:, 0], v[:, 1]) - p[0], a[:, 2] - p[1] / 2.0], 1)
        return _box_kinks(q)
    if name == "brick":
        hd = p[:3] / 2.0; hd[:2] -= p[3]
        q = a - hd
        s01 = np.linalg.norm(np.maximum(q[:, :2], 0), axis=1) + np.minimum(q[:, :2].max(1), 0) - p[3]
        return np.minimum(_box_kinks(q[:, :2]), _box_kinks(np.stack([s01, q[:, 2]], 1)))
    if name == "bowl":
        z = v[:, 2] - p[0] / 2.0
        return np.minimum(np.abs(z), np.abs(z - p[0] / 2.0))
    raise KeyError(name)


def _box_kinks(q):
    """q [n,k]: the box-type SDF max(q, 0).norm() + min(max(q), 0) and its failsafe normal switch branch where the two
    largest components tie (inside) and where the second largest crosses zero (a face meets an edge region).  The
    largest component crossing zero alone is no kink: value and normal are the same on both sides (a flat face)."""
    s = np.sort(q, axis=1)
    return np.minimum(np.abs(s[:, -2]), s[:, -1] - s[:, -2])


def gbar_field(rows, seed):
    """Seeded cotangent on `rows` vertices, on a 2^-10 lattice (it compresses well in the golden file)."""
    return np.round(np.random.default_rng(seed).standard_normal((rows, 3)) * 1024.0) / 1024.0


# ---- marching-cubes fields --------------------------------------------------------------------------------------------
NOISE_SHAPES = ((16, 16, 16), (16, 16, 17), (17, 17, 17), (5, 7, 351))     # one full scan chunk of 4096, two, two, three


def noise(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape)


def lattice_field(shape=(9, 10, 11), seed=5):
    """Integer values in {-2 .. 2}: exact zeros at grid points (0 < 0 is false: a zero sample is outside)."""
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float64)


def cube_case_field(case, seed=0):
    """2 x 2 x 2 grid with corner c = cx + 2 cy + 4 cz inside (negative) iff bit c of `case`, seeded magnitudes."""
    mag = np.random.default_rng(seed + case).uniform(0.5, 1.5, (2, 2, 2))
    c = np.arange(2)
    inside = (case >> (c[:, None, None] + 2 * c[None, :, None] + 4 * c[None, None, :])) & 1
    return np.where(inside == 1, -mag, mag)


def triangles_point_outwards(phi, v, f, iso=0.0):
    """Every vertex of a triangle lies on a grid edge with one end inside and one outside.  True iff for every triangle
    the normal has a positive dot product with the sum, over its three vertices, of the edge direction taken from the
    inside end to the outside end.  (The centroid of all inside corners to the centroid of all outside corners is no
    usable direction: it vanishes for 16 of the 256 cube cases and points the wrong way for one sheet of most
    two-sheet cases.)"""
    inside = phi < iso
    for tri in f:
        P = v[tri]
        n = np.cross(P[1] - P[0], P[2] - P[0])
        d = np.zeros(3)
        for a, b in zip(np.floor(P).astype(int), np.ceil(P).astype(int)):
            if inside[tuple(a)] == inside[tuple(b)]:
                return False
            d += (b - a) if inside[tuple(a)] else (a - b)
        if not n @ d > 0.0:
            return False
    return True


def sparse_sign_field(n2, cuts=3000, seed=9):
    """2 x 2 x n2 field, positive except for seeded short runs along the long axis: a few thousand cut edges spread over
    every scan chunk, non-trivial magnitudes."""
    r = np.random.default_rng(seed)
    phi = r.uniform(0.5, 1.5, (2, 2, n2))
    k = np.unique(np.concatenate([r.integers(1, n2 - 1, cuts // 4), [1, 4095, 4096, n2 - 2]]))
    for (i, j) in ((0, 0), (1, 0), (1, 1)):
        kk = k[r.random(len(k)) < 0.6]
        phi[i, j, kk] *= -1.0
    return phi


# ---- voxel-grid query --------------------------------------------------------------------------------------------------
def grid_query_case():
    """3 x 5 x 4 grid of small integers (three different extents: a swapped n1 / n2 reads other samples) and points at
    dyadic fractions of scale = 1: nodes, the last node of each axis, +-scale exactly, and just outside."""
    G = np.random.default_rng(21).integers(-4, 5, (3, 5, 4)).astype(np.float64)
    r = np.random.default_rng(22)
    pts = [r.integers(-8, 9, (40, 3)) / 8.0,
           np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [1.0, -1.0, 0.5], [0.0, 0.5, 1.0], [-1.0, 0.0, 0.25],
                     [0.0, 0.0, 0.0], [1.0, 0.5, -1.0], [-0.5, 1.0, 1.0]]),
           np.array([[np.nextafter(1.0, 2.0), 0.0, 0.0], [0.0, -np.nextafter(1.0, 2.0), 0.0], [0.0, 0.0, 1.125], [-2.0, 0.5, 0.5]])]
    return G, 1.0, np.concatenate(pts)


def _cell(G, p, cast):
    idx, w = [], []
    for d in range(3):
        n = G.shape[d]
        ind = (cast(p[d]) + 1) * cast(n - 1) / 2
        c = min(max(int(np.floor(float(ind))), 0), n - 2)
        idx.append(c); w.append(ind - c)
    return idx, w


def grid_value_exact(G, pts):
    """Trilinear value at pts (scale 1) in exact rational arithmetic -> list of Fractions (None outside the unit cube)."""
    Fr = fractions.Fraction
    out = []
    for p in pts:
        if np.abs(p).max() > 1.0:
            out.append(None); continue
        (i, j, k), w = _cell(G, [Fr(float(x)) for x in p], Fr)
        acc = Fr(0)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    wt = (w[0] if dx else 1 - w[0]) * (w[1] if dy else 1 - w[1]) * (w[2] if dz else 1 - w[2])
                    acc += Fr(float(G[i + dx, j + dy, k + dz])) * wt
        out.append(acc)
    return out


def grid_grad_longdouble(G, pts):
    """The gradient as the comment above grid_sdf_query_kernel states it, in numpy.longdouble: the central-difference field
    (zero in the boundary layers) interpolated trilinearly, normalised twice with the 1e-12 clamp; zero outside."""
    L = np.longdouble
    C = np.zeros(G.shape + (3,), L)
    C[1:-1, :, :, 0] = (G[2:].astype(L) - G[:-2]) / 2
    C[:, 1:-1, :, 1] = (G[:, 2:].astype(L) - G[:, :-2]) / 2
    C[:, :, 1:-1, 2] = (G[:, :, 2:].astype(L) - G[:, :, :-2]) / 2
    out = np.zeros((len(pts), 3), L)
    for t, p in enumerate(pts):
        if np.abs(p).max() > 1.0:
            continue
        (i, j, k), w = _cell(G, [L(x) for x in p], L)
        g = np.zeros(3, L)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    wt = (w[0] if dx else 1 - w[0]) * (w[1] if dy else 1 - w[1]) * (w[2] if dz else 1 - w[2])
                    g += C[i + dx, j + dy, k + dz] * wt
        for _ in range(2):
            g = g / max(np.sqrt((g * g).sum()), L(1e-12))
        out[t] = g
    return out
