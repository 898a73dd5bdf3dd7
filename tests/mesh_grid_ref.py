"""numpy float64 restatement of csrc/mesh_grid.hip, written differently from it, and the meshes its tests walk.

Distance of a point to a triangle: project the point onto the triangle's plane; where the foot lies inside (three same-signed
edge tests against the normal) the distance is the plane's, otherwise the least of the three segment distances.  (The kernel
classifies the point into Ericson's seven regions and takes the closest point's barycentric coordinates.)  Winding number: the
Van Oosterom-Strackee solid angle, 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|), summed over the faces
and divided by 4 pi.  phi = -dist where w > 1/2, else dist.

The tests' input conditions, asserted on this reference alone before the kernel's sign is demanded at every sample
(`conditions`): |phi| >= 1e-6 scale at every sample (no sample on the surface, where the sign is a rounding matter) and
|w - round(w)| <= 1e-6 (the mesh is closed as seen from every sample).

The value bound: |kernel - reference| <= 1e-12 scale per sample (BOUND), the bound of the project's other fp64 kernels against
numpy: both sides take tens of roundings of 2^-53 relative on coordinates of the size of the scale, in well-shaped triangles
(the barycentric solve's condition is 1 / sin^2 of the smallest angle, at most a few tens here).
"""
import functools

import numpy as np

BOUND = 1e-12
QUAT = (0.9, 0.3, -0.2, 0.1)      # the fixed non-trivial rotation (normalised below)


def rotation(q=QUAT):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _placed(v, f, q, at):
    v = np.asarray(v, np.float64)
    if q is not None:
        v = v @ rotation(q).T
    return v + np.asarray(at, np.float64), np.asarray(f, np.int64)


def box(dims=(1.0, 0.7, 0.5), q=QUAT, at=(0, 0, 0)):
    """12 faces, outward."""
    h = 0.5 * np.asarray(dims, np.float64)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h      # index 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # -x +x -y +y -z +z, outward
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return _placed(v, f, q, at)


def tetrahedron(r=0.5, q=QUAT, at=(0, 0, 0)):
    """4 faces, outward."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (r / np.sqrt(3.0))
    return _placed(v, [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], q, at)


def bipyramid(r=0.5, q=QUAT, at=(0, 0, 0)):
    """Triangular bipyramid: 6 faces, outward."""
    ring = [[np.cos(t), np.sin(t), 0.0] for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)]
    v = np.array(ring + [[0, 0, 0.8], [0, 0, -0.8]], np.float64) * r
    f = [(0, 1, 3), (1, 2, 3), (2, 0, 3), (1, 0, 4), (2, 1, 4), (0, 2, 4)]
    return _placed(v, f, q, at)


def octasphere(k=0, r=0.6, q=QUAT, at=(0, 0, 0)):
    """An octahedron subdivided k times, every vertex pushed to the sphere of radius r: 8 * 4^k faces, outward."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.asarray(x, np.float64) for x in v]
    for _ in range(k):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p)); mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return _placed(np.array(v) * r, f, q, at)


def concat(parts):
    """Disjoint components as one mesh."""
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + n); n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


_MAKERS = {512: lambda r, at: octasphere(3, r, at=at), 128: lambda r, at: octasphere(2, r, at=at), 32: lambda r, at: octasphere(1, r, at=at),
           12: lambda r, at: box((1.6 * r, 1.2 * r, 0.9 * r), at=at), 8: lambda r, at: octasphere(0, r, at=at),
           6: lambda r, at: bipyramid(r, at=at), 4: lambda r, at: tetrahedron(r, at=at)}
# where the small components go: the cube's corners, edge midpoints and face centres at 0.7 of its half side
_SPOTS = [np.array(p, np.float64) for n in (3, 2, 1) for p in
          [(a, b, c) for a in (-0.7, 0, 0.7) for b in (-0.7, 0, 0.7) for c in (-0.7, 0, 0.7)] if sum(x != 0 for x in p) == n]


def mesh_of(nf, scale=1.0):
    """A closed mesh of exactly nf faces (even, >= 4) inside the cube of half side `scale`: the largest maker that fits, of radius
    0.45 scale at the centre, and smaller ones of radius 0.1 scale at _SPOTS (0.7 scale from the centre planes) until the count is
    reached; all rotated by QUAT, all disjoint (0.45 + 0.1 < 0.7, 2 * 0.1 < 0.7)."""
    assert nf >= 4 and nf % 2 == 0
    sizes, left = [], nf
    while left:
        s = next(s for s in sorted(_MAKERS, reverse=True) if s <= left and left - s != 2)
        sizes.append(s); left -= s
    assert len(sizes) - 1 <= len(_SPOTS)
    parts = [_MAKERS[sizes[0]](0.45 * scale, (0, 0, 0))] + [_MAKERS[s](0.1 * scale, _SPOTS[i] * scale) for i, s in enumerate(sizes[1:])]
    v, f = concat(parts)
    assert len(f) == nf
    return v, f


def sample_points(dims, scale):
    """[n0,n1,n2,3]: sample (i, j, k) at scale * (-1 + 2 i / (n0 - 1), ...)."""
    ax = [scale * (-1.0 + 2.0 * np.arange(n) / (n - 1)) for n in dims]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=3)


def _dot(a, b):
    return (a * b).sum(-1)


def _segment(p, a, b):
    e = b - a
    t = np.clip(_dot(p - a, e) / _dot(e, e), 0.0, 1.0)
    return np.linalg.norm(p - a - t[..., None] * e, axis=-1)


def distance(p, verts, faces):
    """[N]: the distance of every point p [N,3] to the nearest triangle."""
    p = p[:, None, :]
    a, b, c = (verts[faces[:, i]][None] for i in range(3))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    t = _dot(p - a, n) / nn
    foot = p - t[..., None] * n
    inside = (_dot(np.cross(b - a, foot - a), n) >= 0) & (_dot(np.cross(c - b, foot - b), n) >= 0) & (_dot(np.cross(a - c, foot - c), n) >= 0)
    edges = np.minimum(np.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, c, a))
    return np.where(inside, np.abs(_dot(p - a, n)) / np.sqrt(nn), edges).min(1)


def winding(p, verts, faces):
    """[N]: the generalised winding number of the mesh about every point p [N,3], the faces summed in order."""
    p = p[:, None, :]
    a, b, c = (verts[faces[:, i]][None] - p for i in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return np.cumsum(2.0 * np.arctan2(num, den), axis=1)[:, -1] / (4.0 * np.pi)


def signed_distance(p, verts, faces):
    """-> (phi [N], w [N]) for points p [N,3]."""
    d, w = distance(p, verts, faces), winding(p, verts, faces)
    return np.where(w > 0.5, -d, d), w


def grid(verts, faces, dims, scale):
    """-> (samples [n0,n1,n2] = phi / scale, as the kernel stores them; w [n0,n1,n2])."""
    phi, w = signed_distance(sample_points(dims, scale).reshape(-1, 3), verts, faces)
    return (phi / scale).reshape(dims), w.reshape(dims)


def conditions(samples, w, scale=1.0):
    """The tests' input conditions on the reference (samples are phi / scale): -> (min |phi| / scale, max |w - round(w)|),
    asserted to be >= 1e-6 and <= 1e-6."""
    lo, off = float(np.abs(samples).min()), float(np.abs(w - np.round(w)).max())
    assert lo >= 1e-6 and off <= 1e-6, (lo, off)
    return lo, off


def box_sdf(p, dims):
    """The analytic distance of an axis-aligned box of full sizes dims centred at the origin."""
    q = np.abs(p) - 0.5 * np.asarray(dims, np.float64)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


MESHES = {"box": lambda: box(q=None), "box_rot": box, "octa0": lambda: octasphere(0), "octa2": lambda: octasphere(2), "octa3": lambda: octasphere(3)}


@functools.lru_cache(maxsize=None)
def case(kind, dims, scale):
    """(verts, faces, samples, min |phi| / scale, max |w - round(w)|) of a mesh of MESHES, or of mesh_of(int(kind), scale), on a
    grid, the conditions asserted; computed once per process and shared (not to be written to)."""
    v, f = MESHES[kind]() if kind in MESHES else mesh_of(int(kind), scale)
    g, w = grid(v, f, dims, scale)
    return (v, f, g) + conditions(g, w)
