"""numpy float64 reference of the chamfer distance (diffsdfsim_amd/chamfer.py, csrc/chamfer.hip) and the cases its tests share.

The definition of record: squared distances in the direct form ((a[:,None] - b[None]) ** 2).sum(-1), a block of rows at a time;
nearest neighbour = argmin (the first minimum); per scene mean_i min_j + mean_j min_i (pytorch3d.loss.chamfer_distance's
defaults); the gradient with the neighbours held fixed, the scattered part by np.add.at.

Bounds (derived from the arithmetic, none measured):
  d2       both sides sum three non-negative squares of once-rounded differences, contracted or not: at most 8 roundings each,
           so within 8 * 2^-53 relative of the exact value each and 2^-49 of each other -> D2_RTOL = 2^-48
  idx      equal to argmin wherever the two smallest distances of a row differ by more than 2^-40 relative (random_clouds
           asserts that they do, in every row and column), and equal to the LOWEST index of the minimum on the integer lattice,
           where every distance is exact
  value    |got - want| <= (N 2^-52 + 2^-48) want: any order of summing N non-negative terms, plus the terms' bound
  gradient a term 2 (a - b) / N is within 4 * 2^-53 relative; a point that is the nearest neighbour of k others sums k + 1
           terms: (k + 4) 2^-52 sum|terms| per component (grad returns it)
  parent   experiments.chamfer expands |a|^2 + |b|^2 - 2 a.b: 2^-44 max(|a_i|^2 + |b_j|^2), absolute (parent_bound)
"""
import numpy as np

D2_RTOL = 2.0 ** -48
GAP = 2.0 ** -40
SHIFT = np.array([1e3, -2e3, 5e2])


def dist2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    return ((a[:, None] - b[None]) ** 2).sum(-1)


def nn(q, r, chunk=1024):
    """(d2 [Nq], idx [Nq]) of q's points in r: row minima and first argmin of the direct form; +inf and -1 where r is empty."""
    q, r = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1, 3)
    d2, idx = np.full(len(q), np.inf), np.full(len(q), -1, np.int64)
    if len(r):
        for i in range(0, len(q), chunk):
            d = dist2(q[i:i + chunk], r)
            idx[i:i + chunk] = d.argmin(1)
            d2[i:i + chunk] = d[np.arange(d.shape[0]), idx[i:i + chunk]]
    return d2, idx


def nn_segments(q, q_off, r, r_off):
    """nn per segment; idx is the row in the packed r."""
    d2, idx = np.zeros(len(q)), np.full(len(q), -1, np.int64)
    for s in range(len(q_off) - 1):
        d, i = nn(q[q_off[s]:q_off[s + 1]], r[r_off[s]:r_off[s + 1]])
        d2[q_off[s]:q_off[s + 1]] = d
        idx[q_off[s]:q_off[s + 1]] = np.where(i >= 0, i + r_off[s], -1)
    return d2, idx


def value(a, b):
    if len(a) == 0 or len(b) == 0:
        return np.nan
    return nn(a, b)[0].mean() + nn(b, a)[0].mean()


def grad(a, b):
    """d value / d a, d value / d b with the neighbours held fixed, and the bound of each component -> (ga, gb, bound_a, bound_b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ga, gb, abs_a, abs_b = np.zeros_like(a), np.zeros_like(b), np.zeros_like(a), np.zeros_like(b)
    k_a, k_b = np.zeros(len(a)), np.zeros(len(b))
    for x, y, gx, gy, ax, ay, ky in ((a, b, ga, gb, abs_a, abs_b, k_b), (b, a, gb, ga, abs_b, abs_a, k_a)):
        j = nn(x, y)[1]
        t = 2.0 * (x - y[j]) / len(x)
        gx += t; ax += np.abs(t)
        np.add.at(gy, j, -t); np.add.at(ay, j, np.abs(t)); np.add.at(ky, j, 1.0)
    return ga, gb, (k_a[:, None] + 4) * 2.0 ** -52 * abs_a, (k_b[:, None] + 4) * 2.0 ** -52 * abs_b


def value_bound(want, n):
    return (n * 2.0 ** -52 + D2_RTOL) * want


def parent_bound(a, b):
    return 2.0 ** -44 * ((np.asarray(a) ** 2).sum(-1).max() + (np.asarray(b) ** 2).sum(-1).max())


def assert_gaps(q, r):
    """In every row and every column of the distance matrix the two smallest entries differ by more than GAP relative."""
    if len(q) == 0 or len(r) == 0:
        return
    d = dist2(q, r)
    for m in (d, d.T):
        if m.shape[1] > 1:
            two = np.partition(m, 1, axis=1)[:, :2]
            assert np.all(two[:, 1] - two[:, 0] > GAP * two[:, 1]), "a near-tie in a random case: pick another seed"


def random_clouds(q_lens, r_lens, seed, shift=None):
    """Packed uniform clouds in [-1, 1]^3 (+ shift) with the given segment lengths -> (q, q_off, r, r_off); gaps asserted."""
    rng = np.random.default_rng(seed)
    q_off, r_off = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(r_lens)]).astype(np.int64)
    q, r = rng.uniform(-1, 1, (q_off[-1], 3)), rng.uniform(-1, 1, (r_off[-1], 3))
    if shift is not None:
        q, r = q + shift, r + shift
    for s in range(len(q_lens)):
        assert_gaps(q[q_off[s]:q_off[s + 1]], r[r_off[s]:r_off[s + 1]])
    return q, q_off, r, r_off


def lattice_clouds(nq, nr, seed):
    """Integer coordinates in [-3, 3] (343 distinct points, so both clouds repeat points once they are longer): every distance
    is exact and ties are everywhere, within a tile, across tiles and across splits."""
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (nq, 3)).astype(np.float64), rng.integers(-3, 4, (nr, 3)).astype(np.float64)


def segment_cases(Q, T):
    """Segment lengths (query, reference) that cross every boundary of the launch: a wavefront (63, 64, 65), the queries of a
    workgroup Q, the tile T; each of 9 segments with an empty query segment, an empty reference segment and a one-point pair in
    the middle.  'direct': at most 2 tiles, one split; 'split': 2 tiles + 3 and 3 tiles + 1, the partials are merged."""
    direct = [(1, 65), (63, T - 1), (64, T), (0, 64), (1, 1), (65, 0), (Q - 1, T + 1), (Q, 2 * T), (Q + 1, 63)]
    split = [(1, 65), (63, T - 1), (64, 3 * T + 1), (0, 64), (1, 1), (65, 0), (Q - 1, T + 1), (Q, 2 * T + 3), (Q + 1, 63)]
    return dict(direct=direct, split=split)


def check_nn(d2, idx, q, q_off, r, r_off, exact=False):
    """d2 / idx of the code under test against nn_segments: idx equal everywhere; d2 equal (exact) or within D2_RTOL relative."""
    wd, wi = nn_segments(q, q_off, r, r_off)
    assert np.array_equal(np.asarray(idx, np.int64), wi), "idx differs at %s" % np.nonzero(np.asarray(idx) != wi)[0][:8]
    fin = np.isfinite(wd)
    assert np.array_equal(np.asarray(d2)[~fin], wd[~fin])
    err = np.abs(np.asarray(d2)[fin] - wd[fin])
    print("chamfer nn: %d queries, worst d2 error / bound %.3g" % (len(wd), (err / np.maximum(D2_RTOL * wd[fin], 1e-300)).max() if fin.any() else 0.0))
    assert np.all(err <= (0.0 if exact else D2_RTOL) * wd[fin])
