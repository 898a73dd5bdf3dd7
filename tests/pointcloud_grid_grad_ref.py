"""Test reference (numpy, test infrastructure): the point-cloud loss of voxel-grid segments and its gradient with respect to the
samples, point by point in float64 (include/pointcloud_loss.h: dss_pointcloud_loss_grids' value, dss_pointcloud_loss_grids_adjoint).

    u = R(q)^T (x - pos) / scale          R normalised by 2 / (q.q); the point counts iff all |R^T (x - pos)| <= scale
    phi = scale * sum_c w_c(u) s[c]       the 8 corners of the cell of index position (u + 1)/2 (n - 1), clamped to [0, n - 2]
    loss_sum[seg] = sum phi^2             d loss_sum[seg] / d s[c] = sum 2 phi scale w_c

Every sample's sum is taken with math.fsum over its terms (correctly rounded), and the sum of the terms' magnitudes is returned
beside it: the scale of the rounding error of any other summation order.  Plain Python floats.  A single term is rounded as
float64 rounds it when the value is formed corner by corner (x slowest) and the factors are multiplied in the order 2, g_sum,
scale, phi, w -- where phi nearly cancels, another order of the 8 products would move a term by more than the summation does,
and the reference is there to isolate the summation.  tests/test_pointcloud_grid_grad_cpu.py holds it to torch autograd and to
central differences of its own loss.
"""
import math

import numpy as np

SHAPE_GRID = 7


def rotation(q):
    r, i, j, k = (float(v) for v in q)
    s = 2.0 / (r * r + i * i + j * j + k * k)
    return [[1.0 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
            [s * (i * j + k * r), 1.0 - s * (i * i + k * k), s * (j * k - i * r)],
            [s * (i * k - j * r), s * (j * k + i * r), 1.0 - s * (i * i + j * j)]]


def point(x, R, pos, scale, dims):
    """-> None for a point outside the query cube, else [(flat corner index, weight)] * 8."""
    d = [float(x[a]) - float(pos[a]) for a in range(3)]
    p = [R[0][a] * d[0] + R[1][a] * d[1] + R[2][a] * d[2] for a in range(3)]
    if not all(abs(v) <= scale for v in p):
        return None
    cell, frac = [], []
    for a in range(3):
        ind = (p[a] / scale + 1.0) * 0.5 * (dims[a] - 1)
        c = min(max(int(math.floor(ind)), 0), dims[a] - 2)
        cell.append(c); frac.append(ind - c)
    out = []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (frac[0] if dx else 1.0 - frac[0]) * (frac[1] if dy else 1.0 - frac[1]) * (frac[2] if dz else 1.0 - frac[2])
                out.append((((cell[0] + dx) * dims[1] + cell[1] + dy) * dims[2] + cell[2] + dz, w))
    return out


def loss_and_grad(pts, seg_off, pose, shape_type, prm, grid_id, grids, g_sum=None, keep=None):
    """grids: a list of [n0,n1,n2] float64 arrays.  -> dict(loss [nseg], count [nseg], grad: one array per grid (the gradient of
    sum_seg g_sum[seg] loss[seg]), abs_sum: likewise (sum of |term| per sample), terms: likewise (how many terms per sample)).
    Analytic segments and grid_id < 0 add nothing (their loss is reported as 0: not this reference's business).
    keep: a dict that receives the per-sample term lists (for tests that re-sum them)."""
    nseg = len(seg_off) - 1
    g_sum = np.ones(nseg) if g_sum is None else np.asarray(g_sum, np.float64)
    terms = [[[] for _ in range(g.size)] for g in grids]
    loss, count = np.zeros(nseg), np.zeros(nseg)
    for s in range(nseg):
        if int(shape_type[s]) != SHAPE_GRID or int(grid_id[s]) < 0:
            continue
        g = int(grid_id[s])
        flat, dims, scale = np.asarray(grids[g], np.float64).reshape(-1), grids[g].shape, float(prm[s][3])
        R, sq = rotation(pose[s][:4]), []
        for x in pts[seg_off[s]:seg_off[s + 1]]:
            c = point(x, R, pose[s][4:], scale, dims)
            if c is None:
                continue
            tri = 0.0
            for i, w in c:      # (the 8 products added in the corners' order, x slowest: the value's own float64 rounding)
                tri = tri + float(flat[i]) * w
            phi = tri * scale
            sq.append(phi * phi)
            for i, w in c:
                terms[g][i].append(2.0 * float(g_sum[s]) * scale * phi * w)
        loss[s], count[s] = math.fsum(sq), len(sq)
    if keep is not None:
        keep["terms"] = terms
    shape = lambda k, f: np.array([f(t) for t in terms[k]], np.float64).reshape(grids[k].shape)
    return dict(loss=loss, count=count, grad=[shape(k, math.fsum) for k in range(len(grids))],
                abs_sum=[shape(k, lambda t: math.fsum(abs(v) for v in t)) for k in range(len(grids))],
                terms=[shape(k, len) for k in range(len(grids))])
