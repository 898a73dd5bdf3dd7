"""Test helpers: the cases of the sample adjoint of the point-cloud loss (dss_pointcloud_loss_grids_adjoint), shared by
tests/test_pointcloud_grid_grad_cpu.py and tests/test_pointcloud_grid_grad_gpu.py, and a float64 torch restatement of the value.
"""
import numpy as np
import torch

SPHERE, GRID = 1, 7
EXACT_POSE = [2.0, 0.0, 0.0, 0.0, 0.25, -0.5, 1.0]      # a raw quaternion of norm 2 whose rotation is exactly the identity
EXACT_SCALE = 0.5                                        # with it u = (x - pos) / scale is exact for dyadic u


def _world(r, pose, scale, n, reach=1.1):
    """n points uniform in the body's cube stretched by `reach`, in the world frame of `pose`."""
    from pointcloud_grid_grad_ref import rotation
    p = (2.0 * r.random((n, 3)) - 1.0) * reach * scale
    return p @ np.array(rotation(pose[:4])).T + np.asarray(pose[4:])


def _exact(u):
    return np.asarray(EXACT_POSE[4:]) + EXACT_SCALE * np.asarray(u, np.float64).reshape(-1, 3)


def _case(segs, grids):
    """segs: (points [n,3], pose [7], type, scale, grid id, upstream weight)"""
    lens = [len(s[0]) for s in segs]
    prm = np.zeros((len(segs), 4))
    prm[:, 3] = [s[3] for s in segs]
    prm[[i for i, s in enumerate(segs) if s[2] == SPHERE], 0] = 0.4
    return dict(pts=np.concatenate([np.asarray(s[0], np.float64).reshape(-1, 3) for s in segs]), seg_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                pose=np.array([s[1] for s in segs], np.float64), shape_type=np.array([s[2] for s in segs], np.int32), prm=prm,
                grid_id=np.array([s[4] for s in segs], np.int32), g_sum=np.array([s[5] for s in segs], np.float64), grids=grids)


def mixed_case(seed=5):
    """One call with everything beside everything else.  Table: 2x3x5 (the least, not cubic), 3x3x3 that no segment uses, 5x4x3,
    9x9x9, 4x3x2.  Segment lengths 0, 1, 63, 64, 65, 2047, 2048, 2049 (a chunk is 2048 points, a wavefront 64).  Two segments share
    grid 0 under weights of different sign, and two grid 2, one of them under weight 0; an analytic segment (grid_id -1) stands
    between them; the poses of the random segments have raw quaternions of norm 0.6 - 1.7.  On the 9^3 grid, seen from a pose
    under which u is exact: 63 points with one, two or three |u_d| = 1 exactly (they count; the last cell is clamped, w = 1),
    1 point on a node, 64 points with some u_d = +-(1 + 2^-40) (outside: they add nothing), 65 points on nodes and cell faces.
    The last segment has 64 points (one full wavefront), all inside the cube, and the 4x3x2 grid to itself: its samples get
    64 x 8 terms from it and from nothing else."""
    r = np.random.default_rng(seed)
    grids = [r.standard_normal(s) for s in ((2, 3, 5), (3, 3, 3), (5, 4, 3), (9, 9, 9), (4, 3, 2))]
    pose = lambda: np.concatenate([r.standard_normal(4) * 0.6, r.standard_normal(3)])
    a, b, c, d = pose(), pose(), pose(), pose()
    # |u_d| = 1: a random sign pattern on 1 - 3 axes, the other coordinates on a 1/64 lattice
    lat = r.integers(-63, 64, (63, 3)) / 64.0
    for k in range(63):
        ax = r.permutation(3)[:1 + k % 3]
        lat[k, ax] = r.choice([-1.0, 1.0], len(ax))
    out = r.integers(-63, 64, (64, 3)) / 64.0
    for k in range(64):
        out[k, k % 3] = (1.0 + 2.0 ** -40) * (1.0 if k % 2 else -1.0)
    nodes = r.integers(0, 9, (65, 3)) / 4.0 - 1.0                 # nodes of the 9^3 grid ...
    nodes[33:, 1] = r.integers(-63, 64, 32) / 64.0                # ... and points on the faces / edges of its cells
    nodes[49:, 2] = r.integers(-63, 64, 16) / 64.0
    segs = [(_world(r, a, 0.8, 2049), a, GRID, 0.8, 0, 1.3),
            (_world(r, b, 1.7, 2047), b, GRID, 1.7, 0, -0.7),
            (_world(r, c, 1.1, 2048), c, GRID, 1.1, 2, 0.9),
            (_world(r, d, 1.1, 65), d, GRID, 1.1, 2, 0.0),
            (_world(r, d, 0.6, 64), d, SPHERE, 0.0, -1, 1.0),
            (_exact(lat), EXACT_POSE, GRID, EXACT_SCALE, 3, 1.1),
            (_exact([[0.25, -0.5, 0.75]]), EXACT_POSE, GRID, EXACT_SCALE, 3, -2.0),
            (np.zeros((0, 3)), EXACT_POSE, GRID, EXACT_SCALE, 3, 1.0),
            (_exact(out), EXACT_POSE, GRID, EXACT_SCALE, 3, 1.0),
            (_exact(nodes), EXACT_POSE, GRID, EXACT_SCALE, 3, 0.5),
            (_world(r, a, 1.3, 64, reach=0.95), a, GRID, 1.3, 4, -0.4)]
    return _case(segs, grids)


def one_cell_case(seed=6):
    """4096 points (two chunks) inside one cell of a 5x4x3 grid: every one of them adds to the same 8 samples."""
    r = np.random.default_rng(seed)
    grids = [r.standard_normal((5, 4, 3))]
    pose = np.concatenate([r.standard_normal(4), r.standard_normal(3)])
    from pointcloud_grid_grad_ref import rotation
    lo, hi = np.array([0.0, -1.0 / 3.0, 0.0]), np.array([0.5, 1.0 / 3.0, 1.0])      # cell (2, 1, 1)
    u = lo + (hi - lo) * (0.02 + 0.96 * r.random((4096, 3)))
    x = (u * 0.9) @ np.array(rotation(pose[:4])).T + pose[4:]
    return _case([(x, pose, GRID, 0.9, 0, 1.0)], grids)


def small_case(seed=7):
    """A few hundred points on 2x3x5 and 3x3x3, for checks that evaluate the reference many times."""
    r = np.random.default_rng(seed)
    grids = [r.standard_normal((2, 3, 5)), r.standard_normal((3, 3, 3))]
    pose = lambda: np.concatenate([r.standard_normal(4) * 0.8, r.standard_normal(3)])
    a, b, c = pose(), pose(), pose()
    return _case([(_world(r, a, 0.7, 150), a, GRID, 0.7, 0, 1.2), (_world(r, b, 1.2, 100), b, GRID, 1.2, 1, -0.6),
                  (_world(r, c, 0.9, 120), c, GRID, 0.9, 0, 0.8)], grids)


def torch_value(case, grids):
    """sum_seg g_sum[seg] loss_sum[seg] restated in float64 torch; grids: tensors (autograd reaches them).  Analytic segments are
    left out (they do not depend on the samples)."""
    total = 0.0
    off = case["seg_off"]
    for s in range(len(off) - 1):
        if case["shape_type"][s] != GRID or case["grid_id"][s] < 0 or off[s + 1] == off[s]:
            continue
        G = grids[case["grid_id"][s]]
        q, pos, scale = torch.tensor(case["pose"][s, :4]), torch.tensor(case["pose"][s, 4:]), float(case["prm"][s, 3])
        r, i, j, k = q
        ts = 2.0 / (q * q).sum()
        R = torch.stack([torch.stack([1 - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r)]),
                         torch.stack([ts * (i * j + k * r), 1 - ts * (i * i + k * k), ts * (j * k - i * r)]),
                         torch.stack([ts * (i * k - j * r), ts * (j * k + i * r), 1 - ts * (i * i + j * j)])])
        d = torch.tensor(case["pts"][off[s]:off[s + 1]]) - pos
        p = d[:, 0:1] * R[0] + d[:, 1:2] * R[1] + d[:, 2:3] * R[2]
        p = p[(p.abs() <= scale).all(1)]
        n = torch.tensor(G.shape, dtype=torch.float64)
        ind = (p / scale + 1.0) * 0.5 * (n - 1)
        c0 = torch.minimum(torch.clamp(torch.floor(ind), min=0.0), n - 2)
        f, c0 = ind - c0, c0.long()
        val = 0.0
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                    val = val + w * G[c0[:, 0] + dx, c0[:, 1] + dy, c0[:, 2] + dz]
        total = total + float(case["g_sum"][s]) * ((scale * val) ** 2).sum()
    return total
