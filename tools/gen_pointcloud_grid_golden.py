"""Generate tests/golden/pointcloud_loss_grid.npz: the point-cloud loss of the reference for voxel-grid bodies, on the CPU.

    python tools/gen_pointcloud_grid_golden.py      (needs the reference checkout that oracle/refshim imports)
The arithmetic of `match_pointcloud` (experiments/trajectory_fitting/optim_pointcloud.py:166-201) as in
tools/gen_pointcloud_golden.py, with the reference's own SDFGrid3D as the body: `grid_interp` is the documented stand-in of
oracle/refshim (plain trilinear interpolation), the value's derivative w.r.t. the point is DiffGridSDF's (the normalised
interpolated central-difference field).  Two grids (tests/grid_ref.py: the 33 x 25 x 21 torus and the 12^3 off-centre sphere) and
two analytic segments in between; per segment out [12] = (sum, count, d / d pose [7], d / d prm [3] = 0) and abs_sum [12], the sums
of the absolute per-point terms.  The generator asserts that every point keeps 1e-6 from the faces of its query cube and that the
interpolated central-difference field is longer than 1e-3 at every point inside (so the normalisation is away from its clamp).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pointcloud_golden as base  # noqa: E402  (installs oracle/refshim)
import grid_ref  # noqa: E402
from pytorch3d.transforms import quaternion_to_matrix  # noqa: E402
from sdf_physics.physics3d.bodies import SDFGrid3D  # noqa: E402

GRID = 7


def central_field(grid, scale, p):
    """The interpolated central-difference field (zero on the boundary layers) at body-frame points p, as grid_sdf_grad forms it."""
    g = np.zeros((3,) + grid.shape)
    g[0, 1:-1] = (grid[2:] - grid[:-2]) / 2
    g[1, :, 1:-1] = (grid[:, 2:] - grid[:, :-2]) / 2
    g[2, :, :, 1:-1] = (grid[:, :, 2:] - grid[:, :, :-2]) / 2
    return np.stack([grid_ref.field(g[k], 1.0, p / scale) for k in range(3)], -1)


def grid_points(r, n, grid, scale, pose, where="mixed"):
    """n world-frame points: near the zero level, anywhere in the cube, a fifth outside it ('outside': all of them)."""
    R = base.rot(pose[:4])
    out = []
    while len(out) < n:
        u = r.random()
        if where == "outside" or (where == "mixed" and u < 0.2):
            p = r.uniform(-1.4 * scale, 1.4 * scale, 3)
            p[r.integers(3)] = r.choice([-1.0, 1.0]) * scale * r.uniform(1.02, 1.5)
        else:
            p = r.uniform(-0.98 * scale, 0.98 * scale, 3)
            if u > 0.6 and abs(grid_ref.field(grid, scale, p)) > 0.15 * scale:      # most of them near the surface
                continue
        x = R @ p + pose[4:]
        pb = R.T @ (x - pose[4:])
        inside = np.all(np.abs(pb) < scale)
        if np.all(np.abs(np.abs(pb) - scale) > 1e-5) and (not inside or np.linalg.norm(central_field(grid, scale, pb)) > 2e-3):
            out.append(x)
    return np.array(out).reshape(n, 3)


def reference_terms(grid, scale, pose, pts):
    """(out [12], abs_sum [12]) of one grid segment from the reference's SDFGrid3D, float64 on the CPU."""
    q = torch.tensor(pose[:4], dtype=torch.double, requires_grad=True)
    pos = torch.tensor(pose[4:], dtype=torch.double, requires_grad=True)
    body = SDFGrid3D([0, 0, 0], scale, torch.tensor(grid, dtype=torch.double))

    def loss(x):
        p = (quaternion_to_matrix(q).T.unsqueeze(0) @ (x - pos).unsqueeze(-1)).squeeze(-1)
        pd = p.detach().numpy()
        assert np.all(np.abs(np.abs(pd) - scale) > 1e-6), "a point within 1e-6 of the query cube's face"
        inside = np.all(np.abs(pd) <= scale, axis=1)
        assert not inside.any() or np.linalg.norm(central_field(grid, scale, pd[inside]), axis=1).min() > 1e-3, "a vanishing gradient field"
        sdf, mask = body.query_sdfs(p, return_grads=False, return_overlapmask=True)
        sdf[mask == False] = 0      # noqa: E712  (as the experiment writes it)
        return torch.sum(sdf ** 2), int(mask.sum())

    out, abs_sum = np.zeros(12), np.zeros(12)
    if len(pts) == 0:
        return out, abs_sum
    x = torch.tensor(pts, dtype=torch.double)
    total, count = loss(x)
    out[0], out[1] = float(total), count
    if count:
        out[2:9] = torch.cat(torch.autograd.grad(total, [q, pos], retain_graph=True)).numpy()
    per_point = np.zeros(12)
    for i in range(len(pts)):
        li, ci = loss(x[i:i + 1])
        if ci == 0:
            continue
        gi = torch.cat(torch.autograd.grad(li, [q, pos])).numpy()
        t = np.concatenate([[float(li), 1.0], gi, np.zeros(3)])
        abs_sum += np.abs(t)
        per_point += t
    assert np.all(np.abs(per_point - out) <= 1e-12 * abs_sum + 1e-300), (per_point, out)
    return out, abs_sum


def main():
    r = np.random.default_rng(2025)
    A, B = grid_ref.torus_grid(), grid_ref.sphere_grid()
    sa, sb = 0.9, 1.3

    def pose(norm=1.0):
        q = r.standard_normal(4)
        return np.concatenate([norm * q / np.linalg.norm(q), r.uniform(-2.0, 2.0, 3)])
    # (name, kind, prm4, grid id, pose, n points, where)
    segs = [("empty", GRID, [0, 0, 0, sa], 0, pose(), 0, "mixed"),
            ("one_point", GRID, [0, 0, 0, sa], 0, pose(), 1, "inside"),
            ("box", base.BOX, [0.9, 1.1, 1.3, 0], -1, pose(), 300, "mixed"),
            ("all_outside", GRID, [0, 0, 0, sb], 1, pose(), 50, "outside"),
            ("torus_257", GRID, [0, 0, 0, sa], 0, pose(), 257, "mixed"),
            ("rounded", base.ROUNDED, [1.2, 1.0, 0.8, 0.2], -1, pose(), 200, "mixed"),
            ("sphere_4133", GRID, [0, 0, 0, sb], 1, pose(), 4096 + 37, "mixed"),
            ("torus_nonunit_quat", GRID, [0, 0, 0, sa], 0, pose(1.3), 300, "mixed")]
    grids = [A, B]
    pts, off, outs, sums = [], [0], [], []
    for name, kind, prm4, gid, ps, n, where in segs:
        prm4 = np.asarray(prm4, np.float64)
        if kind == GRID:
            x = grid_points(r, n, grids[gid], prm4[3], ps, where)
            o, a = reference_terms(grids[gid], float(prm4[3]), ps, x)
        else:
            x = base.segment_points(r, n, kind, prm4, ps, where)
            o, a = base.reference_terms(kind, prm4, ps, x)
        print("%-20s n %5d inside %5d  sum %.6e  |d/dpos| %.3e" % (name, n, int(o[1]), o[0], np.abs(o[6:9]).max()))
        pts.append(x); off.append(off[-1] + n); outs.append(o); sums.append(a)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pointcloud_loss_grid.npz"),
                        names=np.array([s[0] for s in segs]), shape_type=np.array([s[1] for s in segs], np.int32),
                        prm=np.array([s[2] for s in segs], np.float64), grid_id=np.array([s[3] for s in segs], np.int32),
                        pose=np.array([s[4] for s in segs]), pts=np.concatenate(pts), seg_off=np.array(off, np.int32),
                        out=np.array(outs), abs_sum=np.array(sums), grid_0=A, grid_1=B)


if __name__ == "__main__":
    main()
