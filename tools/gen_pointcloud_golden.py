"""Generate tests/golden/pointcloud_loss.npz: the point-cloud loss of the reference on the CPU, value and gradient.

    python tools/gen_pointcloud_golden.py      (needs the reference checkout that oracle/refshim imports)
For every segment of one batch (the inputs of tests/test_pointcloud_loss_gpu.py, stored in the file) the arithmetic of
`match_pointcloud` (experiments/trajectory_fitting/optim_pointcloud.py:166-201): points into the body frame with
quaternion_to_matrix(q)^T, `query_sdfs(..., return_grads=False, return_overlapmask=True)` of the reference body built from the
segment's parameters, values outside the query cube set to zero, sum of squares -- and its autograd gradient w.r.t. the pose
(raw quaternion + position) and the three shape parameters.  Stored per segment: out [12] = (sum, count, d / d pose [7],
d / d prm [3]) and abs_sum [12], the sums of the absolute per-point terms (each point differentiated on its own), which is the
scale the tests' tolerance refers to.  One exception, sphere segments' four quaternion outputs: see reference_terms.  The generator checks that no point lies within 1e-6 of a face of its query cube.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

refshim.install()
from pytorch3d.transforms import quaternion_to_matrix  # noqa: E402
from sdf_physics.physics3d.bodies import SDFBowl, SDFBox, SDFBoxRounded, SDFBrick, SDFCylinder, SDFSphere  # noqa: E402

BOX, SPHERE, CYLINDER, ROUNDED, BRICK, BOWL = range(6)


def body_of(kind, prm, r):
    """The reference body of a segment and its scale; prm: tensor [3] that requires grad."""
    z = [0, 0, 0]
    if kind == BOX:
        return SDFBox(z, prm, custom_mesh=True, custom_inertia=True)
    if kind == SPHERE:
        return SDFSphere(z, prm[0], custom_mesh=True, custom_inertia=True)
    if kind == CYLINDER:
        return SDFCylinder(z, prm[0], prm[1], custom_mesh=True, custom_inertia=True)
    if kind == ROUNDED:
        return SDFBoxRounded(z, prm, r)
    if kind == BRICK:
        return SDFBrick(z, prm, r)
    return SDFBowl(z, prm[0], prm[1], custom_mesh=True)


def scale_of(kind, prm):
    if kind == SPHERE:
        return 1.5 * prm[0]
    if kind == CYLINDER:
        return 1.5 * max(prm[0], prm[1] / 2)
    if kind == BOWL:
        return (prm[0] + prm[1]) * 1.3333
    return 1.5 * max(prm[:3]) / 2


def rot(q):
    return quaternion_to_matrix(torch.tensor(q, dtype=torch.double)).numpy()


def segment_points(r, n, kind, prm, pose, where="mixed"):
    """n world-frame points whose body-frame images keep 1e-6 from the faces of the query cube: near the surface, anywhere
    in the cube, and a fifth outside it (where='outside': all of them outside)."""
    s = scale_of(kind, prm)
    R = rot(pose[:4])
    out = []
    while len(out) < n:
        u = r.random()
        if where == "outside" or (where == "mixed" and u < 0.2):
            p = r.uniform(-1.4 * s, 1.4 * s, 3)
            p[r.integers(3)] = r.choice([-1.0, 1.0]) * s * r.uniform(1.02, 1.5)
        elif u < 0.6:
            p = r.uniform(-0.98 * s, 0.98 * s, 3)
        else:        # around the body: its extent times 0.6 .. 1.3 per axis
            ext = {SPHERE: [prm[0]] * 3, CYLINDER: [prm[0], prm[0], prm[1] / 2], BOWL: [prm[0]] * 3}.get(kind, [d / 2 for d in prm[:3]])
            p = np.array([e * r.uniform(0.6, 1.3) * r.choice([-1.0, 1.0]) for e in ext])
            p = np.clip(p, -0.98 * s, 0.98 * s)
        x = R @ p + pose[4:]
        pb = R.T @ (x - pose[4:])
        if np.all(np.abs(np.abs(pb) - s) > 1e-5):
            out.append(x)
    return np.array(out).reshape(n, 3)


def reference_terms(kind, prm4, pose, pts):
    """(out [12], abs_sum [12]) of one segment from the reference body, float64 on the CPU."""
    q = torch.tensor(pose[:4], dtype=torch.double, requires_grad=True)
    pos = torch.tensor(pose[4:], dtype=torch.double, requires_grad=True)
    prm = torch.tensor(prm4[:3], dtype=torch.double, requires_grad=True)
    body = body_of(kind, prm, float(prm4[3]))
    scale = float(body.scale)
    assert abs(scale - scale_of(kind, prm4)) < 1e-12

    def loss(x):
        p = (quaternion_to_matrix(q).T.unsqueeze(0) @ (x - pos).unsqueeze(-1)).squeeze(-1)
        assert bool((torch.abs(torch.abs(p.detach()) - scale) > 1e-6).all()), "a point within 1e-6 of the query cube's face"
        sdf, mask = body.query_sdfs(p, return_grads=False, return_overlapmask=True)
        sdf[mask == False] = 0      # noqa: E712  (as the experiment writes it)
        return torch.sum(sdf ** 2), int(mask.sum())

    out, abs_sum = np.zeros(12), np.zeros(12)
    if len(pts) == 0:
        return out, abs_sum
    x = torch.tensor(pts, dtype=torch.double)
    total, count = loss(x)
    g = torch.autograd.grad(total, [q, pos, prm], retain_graph=True, allow_unused=True)
    g = [torch.zeros(n) if t is None else t for t, n in zip(g, (4, 3, 3))]
    out[0], out[1] = float(total), count
    out[2:] = torch.cat(g).numpy()
    per_point = np.zeros(12)
    for i in range(len(pts)):
        li, ci = loss(x[i:i + 1])
        if ci == 0:
            continue
        gi = torch.autograd.grad(li, [q, pos, prm], retain_graph=True, allow_unused=True)
        gi = torch.cat([torch.zeros(n, dtype=torch.double) if t is None else t for t, n in zip(gi, (4, 3, 3))]).numpy()
        t = np.concatenate([[float(li), 1.0], gi])
        abs_sum += np.abs(t)
        per_point += t
    if kind == SPHERE and count:
        # A sphere's SDF does not depend on the rotation: each point's quaternion term is exactly zero in exact arithmetic and the
        # reference's autograd returns rounding noise of the size of the summands of sum_i (d phi^2 / d p_i) (d p_i / d q_k),
        # which no multiple of the (vanishing) per-point result bounds.  For a sphere segment's four quaternion outputs, and for
        # those alone, abs_sum adds up the absolute summands of that contraction, the numbers that are actually rounded.
        p_leaf = (quaternion_to_matrix(q).T.unsqueeze(0) @ (x - pos).unsqueeze(-1)).squeeze(-1).detach().requires_grad_()
        sdf, mask = body.query_sdfs(p_leaf, return_grads=False, return_overlapmask=True)
        gp = torch.autograd.grad(torch.sum(sdf[mask] ** 2), p_leaf, retain_graph=True)[0]
        J = torch.autograd.functional.jacobian(lambda qq: (quaternion_to_matrix(qq).T.unsqueeze(0) @ (x - pos.detach()).unsqueeze(-1)).squeeze(-1), q.detach())
        abs_sum[2:6] = (gp.abs()[:, :, None] * J.abs()).sum(dim=(0, 1)).numpy()
    # the reference's own summation agrees with the point-by-point sum to the bound the tests use
    assert np.all(np.abs(per_point - out) <= 1e-12 * abs_sum + 1e-300), (per_point, out)
    return out, abs_sum


def main():
    r = np.random.default_rng(2024)

    def unit_quat(norm=1.0):
        q = r.standard_normal(4)
        return norm * q / np.linalg.norm(q)
    pose = lambda norm=1.0: np.concatenate([unit_quat(norm), r.uniform(-2.0, 2.0, 3)])
    # (name, kind, prm4, pose, n points, where)
    segs = [("empty", SPHERE, [0.7, 0, 0, 0], pose(), 0, "mixed"),
            # (a sphere: every non-zero output of its single point is a number of its own size.  A box's lone point has outputs
            # that vanish analytically -- a dim that neither the nearest face nor the scale involves, or the paths through the
            # scale cancelling -- where the reference's autograd and any restatement return rounding noise that no multiple of
            # the point's own |term| bounds; among the thousands of points of the other segments that noise is far below abs_sum)
            ("one_point", SPHERE, [0.75, 0, 0, 0], pose(), 1, "inside"),
            ("all_outside", SPHERE, [0.6, 0, 0, 0], pose(), 50, "outside"),
            ("rounded_257", ROUNDED, [1.2, 1.0, 0.8, 0.2], pose(), 257, "mixed"),
            ("box_4133", BOX, [0.9, 1.1, 1.3, 0], pose(), 4096 + 37, "mixed"),
            ("box_nonunit_quat", BOX, [1.0, 0.7, 1.2, 0], pose(1.3), 300, "mixed"),
            ("box_equal_dims", BOX, [1.1, 1.1, 1.1, 0], pose(), 200, "mixed"),
            ("cube_rounded", ROUNDED, [1.4, 1.4, 1.4, 0.2], pose(), 200, "mixed"),
            ("sphere", SPHERE, [0.8, 0, 0, 0], pose(0.8), 300, "mixed"),
            ("cylinder", CYLINDER, [0.4, 1.2, 0, 0], pose(), 150, "mixed"),
            ("brick", BRICK, [1.0, 0.8, 0.6, 0.15], pose(), 150, "mixed"),
            ("bowl", BOWL, [0.8, 0.1, 0, 0], pose(), 150, "mixed")]
    pts, off, outs, sums = [], [0], [], []
    for name, kind, prm4, ps, n, where in segs:
        prm4 = np.asarray(prm4, np.float64)
        x = segment_points(r, n, kind, prm4, ps, where)
        o, a = reference_terms(kind, prm4, ps, x)
        print("%-18s n %5d inside %5d  sum %.6e  |d/dpos| %.3e" % (name, n, int(o[1]), o[0], np.abs(o[6:9]).max()))
        pts.append(x); off.append(off[-1] + n); outs.append(o); sums.append(a)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pointcloud_loss.npz"),
                        names=np.array([s[0] for s in segs]), shape_type=np.array([s[1] for s in segs], np.int32),
                        prm=np.array([s[2] for s in segs], np.float64), pose=np.array([s[3] for s in segs]),
                        pts=np.concatenate(pts), seg_off=np.array(off, np.int32), out=np.array(outs), abs_sum=np.array(sums))


if __name__ == "__main__":
    main()
