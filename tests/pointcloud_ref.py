"""float64 torch-autograd restatement of the point-cloud loss (match_pointcloud, optim_pointcloud.py:166-201) for the tests:
pytorch3d's quaternion_to_matrix and the sphere / box / rounded-box SDFs of sdf_physics/physics3d/bodies.py in the unit frame
of SDF3D.query_sdfs.  Runs on whatever device its tensors are on."""
import torch

BOX, SPHERE, ROUNDED = 0, 1, 3


def quaternion_to_matrix(q):
    r, i, j, k = q[0], q[1], q[2], q[3]
    two_s = 2.0 / (q * q).sum()
    return torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                        two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)]).reshape(3, 3)


def segment_loss(kind, prm, r, pose, pts):
    """-> (sum of sdf^2 over the points inside the query cube, their number); prm [3], pose [7] may require grad."""
    R = quaternion_to_matrix(pose[:4])
    p = (R.T.unsqueeze(0) @ (pts - pose[4:]).unsqueeze(-1)).squeeze(-1)
    scale = prm[0] * 1.5 if kind == SPHERE else torch.max(prm) * 1.5 / 2
    mask = torch.all(torch.abs(p) <= scale, dim=1)
    u = p[mask] / scale
    if kind == SPHERE:
        sdf = torch.linalg.norm(u, dim=1) - prm[0] / scale
    else:
        hd = (prm - 2 * r) / scale / 2 if kind == ROUNDED else prm / scale / 2
        q = torch.abs(u) - hd
        sdf = torch.linalg.norm(torch.clamp(q, min=0.0), dim=1) + torch.clamp(torch.max(q, dim=1).values, max=0.0)
        if kind == ROUNDED:
            sdf = sdf - r / scale
    sdf = sdf * scale
    return torch.sum(sdf ** 2), mask.sum()
