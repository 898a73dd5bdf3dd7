"""Generate tests/golden/depth_camera_points.npz: what the reference selects from a depth camera's images, and its loss.

    python tools/gen_depth_camera_golden.py      (needs the reference checkout that oracle/refshim imports)
Three small synthetic inputs (48 x 36 images built here in numpy: a depth image, a colour segmentation, a camera pose and a
sphere or rounded-cube estimate) go through the reference's own Recorder3D.get_pointcloud (sdf_physics/physics3d/utils.py) and
match_pointcloud (experiments/trajectory_fitting/optim_pointcloud.py:166-201).  Stored per input: the images (the segmentation
as body indices, the thrown body = BODY), the camera, the estimate, the world-frame points match_pointcloud selects, in its
order, loss_pc_t and the sample count.  The points are read off the reference's own call: with the estimate at the identity
pose the body-frame points it hands to query_sdfs ARE the world-frame points.
The masks: (0) a blob that touches the image border and a one-pixel line, (1) a blob with a hole of depth 0 inside it,
(2) an empty mask."""
import os
import sys
import types

import numpy as np
import scipy.ndimage  # noqa: F401  (the experiment calls sp.ndimage after `import scipy as sp`)
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

refshim.install()
import optim_pointcloud as ref_exp  # noqa: E402
from pytorch3d.transforms import quaternion_to_matrix  # noqa: E402
from sdf_physics.physics3d.bodies import SDFBoxRounded, SDFSphere  # noqa: E402
from sdf_physics.physics3d.utils import Recorder3D  # noqa: E402

W, H, BODY = 48, 36, 2
FX = FY = 38.625      # the experiment's 515 at 48 / 640 of its width
CX, CY = 23.5, 17.5
SPHERE, ROUNDED = 1, 3
COLOURS = {-1: (0, 0, 0), 0: (40, 40, 40), 1: (90, 20, 20), BODY: (10, 200, 30)}


def look_from(eye, yaw, pitch):
    cy_, sy, cp, sp_ = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp_], [0, sp_, cp]])
    M = np.eye(4); M[:3, :3] = Ry @ Rx; M[:3, 3] = eye
    return M


def sphere_depth(centre_cam, r):
    """Depth image of a sphere given in the camera frame (OpenGL: it looks along -z); 0 where the ray misses."""
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(col + 0.5 - CX) / FX, -(row + 0.5 - CY) / FY, -np.ones((H, W))], -1)
    a, b = (d * d).sum(-1), d @ centre_cam
    disc = b * b - a * (centre_cam @ centre_cam - r * r)
    return np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)


class Recording:
    """The estimate as match_pointcloud sees it; keeps the points handed to query_sdfs."""

    def __init__(self, body):
        self.body, self.col, self.pts = body, COLOURS[BODY], None

    def query_sdfs(self, pts, **kw):
        self.pts = pts.detach().clone()
        return self.body.query_sdfs(pts, **kw)


def main():
    r = np.random.default_rng(7)
    inputs = []
    # (0) a sphere cut by the left border, and a one-pixel line of the body's colour over a plane of depth 9
    depth = sphere_depth(np.array([-4.6, 0.8, -9.0]), 1.6)
    seg = np.where(depth > 0, BODY, 0)
    depth[depth == 0] = 12.0
    seg[30, 20:41] = BODY; depth[30, 20:41] = 9.0
    seg[3:9, 40:46] = 1
    inputs.append((depth, seg, look_from([3.0, 6.0, 9.0], 0.3, -0.4), SPHERE, [1.8, 0, 0, 0]))
    # (1) a sphere in the middle with a hole of depth 0 (two pixels and a 2 x 2 block) inside its mask
    depth = sphere_depth(np.array([0.3, -0.2, -8.0]), 2.0)
    seg = np.where(depth > 0, BODY, -1)
    depth[17, 24] = 0.0; depth[14, 20] = 0.0; depth[20:22, 27:29] = 0.0
    inputs.append((depth, seg, look_from([-2.0, 7.0, 8.0], -0.2, -0.5), ROUNDED, [3.6, 3.6, 3.6, 0.2]))
    # (2) nothing of the body in view
    depth = np.full((H, W), 10.0)
    seg = np.zeros((H, W), int); seg[10:20, 10:30] = 1
    inputs.append((depth, seg, look_from([0.0, 5.0, 10.0], 0.0, -0.3), SPHERE, [1.0, 0, 0, 0]))

    rec = Recorder3D.__new__(Recorder3D)      # (its constructor makes directories; get_pointcloud reads these three)
    rec.resolution, rec.noise_factor = (W, H), 0.0
    rec.scene = types.SimpleNamespace(camera_nodes=[types.SimpleNamespace(_camera=types.SimpleNamespace(fx=FX, fy=FY, cx=CX, cy=CY))])
    out = dict(depth=[], seg=[], cam=[], kind=[], prm=[], pose=[], pts=[], off=[0], loss=[], count=[])
    for depth, seg, cam, kind, prm in inputs:
        colour = np.zeros((H, W, 3), np.uint8)
        for k, c in COLOURS.items():
            colour[seg == k] = c
        cloud = rec.get_pointcloud(depth)
        z = [0, 0, 0]
        body = SDFSphere(z, prm[0], custom_mesh=True, custom_inertia=True) if kind == SPHERE else \
            SDFBoxRounded(z, torch.tensor(prm[:3], dtype=torch.double), prm[3])
        est = Recording(body)
        ref_exp.match_pointcloud(cloud, colour, cam, est, torch.zeros(3, dtype=torch.double), torch.eye(3, dtype=torch.double))
        pts = est.pts.numpy().reshape(-1, 3)
        # the estimate: near the points' centre, the cube turned
        q = r.standard_normal(4) if kind == ROUNDED else np.array([1.0, 0, 0, 0])
        q /= np.linalg.norm(q)
        centre = pts.mean(0) if len(pts) else cam[:3, 3] - 10.0 * cam[:3, 2]
        size = prm[0] if kind == SPHERE else prm[0] / 2
        pose = np.concatenate([q, centre + 0.6 * size * (-cam[:3, 2]) + r.uniform(-0.1, 0.1, 3)])      # behind the seen cap
        pos = torch.tensor(pose[4:], dtype=torch.double)
        loss, count = ref_exp.match_pointcloud(cloud, colour, cam, est, pos, quaternion_to_matrix(torch.tensor(q, dtype=torch.double)))
        print("kind %d  selected %4d  in the cube %4d  loss %.6e" % (kind, len(pts), int(count), float(loss)))
        for k, v in zip(("depth", "seg", "cam", "kind", "prm", "pose", "pts", "loss", "count"),
                        (depth, seg.astype(np.int32), cam, kind, prm, pose, pts, float(loss), int(count))):
            out[k].append(v)
        out["off"].append(out["off"][-1] + len(pts))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "depth_camera_points.npz"),
                        depth=np.array(out["depth"]), seg=np.array(out["seg"], np.int32), cam=np.array(out["cam"]),
                        intrinsics=np.array([FX, FY, CX, CY]), body=np.int32(BODY), shape_type=np.array(out["kind"], np.int32),
                        prm=np.array(out["prm"], np.float64), pose=np.array(out["pose"]), pts=np.concatenate(out["pts"]),
                        seg_off=np.array(out["off"], np.int64), loss=np.array(out["loss"]), count=np.array(out["count"], np.int64))


if __name__ == "__main__":
    main()
