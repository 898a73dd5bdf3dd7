"""Defaults of the 3-D SDF layer (mirrors sdf_physics/physics3d/utils.py:41-62, lcp_physics/physics/utils.py:33-67)."""
import torch


class Defaults3D:
    DIM = 3
    EPSILON = 0.001          # contact detection band
    TOL = 1e-8               # penetration tolerance
    RESTITUTION = 0.5
    FRIC_COEFF = 0.9
    FRIC_DIRS = 8
    FPS = 30
    DT = 1.0 / FPS
    ENGINE = "HipPdipmEngine"
    CONTACT = "FWContactHandler"
    SOLVER = 1
    DTYPE = torch.double
    DEVICE = torch.device("cuda:0")
    POST_STABILIZATION = False
    CUSTOM_MESH = False      # as sdf_physics/physics3d/utils.py:56-57: level-set (marching cubes) mesh and mesh inertia unless
    CUSTOM_INERTIA = False   # the caller asks for the analytic ones


def get_tensor(x, base_tensor=None, **kw):
    """Wrap array or scalar in a float64 tensor (reference utils.py:270-283); host-side parameters live on the CPU
    unless the caller passes device tensors -- the engine copies them to the HIP device."""
    if isinstance(x, torch.Tensor):
        return x
    if base_tensor is not None:
        return base_tensor.new_tensor(x, **kw)
    return torch.tensor(x, dtype=Defaults3D.DTYPE, **kw)


def decode_igr(network):
    """`decode_igr` (sdf_physics/physics3d/utils.py:330-350): IGR ImplicitNet -> ``sdf(pts, latent)`` evaluated on the device;
    the result is what ``SDF3D(sdf_func=...)`` takes (diffsdfsim_amd/igr.py)."""
    from ..igr import decode_igr as _decode
    return _decode(network)


def _rot4(rows):
    return torch.stack([torch.stack([torch.as_tensor(x, dtype=Defaults3D.DTYPE) for x in r]) for r in rows])


def Rx(theta):
    """Homogeneous 4x4 rotation about x (sdf_physics/physics3d/utils.py:183-188)."""
    t = get_tensor(theta); c, s = torch.cos(t), torch.sin(t)
    return _rot4([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]])


def Ry(theta):
    """About y, with the reference's sign convention (-sin in the first row; utils.py:191-196)."""
    t = get_tensor(theta); c, s = torch.cos(t), torch.sin(t)
    return _rot4([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]])


def Rz(theta):
    """About z (utils.py:199-204)."""
    t = get_tensor(theta); c, s = torch.cos(t), torch.sin(t)
    return _rot4([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


class Scene:
    """What the recorder needs of the reference's pyrender.Scene: one pinhole camera, directional lights, an ambient term and a
    background colour.  camera_pose: the 4 x 4 camera-to-world matrix (OpenGL convention, the camera looks along its -z); fx, fy,
    cx, cy in pixels of the recorder's resolution (yfov: fy = H / 2 / tan(yfov / 2)).  A light is (direction, intensity): a
    3-vector along which the light travels, or a 4 x 4 pose whose -z axis is that direction, as pyrender.DirectionalLight is posed.
    ambient_light: a number, or an rgb triple whose mean is taken.  run_world puts the world's bodies into `bodies`."""

    def __init__(self, camera_pose, fx, fy, cx, cy, znear=0.1, zfar=100.0, lights=(), ambient_light=0.1, bg_color=(1.0, 1.0, 1.0)):
        import numpy as np
        self.camera_pose = np.array(_np(camera_pose), np.float64).reshape(4, 4)
        self.fx, self.fy, self.cx, self.cy, self.znear, self.zfar = float(fx), float(fy), float(cx), float(cy), float(znear), float(zfar)
        self.lights = []
        for direction, intensity in lights:
            self.add_light(direction, intensity)
        self.ambient_light = float(np.mean(_np(ambient_light)))
        self.bg_color = tuple(float(c) for c in bg_color)[:3]
        self.bodies = []

    def add_light(self, direction, intensity=1.0):
        import numpy as np
        d = np.array(_np(direction), np.float64)
        d = -d[:3, 2] if d.shape == (4, 4) else d.reshape(3)      # (a pose: the light travels along its -z)
        self.lights.append((-d, float(intensity)))      # kept as the direction TOWARDS the light, as the kernel takes it


def _col01(col):
    """A body's colour in [0, 1]: integers are 0..255 as in the reference (bodies.py:444-447), anything else is taken as given."""
    return [c / 255.0 for c in col[:3]] if all(isinstance(c, int) for c in col) else [float(c) for c in col[:3]]


def write_png(path, img):
    """An 8-bit PNG from a [H,W] (grey) or [H,W,3] (rgb) uint8 array: one zlib stream, every row with filter type 0."""
    import struct
    import zlib

    import numpy as np
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, -1)], 1).tobytes()
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))


class Recorder3D:
    """The reference's frame recorder (utils.py:65-154) on the device's colour camera (depth_camera.render_color) in place of
    pyrender.  With a `Scene`, record(t) -- once `dt` has passed since the last frame, as there -- returns (color_img [H,W,3] uint8,
    depth_img [H,W] float64, pc [H,W,3] or None, segmentation_mask [H,W,3] uint8 or None, [camera pose]); pc is the reference's
    back-projection (x, y, z) = (nx d, ny d, d) of the depth with noise_factor * d^2 * randn added (record_points), the mask is
    coloured by the bodies' `col` or by seg_node_map[body] (record_seg).  rotate: the camera turns about rotate_axis by
    dt * rotate_rate per frame.  save_to_disk writes color_N.png, depth_N.png (8-bit grey, depth / its maximum), depth_N.npy,
    seg_N.png and pointcloud_N.npy into `path`.  The bodies drawn are scene.bodies, which run_world sets.
    Without a Scene (scene=None, or any other object) nothing is rendered: the recorder keeps the time stamps and returns Nones."""

    def __init__(self, dt, scene=None, path=None, resolution=(640, 480), rotate=False, rotate_rate=0.0, rotate_axis=(0, 0, 1),
                 record_points=False, record_seg=False, noise_factor=0.0, save_to_disk=False):
        self.dt, self.scene, self.path, self.frame, self.prev_t, self.times = dt, scene, path, 0, 0.0, []
        self.resolution, self.rotate, self.rotate_rate, self.rotate_axis = tuple(resolution), rotate, rotate_rate, rotate_axis
        self.record_points, self.record_seg, self.noise_factor, self.save_to_disk = record_points, record_seg, noise_factor, save_to_disk

    def get_pointcloud(self, depth_img):
        """utils.py:81-105: camera-frame points [H,W,3] = (nx d, ny d, d) of the noisy depth (y down, z forward, not yet flipped)."""
        import numpy as np
        s = self.scene
        x, y = np.meshgrid(np.arange(self.resolution[0]), np.arange(self.resolution[1]))
        nx, ny = (x + 0.5 - s.cx) / s.fx, (y + 0.5 - s.cy) / s.fy
        d = depth_img + np.random.randn(*depth_img.shape) * self.noise_factor * depth_img ** 2
        return np.stack((nx * d, ny * d, d), axis=-1)

    def _views(self):
        """The scene's bodies as one view of the camera's arguments."""
        import numpy as np

        from .. import depth_camera, world_abi as abi
        bodies = self.scene.bodies
        dev = Defaults3D.DEVICE
        pose = torch.stack([b.p.detach().to(torch.float64).cpu() for b in bodies])[None].to(dev)
        prm = torch.stack([torch.cat([b.shape_prm().detach().reshape(-1).to(torch.float64).cpu(), torch.tensor([b.shape_aux()], dtype=torch.float64)])
                           for b in bodies])[None].to(dev)
        types = np.array([[b.shape_type for b in bodies]], np.int32)
        level = [b for b in bodies if b.shape_type in (abi.SHAPE_GRID, abi.SHAPE_IGR)]
        grids, gid = None, None
        if level:      # a voxel grid, or the value grid a neural body's mesh is extracted from
            grids = [depth_camera.body_grid(b)[0] for b in level]
            gid = np.array([[level.index(b) if b in level else -1 for b in bodies]], np.int32)
        return pose, types, prm, grids, gid

    def record(self, t, seg_node_map=None):
        if not isinstance(self.scene, Scene):
            if t - self.prev_t >= self.dt:
                self.times.append(float(t)); self.frame += 1; self.prev_t += self.dt
            return None, None, None, None, []
        color_img, depth_img, pc, mask, camera_poses = None, None, None, None, []
        if t - self.prev_t >= self.dt:
            import os

            import numpy as np

            from .. import depth_camera
            s = self.scene
            if self.rotate:      # utils.py:112-118: axis_angle_to_matrix(axis * angle) in front of the camera's pose
                a = np.asarray(_np(get_tensor(self.rotate_axis)), np.float64) * (self.dt * self.rotate_rate)
                th = np.linalg.norm(a)
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / (th if th > 0 else 1.0)
                rot = np.eye(4)
                rot[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
                s.camera_pose = rot @ s.camera_pose
            camera_poses.append(s.camera_pose.copy())
            pose, types, prm, grids, gid = self._views()
            cols = [_col01(b.col) for b in s.bodies]
            rgb, depth, seg = depth_camera.render_color(pose, types, prm, s.camera_pose, s.fx, s.fy, s.cx, s.cy, cols, s.lights, size=self.resolution,
                                                        znear=s.znear, zfar=s.zfar, ambient=s.ambient_light, background=s.bg_color,
                                                        grids=grids, grid_id=gid)
            color_img, depth_img, seg = rgb[0].cpu().numpy(), depth[0].cpu().numpy(), seg[0].cpu().numpy()
            if self.save_to_disk:
                os.makedirs(self.path, exist_ok=True)
                write_png(os.path.join(self.path, "color_{}.png".format(self.frame)), color_img)
                top = depth_img.max()
                write_png(os.path.join(self.path, "depth_{}.png".format(self.frame)), np.floor(255.0 * depth_img / (top if top > 0 else 1.0) + 0.5))
                np.save(os.path.join(self.path, "depth_{}.npy".format(self.frame)), depth_img)
            if self.record_seg:
                table = np.zeros((len(s.bodies) + 1, 3), np.uint8)      # (the last row: no body, black as pyrender's SEG background)
                for j, b in enumerate(s.bodies):
                    c = (seg_node_map or {}).get(b, b.col)
                    table[j] = np.floor(255.0 * np.asarray(_col01(tuple(c))) + 0.5)
                mask = table[np.where(seg >= 0, seg, len(s.bodies))]
                if self.save_to_disk:
                    write_png(os.path.join(self.path, "seg_{}.png".format(self.frame)), mask)
            if self.record_points:
                pc = self.get_pointcloud(depth_img)
                if self.save_to_disk:
                    np.save(os.path.join(self.path, "pointcloud_{}.npy".format(self.frame)), pc)
            self.times.append(float(t)); self.frame += 1; self.prev_t += self.dt
        return color_img, depth_img, pc, mask, camera_poses


class _LoadedImplicitNet(torch.nn.Module):
    """lin0 .. lin{n-1} rebuilt from an IGR checkpoint's state dict: the shape decode_igr needs (the class itself lives in the
    external IGR repository, which the reference imports by file path, utils.py:300-308)."""

    def __init__(self, state):
        super().__init__()
        n = 0
        while "lin%d.weight" % n in state:
            W = state["lin%d.weight" % n]
            lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(Defaults3D.DTYPE)
            with torch.no_grad():
                lin.weight.copy_(W); lin.bias.copy_(state["lin%d.bias" % n])
            setattr(self, "lin%d" % n, lin)
            n += 1
        self.num_layers = n + 1


def load_igrnet(experiment_dir, timestamp='latest', checkpoint='latest', run=None):
    """`load_igrnet` (utils.py:286-327): (network, latent codes) of a trained IGR run -- newest time stamp directory unless given,
    ``checkpoints/LatentCodes/<ckpt>.pth['latent_codes']`` and ``checkpoints/ModelParameters/<ckpt>.pth['model_state_dict']``.
    The layer sizes are read off the state dict (the reference reads them from exp.conf through pyhocon)."""
    import os
    if timestamp == 'latest':
        stamps = sorted(os.listdir(experiment_dir))
        if not stamps:
            raise FileNotFoundError('No timestamp directories found in {}'.format(experiment_dir))
        timestamp = stamps[-1]
    ck = os.path.join(experiment_dir, timestamp, 'checkpoints')
    lat = torch.load(os.path.join(ck, 'LatentCodes', str(checkpoint) + '.pth'), map_location='cpu')["latent_codes"]
    state = torch.load(os.path.join(ck, 'ModelParameters', str(checkpoint) + '.pth'), map_location='cpu')["model_state_dict"]
    net = _LoadedImplicitNet({k: v.detach().to(Defaults3D.DTYPE) for k, v in state.items()})
    net.eval()
    return net, lat.detach().to(Defaults3D.DTYPE)
