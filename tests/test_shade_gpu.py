"""GPU: the colour camera (dss_shade_render of csrc/shade_camera.hip, depth_camera.shade / render_color over it) against the
float64 oracle of tests/shade_ref.py.  The checks and tolerances are those of tests/shade_checks.py, the same that
tests/test_emu_shade.py runs through the emulator; depth and seg come from the device's own depth camera.  The last tests are the
Python surface: shade and render_color return the entry's bits, in one chunk of views and in chunks of one."""
import numpy as np
import pytest
import torch

import depth_camera_ref as ref
import shade_checks as C
import shade_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORDER = ("nview", "nbody", "pose", "shape_type", "prm", "cam", "fx", "fy", "cx", "cy", "W", "H", "zfar", "grid_id", "ngrid", "grid_off", "grid_dims",
         "grid_data", "blk_off", "blk_min", "depth", "seg", "color", "nlight", "light", "ambient", "background", "shadows", "shadow_bias", "normal",
         "shade", "rgb", "flags")
OUT = ("normal", "shade", "rgb", "flags")


def call(A):
    """dss_shade_render on device copies of the arrays of A (background stays on the host); the outputs are copied back into A."""
    from diffsdfsim_amd import _lib
    held, args = {}, []
    for k in ORDER:
        a = A[k]
        if isinstance(a, np.ndarray) and k != "background":
            held[k] = torch.as_tensor(a).to(DEV).contiguous()
            args.append(_lib.ptr(held[k]))
        elif isinstance(a, np.ndarray):
            args.append(a.ctypes.data)
        else:
            args.append(a)
    rc = _lib.lib().dss_shade_render(*args, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    for k in OUT:
        if k in held:
            A[k][...] = held[k].cpu().numpy()
    return rc


def render(pose, kind, prm, grids, gid, cam, fx, fy, cx, cy, W, H):
    from diffsdfsim_amd import depth_camera
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)
    depth, seg = depth_camera.render_depth(t(pose), t(kind, torch.int32), t(prm), cam, fx, fy, cx, cy, size=(W, H), grids=grids, grid_id=gid)
    return depth.cpu().numpy(), seg.cpu().numpy()


@pytest.mark.parametrize("v", range(5))
def test_shaded_view_matches_the_oracle(v):
    C.view_matches_the_oracle(call, render, v)


def test_the_views_hold_shadows_of_object_and_wall_and_unlit_object_pixels():
    C.views_are_not_vacuous(call, render)


def test_four_lights_match_the_oracle():
    C.four_lights_match_the_oracle(call, render)


def test_two_calls_return_the_same_bits():
    C.two_calls_return_the_same_bits(call, render)


def test_shadows_off_and_no_light():
    C.switches(call, render)


def test_a_sphere_over_a_floor_does_not_shadow_itself():
    C.a_convex_body_does_not_shadow_itself(call, render)


@pytest.mark.parametrize("shape", [(33, 33, 33), (33, 17, 25)])
def test_grid_torus_normals_and_self_shadow(shape):
    C.grid_self_shadow(call, render, shape)


@pytest.mark.parametrize("W,H,nview,nbody,nlight", C.BOUNDARIES)
def test_launch_boundaries_guard_view_and_garbage_segments(W, H, nview, nbody, nlight):
    C.launch_boundary(call, render, W, H, nview, nbody, nlight)


def test_refused_arguments_give_a_status_and_leave_the_outputs_alone():
    C.statuses(call, render)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _surface_inputs():
    pose, kind, prm = ref.bounce_views(3)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)
    f = ref.SMALL
    return pose, kind, prm, t(pose), t(kind, torch.int32), t(prm), ref.experiment_camera(), (f["fx"], f["fy"], f["cx"], f["cy"])


def test_shade_returns_the_entrys_bits():
    from diffsdfsim_amd import depth_camera
    pose, kind, prm, tp, tk, tq, cam, K = _surface_inputs()
    depth, seg = depth_camera.render_depth(tp, tk, tq, cam, *K, size=(80, 60))
    lights = [(l[:3], l[3]) for l in S.FOUR_LIGHTS[:2]]
    rgb, normal, shade, flags = depth_camera.shade(depth, seg, tp, tk, tq, cam, *K, S.COLORS[:3], lights, ambient=S.AMBIENT,
                                                   background=S.BACKGROUND)
    want = S.run(call, S.arguments(pose, kind, prm, cam, depth.cpu().numpy(), seg.cpu().numpy(), lights=S.FOUR_LIGHTS[:2]))
    for name, got in (("rgb", rgb), ("normal", normal), ("shade", shade), ("flags", flags)):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want[name]), name
    assert (seg >= 0).any() and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (5, 60, 80, 3)


def test_render_color_is_render_depth_then_shade_in_any_chunks(monkeypatch):
    from diffsdfsim_amd import depth_camera
    pose, kind, prm, tp, tk, tq, cam, K = _surface_inputs()
    lights = [(S.LIGHT[0][:3], S.LIGHT[0][3])]
    kw = dict(size=(80, 60), ambient=S.AMBIENT, background=S.BACKGROUND)
    rgb, depth, seg = depth_camera.render_color(tp, tk, tq, cam, *K, S.COLORS[:3], lights, **kw)
    d0, s0 = depth_camera.render_depth(tp, tk, tq, cam, *K, size=(80, 60))
    want = S.run(call, S.arguments(pose, kind, prm, cam, d0.cpu().numpy(), s0.cpu().numpy()))
    assert torch.equal(depth, d0) and torch.equal(seg, s0) and np.array_equal(rgb.cpu().numpy(), want["rgb"])
    chunks = []
    monkeypatch.setattr(depth_camera, "views_per_chunk", lambda *a, **k: chunks.append(a) or 1)
    r1, d1, s1 = depth_camera.render_color(tp, tk, tq, cam, *K, S.COLORS[:3], lights, **kw)
    assert chunks and torch.equal(r1, rgb) and torch.equal(d1, depth) and torch.equal(s1, seg)
    monkeypatch.undo()
    assert depth_camera.views_per_chunk((80, 60), 48 * 4800 * 3, 48) == 3 and depth_camera.views_per_chunk((80, 60), 1, 48) == 1


def test_a_library_without_the_entry_raises(monkeypatch):
    from diffsdfsim_amd import _lib, depth_camera
    real = _lib.lib()

    class Without:      # the loaded library, less the one entry
        def __getattr__(self, name):
            if name == "dss_shade_render":
                raise AttributeError(name)
            return getattr(real, name)
    pose, kind, prm, tp, tk, tq, cam, K = _surface_inputs()
    depth, seg = depth_camera.render_depth(tp[:1], tk[:1], tq[:1], cam, *K, size=(16, 16))
    # the loader is where a library is held to the headers: let it load this one
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Without())
    with pytest.raises(_lib.HipLibraryError, match="dss_shade_render"):
        depth_camera.shade(depth, seg, tp[:1], tk[:1], tq[:1], cam, *K, S.COLORS[:3], [])
