"""CPU: the colour camera (dss_shade_render of csrc/shade_camera.hip) through the emulator -- the kernels, their launch shapes and
the LDS tables as on the device -- against the float64 oracle of tests/shade_ref.py.  The checks and their tolerances are those of
tests/shade_checks.py, which tests/test_shade_gpu.py runs on the device; depth and seg come from the emulated dss_depth_render /
dss_depth_render_grids."""
import numpy as np
import pytest

import grid_ref as G
import shade_checks as C
from emu import emu

_c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)
_p = lambda a: None if a is None else a.ctypes.data
ORDER = ("nview", "nbody", "pose", "shape_type", "prm", "cam", "fx", "fy", "cx", "cy", "W", "H", "zfar", "grid_id", "ngrid", "grid_off", "grid_dims",
         "grid_data", "blk_off", "blk_min", "depth", "seg", "color", "nlight", "light", "ambient", "background", "shadows", "shadow_bias", "normal",
         "shade", "rgb", "flags")


def call(A):
    return emu.lib().dss_shade_render(*[_p(A[k]) if (A[k] is None or isinstance(A[k], np.ndarray)) else A[k] for k in ORDER], None)


def render(pose, kind, prm, grids, gid, cam, fx, fy, cx, cy, W, H):
    L = emu.lib()
    pose, kind, prm, cam = _c(pose), _c(kind, np.int32), _c(prm), _c(cam)
    nview, nbody = kind.shape
    depth, seg = np.zeros((nview, H, W)), np.full((nview, H, W), -1, np.int32)
    if grids is None:
        rc = L.dss_depth_render(nview, nbody, _p(pose), _p(kind), _p(prm), _p(cam), fx, fy, cx, cy, W, H, 0.1, 100.0, _p(depth), _p(seg), None)
    else:
        off, dims, data, blk_off, nblk = G.pooled(grids)
        bmin, gid = _c(np.concatenate([G.block_min(g) for g in grids])), _c(gid, np.int32)
        rc = L.dss_depth_render_grids(nview, nbody, _p(pose), _p(kind), _p(prm), _p(cam), fx, fy, cx, cy, W, H, 0.1, 100.0, _p(gid), len(grids),
                                      _p(off), _p(dims), _p(data), _p(blk_off), _p(bmin), _p(depth), _p(seg), None)
    assert rc == 0
    return depth, seg


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
