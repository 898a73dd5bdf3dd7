"""GPU: the statuses of the camera entries and of the point-cloud entries that take a grid table, on the device: the cases of
tests/camera_status_cases.py, which tests/test_emu_camera_statuses.py runs through the emulator."""
import numpy as np
import pytest
import torch

import camera_status_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def lib():
    from diffsdfsim_amd import _lib
    return _lib.lib()


def run(name, args, outs):
    """The entry on device copies of the arrays; the device's values of `outs` are copied back into them."""
    from diffsdfsim_amd import _lib
    held = [torch.as_tensor(a).to(DEV).contiguous() if isinstance(a, np.ndarray) else None for a in args]
    at = [_lib.ptr(t) if t is not None else a.a.ctypes.data if isinstance(a, C.Host) else a for a, t in zip(args, held)]
    rc = getattr(lib(), name)(*at, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    for a, t in zip(args, held):
        if any(a is o for o in outs):
            a[...] = t.cpu().numpy()
    return rc


@pytest.mark.parametrize("entry,name", C.CAMERA_IDS)
def test_camera_status(entry, name):
    C.check_camera(run, lib, entry, name)


@pytest.mark.parametrize("entry,name", C.POINTCLOUD_IDS)
def test_pointcloud_status(entry, name):
    C.check_pointcloud(run, lib, entry, name)
