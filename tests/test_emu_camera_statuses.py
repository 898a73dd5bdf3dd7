"""CPU: the statuses of the camera entries and of the point-cloud entries that take a grid table, through the emulator: the cases of
tests/camera_status_cases.py, which tests/test_camera_statuses_gpu.py runs on the device."""
import numpy as np
import pytest

import camera_status_cases as C
from emu import emu


def run(name, args, outs):
    at = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.a.ctypes.data if isinstance(a, C.Host) else a
    return getattr(emu.lib(), name)(*[at(a) for a in args], None)


@pytest.mark.parametrize("entry,name", C.CAMERA_IDS)
def test_camera_status(entry, name):
    C.check_camera(run, emu.lib, entry, name)


@pytest.mark.parametrize("entry,name", C.POINTCLOUD_IDS)
def test_pointcloud_status(entry, name):
    C.check_pointcloud(run, emu.lib, entry, name)
