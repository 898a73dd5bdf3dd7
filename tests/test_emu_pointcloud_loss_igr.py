"""CPU: dss_pointcloud_loss_igr (csrc/pointcloud_loss_igr.hip: count, scan, ordered compaction, the MFMA network over the compacted
list, reduction) through the emulator against tests/golden/pointcloud_loss_igr.npz, the reference's match_pointcloud arithmetic
over SDF3D.query_sdfs and decode_igr with torch autograd (tools/gen_pointcloud_igr_golden.py).  Cases, tolerance and its
derivation: tests/pointcloud_igr_cases.py; the device twin is tests/test_pointcloud_loss_igr_gpu.py.
The emulated MFMA network takes 0.09 s per point on the 128-wide network and 0.6 s on the 256-wide one, so beside sparse_4133
(three chunks, 151 inside), the adjacent pair, the shared rows and the empty, one-point and all-outside segments this module
walks the golden's small twins of the large segments -- mixed_33, nonunit_25 (|q| = 1.3, scale 0.7) and, on the 256-wide network,
mixed_12 and the adjacent pair small_a (|q| = 1.2) / small_b with different latent rows -- and takes its central differences on
fd_nonunit_6 (six points inside, |q| = 1.3) and, 256-wide, on one_point; mixed_257 and nonunit_quat themselves run on the device.
tests/emu/check_pointcloud_loss_igr.cpp walks the compaction as a program of its own under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import igr_helpers as H
import pointcloud_igr_cases as C
from emu import emu

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = {0: C.named(0, ["empty", "one_point", "all_outside", "sparse_4133", "pair_a", "pair_b", "shared_a", "shared_b", "mixed_33", "nonunit_25",
                      "fd_nonunit_6"]),
       1: C.named(1, ["small_a", "small_b", "mixed_12", "one_point"])}      # (the pair's boundary after 3 entries: inside a 4-point group)
FD = {0: "fd_nonunit_6", 1: "one_point"}


@pytest.fixture(scope="module")
def backend():
    return emu.EmuBackend()


@pytest.fixture(scope="module")
def packed(backend):
    return {k: H.packed_on(backend, *C.weights(k)) for k in (0, 1)}


@pytest.fixture(scope="module")
def full(backend, packed):
    """One call per network over the segments this module walks, shared by the tests below and left unchanged."""
    return {k: C.launch(backend, packed[k], k, IDS[k]) for k in (0, 1)}


@pytest.mark.parametrize("k", [0, 1])
def test_every_segment_matches_the_reference_golden(full, k):
    C.check_against_golden(full[k], IDS[k], "emu")


@pytest.mark.parametrize("k", [0, 1])
def test_every_slot_is_written_and_the_zeros_are_exact(full, k):
    C.check_exact_zeros(full[k], IDS[k], k)


def test_a_subset_of_segments_returns_the_rows_of_the_full_call_and_two_calls_the_same_bits(backend, packed, full):
    ids = IDS[0]
    pick = C.named(0, ["pair_b", "empty", "one_point"])      # other offsets in the list, other tile mates
    sub = C.launch(backend, packed[0], 0, pick)
    for row, s in zip(sub, pick):
        assert np.array_equal(row, full[0][ids.index(s)]), C.golden()["names"][s]
    assert np.array_equal(C.launch(backend, packed[0], 0, pick), sub)


def test_only_empty_segments_need_no_workspace_and_give_zeros(backend, packed):
    c = C.Call(backend, packed[0], 0, [C.index_of(0, "empty")] * 2)
    assert c.nbytes == 0 and c.run() == 0 and np.all(c.result() == 0.0)


@pytest.mark.parametrize("k", [0, 1])
def test_central_differences_in_pose_and_latent(backend, packed, full, k):
    ids, pose, table, rows = C.central_difference_segments(k, FD[k])
    out = C.launch(backend, packed[k], k, ids, pose=pose, table=table, lat_rows=rows)
    C.check_central_differences(out, full[k][IDS[k].index(ids[0])], k, FD[k])


@pytest.mark.parametrize("k", [0, 1])
def test_return_codes(backend, packed, k):
    C.check_return_codes(backend, packed[k], k)


def test_stand_alone_program_under_the_sanitizers():
    out = os.path.join(HERE, "emu", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "check_pointcloud_loss_igr")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w", "-DDSS_EMU", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(HERE, "..", "diffsdfsim_amd", "csrc"),
           "-o", exe, os.path.join(HERE, "emu", "check_pointcloud_loss_igr.cpp")]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        # only a link without the sanitizers' runtimes may fall back to a plain build; any other failure is the program's
        assert "cannot find" in san.stderr and ("asan" in san.stderr or "ubsan" in san.stderr), san.stderr[-2000:]
        subprocess.check_call(cmd)
    print("check_pointcloud_loss_igr built %s the sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    w = r.stdout.split()
    assert int(w[0]) == 3 and int(w[2]) > 0, r.stdout      # calls walked, points compacted
