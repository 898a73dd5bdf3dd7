"""GPU: dss_pointcloud_loss_grids (csrc/pointcloud_loss.hip) through diffsdfsim_amd.pointcloud against
tests/golden/pointcloud_loss_grid.npz, the reference's match_pointcloud arithmetic with its own SDFGrid3D
(tools/gen_pointcloud_grid_golden.py).  Segments, tolerance (1e-12 x abs_sum per output, counts exact, prm outputs of grid
segments exactly 0) and their derivation: tests/test_emu_pointcloud_loss_grid.py."""
import os

import numpy as np
import pytest
import torch

from test_emu_pointcloud_loss_grid import check_against_golden

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "pointcloud_loss_grid.npz")


@pytest.fixture(scope="module")
def case():
    from diffsdfsim_amd import pointcloud
    from diffsdfsim_amd.grids import GridTable
    g = dict(np.load(G))
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
    g["table"] = GridTable([g["grid_0"], g["grid_1"]], dev)
    g["t"] = dict(pts=t(g["pts"]), pose=t(g["pose"]), prm=t(g["prm"]), types=t(g["shape_type"], torch.int32), gid=t(g["grid_id"], torch.int32),
                  off=t(g["seg_off"], torch.int32))
    T = g["t"]
    g["max_len"] = int(np.diff(g["seg_off"]).max())
    g["raw"] = pointcloud._launch(T["pts"], T["off"], g["max_len"], T["pose"], T["types"], T["prm"], g["table"], T["gid"])
    return g


def test_every_segment_matches_the_reference_golden(case):
    check_against_golden(case["raw"].cpu().numpy(), case)


def test_two_calls_return_the_same_bits_and_analytic_segments_those_of_the_analytic_call(case):
    from diffsdfsim_amd import pointcloud
    T = case["t"]
    again = pointcloud._launch(T["pts"], T["off"], case["max_len"], T["pose"], T["types"], T["prm"], case["table"], T["gid"])
    assert torch.equal(again, case["raw"])
    off = case["seg_off"]
    for s in np.nonzero(case["shape_type"] != 7)[0]:
        n = int(off[s + 1] - off[s])
        one = pointcloud._launch(T["pts"][off[s]:off[s + 1]].contiguous(), torch.tensor([0, n], dtype=torch.int32, device=T["pts"].device), n,
                                 T["pose"][s:s + 1].contiguous(), T["types"][s:s + 1].contiguous(), T["prm"][s:s + 1].contiguous())
        assert n > 0 and torch.equal(one[0], case["raw"][s]), case["names"][s]      # one chunk either way: the same lanes, the same order


def test_autograd_function_returns_sum_count_and_the_kernels_jacobian(case):
    from diffsdfsim_amd import pointcloud
    T = case["t"]
    pose, prm = T["pose"].clone().requires_grad_(), T["prm"].clone().requires_grad_()
    loss, count = pointcloud.match_pointcloud(T["pts"], case["seg_off"], pose, case["shape_type"], prm, grids=case["table"], grid_id=case["grid_id"])
    assert torch.equal(loss, case["raw"][:, 0]) and torch.equal(count, case["raw"][:, 1]) and not count.requires_grad
    w = torch.linspace(0.5, 2.0, loss.numel(), dtype=torch.float64, device=loss.device)
    (loss * w).sum().backward()
    assert torch.equal(pose.grad, w[:, None] * case["raw"][:, 2:9])
    grid = torch.as_tensor(case["shape_type"] == 7, device=loss.device)
    assert bool((prm.grad[grid] == 0).all()) and torch.equal(prm.grad[:, :3], w[:, None] * case["raw"][:, 9:12])
    assert bool((prm.grad[~grid][:, :3] != 0).any())


@pytest.mark.parametrize("kind,gid", [(6, 0), (6, -1), (7, -1)])
def test_refused_segments_leave_out_alone_and_raise(case, kind, gid):
    from diffsdfsim_amd import _lib, pointcloud
    T, tab = case["t"], case["table"]
    dev = T["pts"].device
    types, ids = T["types"].clone(), T["gid"].clone()
    types[4], ids[4] = kind, gid
    nseg = types.numel()
    L = _lib.lib()
    out = torch.full((nseg, 12), -7.0, dtype=torch.float64, device=dev)
    nbytes = L.dss_pointcloud_loss_workspace_bytes(nseg, case["max_len"])
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    rc = L.dss_pointcloud_loss_grids(nseg, case["max_len"], _lib.ptr(T["off"]), _lib.ptr(T["pts"]), _lib.ptr(T["pose"]), _lib.ptr(types),
                                     _lib.ptr(T["prm"]), _lib.ptr(ids), tab.ngrid, _lib.ptr(tab.off), _lib.ptr(tab.dims), _lib.ptr(tab.data),
                                     _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == -7.0).all())
    with pytest.raises(_lib.HipLibraryError):
        pointcloud.match_pointcloud(T["pts"], case["seg_off"], T["pose"], types, T["prm"], grids=tab, grid_id=ids)


def test_grid_body_pointcloud_loss_is_the_single_segment_call(case):
    from diffsdfsim_amd.physics3d import SDFGrid3D
    names, off = list(case["names"]), case["seg_off"]
    s = names.index("torus_257")
    pose = torch.tensor(case["pose"][s], dtype=torch.float64, requires_grad=True)
    body = SDFGrid3D(pose, float(case["prm"][s, 3]), case["grid_0"])
    loss, count = body.pointcloud_loss(case["pts"][off[s]:off[s + 1]])
    loss.backward()
    # one segment of 257 points is one chunk, summed by the same lanes as in the batched call -> the same bits
    assert float(loss.detach()) == float(case["raw"][s, 0]) and float(count) == float(case["raw"][s, 1])
    assert np.array_equal(pose.grad.numpy(), case["raw"][s, 2:9].cpu().numpy())
