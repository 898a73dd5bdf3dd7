"""GPU: dss_pointcloud_loss (csrc/pointcloud_loss.hip) through diffsdfsim_amd.pointcloud against
  - tests/golden/pointcloud_loss.npz, the reference's `match_pointcloud` arithmetic and its autograd gradient on the CPU
    (tools/gen_pointcloud_golden.py), every primitive, and
  - a float64 torch-autograd restatement on the device (tests/pointcloud_ref.py: sphere, box, rounded box).
All segments go through ONE call: empty, one point, every point outside the query cube, 257 points (crosses a workgroup),
4096 + 37 points (three chunks), a quaternion of length 1.3, a box with three equal dims, mixed shape types.

Tolerance: an output is held to 1e-12 x abs_sum of that output (the golden's sum of absolute per-point terms): the order of
summation costs at most n 2^-53 abs_sum = 4.5e-13 abs_sum at n = 4133, the rounding of a term's ~100 operations about 1e-14
abs_sum.  Never relative to the value: position gradients cancel.  Every point keeps 1e-6 from the faces of its query cube
(checked by the generator), so the count is asserted exactly.

One exception to abs_sum, made in the generator: a sphere's SDF does not depend on the rotation, so each point's quaternion
term is exactly zero and what the reference and the kernel return there is rounding noise of the chain rule's summands.  For
the quaternion outputs (2..5) of SPHERE segments only, abs_sum is the sum of |d phi^2 / d p_i| |d p_i / d q_k| over points and
i; every other output of every segment uses the sum of the absolute per-point terms."""
import os

import numpy as np
import pytest
import torch

import pointcloud_ref as ref

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "pointcloud_loss.npz")


@pytest.fixture(scope="module")
def case():
    from diffsdfsim_amd import pointcloud
    g = dict(np.load(G))
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
    g["t"] = dict(pts=t(g["pts"]), pose=t(g["pose"]), prm=t(g["prm"]), types=t(g["shape_type"], torch.int32))
    T = g["t"]
    g["raw"] = pointcloud._launch(T["pts"], t(g["seg_off"], torch.int32), int(np.diff(g["seg_off"]).max()), T["pose"], T["types"], T["prm"])
    return g


def test_every_segment_matches_the_reference_golden(case):
    out, gold, abs_sum = case["raw"].cpu().numpy(), case["out"], case["abs_sum"]
    names = list(case["names"])
    assert sorted(set(case["shape_type"])) == [0, 1, 2, 3, 4, 5]
    assert np.diff(case["seg_off"])[[names.index(n) for n in ("empty", "one_point", "rounded_257", "box_4133")]].tolist() == [0, 1, 257, 4133]
    assert abs(np.linalg.norm(case["pose"][names.index("box_nonunit_quat"), :4]) - 1.3) < 1e-12
    for s, name in enumerate(names):
        print(name, "count", out[s, 1], "worst |out - golden| / abs_sum %.2e" % (np.abs(out[s] - gold[s]) / np.maximum(abs_sum[s], 1e-300)).max())
    assert np.array_equal(out[:, 1], gold[:, 1]), "mask counts differ"
    for name in ("empty", "all_outside"):
        assert np.all(out[names.index(name)] == 0.0), name
    assert np.all(np.abs(out - gold) <= 1e-12 * abs_sum), np.argwhere(np.abs(out - gold) > 1e-12 * abs_sum)


def test_sphere_box_rounded_segments_match_torch_autograd(case):
    out, abs_sum, off = case["raw"].cpu().numpy(), case["abs_sum"], case["seg_off"]
    T = case["t"]
    seen = set()
    for s, kind in enumerate(case["shape_type"]):
        if kind not in (ref.BOX, ref.SPHERE, ref.ROUNDED):
            continue
        seen.add(int(kind))
        pose, prm = T["pose"][s].clone().requires_grad_(), T["prm"][s, :3].clone().requires_grad_()
        loss, count = ref.segment_loss(int(kind), prm, float(case["prm"][s, 3]), pose, T["pts"][off[s]:off[s + 1]])
        want = np.zeros(12)
        want[0], want[1] = float(loss), int(count)
        if int(count):
            gp, gr = torch.autograd.grad(loss, [pose, prm])
            want[2:9], want[9:] = gp.cpu().numpy(), gr.cpu().numpy()
        assert out[s, 1] == want[1], case["names"][s]
        assert np.all(np.abs(out[s] - want) <= 1e-12 * abs_sum[s]), (case["names"][s], out[s] - want, abs_sum[s])
    assert seen == {ref.BOX, ref.SPHERE, ref.ROUNDED}


def test_autograd_function_returns_sum_count_and_the_kernels_jacobian(case):
    from diffsdfsim_amd import pointcloud
    T = case["t"]
    pose, prm = T["pose"].clone().requires_grad_(), T["prm"].clone().requires_grad_()
    loss, count = pointcloud.match_pointcloud(T["pts"], case["seg_off"], pose, case["shape_type"], prm)
    assert torch.equal(loss, case["raw"][:, 0]) and torch.equal(count, case["raw"][:, 1]) and not count.requires_grad
    w = torch.linspace(0.5, 2.0, loss.numel(), dtype=torch.float64, device=loss.device)
    (loss * w).sum().backward()
    assert torch.equal(pose.grad, w[:, None] * case["raw"][:, 2:9])
    assert torch.equal(prm.grad[:, :3], w[:, None] * case["raw"][:, 9:12]) and bool((prm.grad[:, 3] == 0).all())


def test_two_calls_return_the_same_bits(case):
    from diffsdfsim_amd import pointcloud
    T = case["t"]
    again = pointcloud._launch(T["pts"], torch.tensor(case["seg_off"], dtype=torch.int32, device=T["pts"].device),
                               int(np.diff(case["seg_off"]).max()), T["pose"], T["types"], T["prm"])
    assert torch.equal(again, case["raw"])


@pytest.mark.parametrize("kind", ["SHAPE_IGR", "SHAPE_GRID"])
def test_neural_and_grid_bodies_are_refused_and_out_is_left_alone(case, kind):
    import ctypes
    from diffsdfsim_amd import _lib, pointcloud, world_abi
    T = case["t"]
    dev = T["pts"].device
    types = T["types"].clone()
    types[4] = getattr(world_abi, kind)
    off = torch.tensor(case["seg_off"], dtype=torch.int32, device=dev)
    nseg, max_len = types.numel(), int(np.diff(case["seg_off"]).max())
    L = _lib.lib()
    out = torch.full((nseg, 12), -7.0, dtype=torch.float64, device=dev)
    nbytes = L.dss_pointcloud_loss_workspace_bytes(nseg, max_len)
    assert nbytes == nseg * 3 * 12 * 8      # ceil(4133 / 2048) partials per segment
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    rc = L.dss_pointcloud_loss(nseg, max_len, _lib.ptr(off), _lib.ptr(T["pts"]), _lib.ptr(T["pose"]), _lib.ptr(types), _lib.ptr(T["prm"]),
                               _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == -7.0).all())
    with pytest.raises(_lib.HipLibraryError):
        pointcloud.match_pointcloud(T["pts"], case["seg_off"], T["pose"], types, T["prm"])


def test_cpu_tensors_are_refused(case):
    from diffsdfsim_amd import _lib, pointcloud
    with pytest.raises(_lib.HipLibraryError):
        pointcloud.match_pointcloud(torch.tensor(case["pts"]), case["seg_off"], torch.tensor(case["pose"]), case["shape_type"], torch.tensor(case["prm"]))


def test_body_pointcloud_loss_is_the_single_segment_call(case):
    from diffsdfsim_amd.physics3d import SDFBoxRounded
    names, off = list(case["names"]), case["seg_off"]
    s = names.index("rounded_257")
    dims = torch.tensor(case["prm"][s, :3], dtype=torch.float64, requires_grad=True)
    pose = torch.tensor(case["pose"][s], dtype=torch.float64, requires_grad=True)
    body = SDFBoxRounded(pose, dims, float(case["prm"][s, 3]))
    loss, count = body.pointcloud_loss(case["pts"][off[s]:off[s + 1]])
    loss.backward()
    # one segment of 257 points is one chunk, summed by the same lanes as in the batched call -> the same bits
    assert float(loss) == float(case["raw"][s, 0]) and float(count) == float(case["raw"][s, 1])
    assert np.array_equal(pose.grad.numpy(), case["raw"][s, 2:9].cpu().numpy()) and np.array_equal(dims.grad.numpy(), case["raw"][s, 9:12].cpu().numpy())
