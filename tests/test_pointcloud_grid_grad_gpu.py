"""GPU: dss_pointcloud_loss_grids_adjoint (csrc/pointcloud_loss_grid_adj.hip) -- the gradient of the point-cloud loss with respect
to a voxel grid's samples -- against tests/pointcloud_grid_grad_ref.py (float64 per point, every sample's sum exact), from the
raw call up to SDFGrid3D.pointcloud_loss and experiments.fit_pointcloud_grid.  The cases: pointcloud_grid_grad_helpers.

Tolerance: |g - ref| <= 1e-12 x (the sample's abs-sum, sum |term|); a sample that no point reaches is exactly 0.  A term is
computed by the kernel and by the reference with the same float64 operations, so the two differ by the summation alone: the
reference's sum is exact, the kernel's atomic adds arrive in any order, and a float64 sum of n terms in any order is within
(n - 1) 2^-53 of the abs-sum -- below 1e-12 while n < about 9000.  Every sample here gets at most 4096 terms (asserted).  Two runs of
the kernel agree within the same bound, 1e-12 x abs-sum.
"""

import numpy as np
import pytest
import torch

import pointcloud_grid_grad_helpers as H
import pointcloud_grid_grad_ref as ref

pytestmark = pytest.mark.gpu


def _prepare(case):
    from diffsdfsim_amd.grids import GridTable
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
    c = dict(case)
    c["ref"] = ref.loss_and_grad(case["pts"], case["seg_off"], case["pose"], case["shape_type"], case["prm"], case["grid_id"], case["grids"], case["g_sum"])
    c["table"] = GridTable(case["grids"], dev)
    c["t"] = dict(pts=t(case["pts"]), off=t(case["seg_off"], torch.int32), pose=t(case["pose"]), types=t(case["shape_type"], torch.int32),
                  prm=t(case["prm"]), gid=t(case["grid_id"], torch.int32), w=t(case["g_sum"]))
    c["max_len"] = int(np.diff(case["seg_off"]).max())
    c["flat"] = lambda key: np.concatenate([a.reshape(-1) for a in c["ref"][key]])
    return c


@pytest.fixture(scope="module")
def mixed():
    return _prepare(H.mixed_case())


@pytest.fixture(scope="module")
def one_cell():
    return _prepare(H.one_cell_case())


def _raw(c, g_data, **over):
    """The C call on the case's device tensors (over: replacements); -> status."""
    from diffsdfsim_amd import _lib
    T, tab = dict(c["t"], **over), c["table"]
    L = _lib.lib()
    rc = L.dss_pointcloud_loss_grids_adjoint(over.get("nseg", T["types"].numel()), c["max_len"], _lib.ptr(T["off"]), _lib.ptr(T["pts"]), _lib.ptr(T["pose"]),
                                             _lib.ptr(T["types"]), _lib.ptr(T["prm"]), _lib.ptr(T["gid"]), over.get("ngrid", tab.ngrid), _lib.ptr(tab.off),
                                             _lib.ptr(over.get("dims", tab.dims)), _lib.ptr(tab.data), _lib.ptr(T["w"]), _lib.ptr(g_data),
                                             _lib.stream_ptr(g_data.device))
    torch.cuda.synchronize()
    return rc


def _check(c, got, label):
    want, mag, n = c["flat"]("grad"), c["flat"]("abs_sum"), c["flat"]("terms")
    assert n.max() <= 4096, n.max()
    err = np.abs(got - want)
    worst = float((err[mag > 0] / mag[mag > 0]).max())
    print("%s: %d samples reached, at most %d terms each, worst |g - ref| / abs-sum = %.2e" % (label, int((n > 0).sum()), int(n.max()), worst))
    assert np.all(got[n == 0] == 0.0), "a sample without a contribution is not exactly 0"
    assert np.all(err <= 1e-12 * mag), worst
    return worst


def test_mixed_call_matches_the_reference_and_a_second_run_agrees(mixed):
    g1, g2 = torch.zeros_like(mixed["table"].data), torch.zeros_like(mixed["table"].data)
    assert _raw(mixed, g1) == 0 and _raw(mixed, g2) == 0
    a, b = g1.cpu().numpy(), g2.cpu().numpy()
    _check(mixed, a, "mixed")
    mag = mixed["flat"]("abs_sum")
    assert np.all(np.abs(a - b) <= 1e-12 * mag)
    off, n = mixed["table"].off.cpu().numpy(), mixed["flat"]("terms")
    assert np.all(a[off[1]:off[2]] == 0.0) and n[off[1]:off[2]].max() == 0            # the grid no segment uses
    for k in (0, 2, 3):
        assert n[off[k]:off[k + 1]].max() > 0                                         # every other grid is reached
    # the segment of exactly 64 points: all of them count, and the 4x3x2 grid hears of no other segment
    assert mixed["seg_off"][-1] - mixed["seg_off"][-2] == 64 and mixed["ref"]["count"][-1] == 64 and mixed["g_sum"][-1] != 0
    assert n[off[4]:].sum() == 64 * 8 and n[off[4]:].min() > 0 and np.all(a[off[4]:] != 0.0)
    # the points at 1 + 2^-40 and the segment of weight 0 are in the call and in the reference alike; the points with |u_d| = 1
    # reach the last layer of the 9^3 grid
    last = mixed["ref"]["terms"][3]
    assert last[8].max() > 0 and last[0].max() > 0 and last[:, 8].max() > 0 and last[:, :, 0].max() > 0


def test_4096_points_in_one_cell(one_cell):
    g = torch.zeros_like(one_cell["table"].data)
    assert _raw(one_cell, g) == 0
    n = one_cell["flat"]("terms")
    assert int((n > 0).sum()) == 8 and n.max() == 4096
    _check(one_cell, g.cpu().numpy(), "one cell")


def test_a_prefilled_g_data_comes_back_as_prefill_plus_gradient(mixed):
    fill = torch.linspace(-2.0, 3.0, mixed["table"].data.numel(), dtype=torch.float64, device="cuda:0")
    g = fill.clone()
    assert _raw(mixed, g) == 0
    want, mag, f = mixed["flat"]("grad"), mixed["flat"]("abs_sum"), fill.cpu().numpy()
    got = g.cpu().numpy()
    assert np.array_equal(got[mag == 0], f[mag == 0])
    # the pre-fill is one more term of the sum: n + 1 terms of abs-sum |fill| + mag
    assert np.all(np.abs(got - (f + want)) <= 1e-12 * (np.abs(f) + mag))


@pytest.mark.parametrize("what", ["nseg", "ngrid", "null_g_sum", "null_seg_off", "grid_id_past_table", "dim_1", "neural", "grid_without_grid"])
def test_refused_calls_leave_g_data_untouched(mixed, what):
    T = mixed["t"]
    empty = torch.zeros(0, dtype=torch.float64, device="cuda:0")      # (_lib.ptr: a null pointer)
    over, bad_arg = {}, True
    if what == "nseg":
        over = dict(nseg=0)
    elif what == "ngrid":
        over = dict(ngrid=-1)
    elif what == "null_g_sum":
        over = dict(w=empty)
    elif what == "null_seg_off":
        over = dict(off=empty.to(torch.int32))
    elif what == "grid_id_past_table":
        ids = T["gid"].clone(); ids[2] = 5
        over = dict(gid=ids)
    elif what == "dim_1":
        dims = mixed["table"].dims.clone(); dims[1, 2] = 1
        over = dict(dims=dims)
    elif what == "neural":
        types = T["types"].clone(); types[4] = 6
        over, bad_arg = dict(types=types), False
    else:
        ids = T["gid"].clone(); ids[2] = -1
        over, bad_arg = dict(gid=ids), False
    g = torch.full_like(mixed["table"].data, -7.0)
    rc = _raw(mixed, g, **over)
    assert rc == (-1 if bad_arg else -3), rc      # DSS_E_BADARG / DSS_E_UNSUPPORTED, as dss_pointcloud_loss_grids answers
    assert bool((g == -7.0).all())
    if what == "nseg":      # a null g_data with grids in the table
        assert _raw(mixed, empty) == -1


def test_autograd_path_returns_the_detached_calls_bits_and_the_sample_gradient(mixed):
    from diffsdfsim_amd import pointcloud
    from diffsdfsim_amd.grids import GridTable
    T = mixed["t"]
    grids = [torch.tensor(g, device="cuda:0", requires_grad=(k != 1)) for k, g in enumerate(mixed["grids"])]
    live = GridTable(grids, "cuda:0")
    assert live.data.requires_grad and not mixed["table"].data.requires_grad
    out = []
    for table in (mixed["table"], live):
        pose = T["pose"].clone().requires_grad_()
        loss, count = pointcloud.match_pointcloud(T["pts"], mixed["seg_off"], pose, mixed["shape_type"], T["prm"], grids=table, grid_id=mixed["grid_id"])
        (loss * T["w"]).sum().backward()
        out.append((loss.detach(), count, pose.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert grids[1].grad is None
    got = np.concatenate([(torch.zeros_like(g) if g.grad is None else g.grad).cpu().numpy().reshape(-1) for g in grids])
    _check(mixed, got, "autograd")
    assert np.allclose(out[1][0].cpu().numpy()[mixed["shape_type"] == 7], mixed["ref"]["loss"][mixed["shape_type"] == 7], rtol=1e-12, atol=0)


def test_grid_body_fills_the_samples_gradient_and_follows_their_updates():
    from diffsdfsim_amd.physics3d import SDFGrid3D
    case = H.small_case()
    lo, hi = case["seg_off"][0], case["seg_off"][1]
    g = np.linspace(-1.0, 1.0, 7)
    ball = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) - 0.6      # (the body's mesh needs a surface)
    one = dict(case, pts=case["pts"][lo:hi], seg_off=np.array([0, hi - lo]), pose=case["pose"][:1], shape_type=case["shape_type"][:1],
               prm=case["prm"][:1], grid_id=np.array([0], np.int32), g_sum=np.ones(1),
               grids=[ball + 0.05 * np.random.default_rng(3).standard_normal((7, 7, 7))])
    sdf = torch.tensor(one["grids"][0], requires_grad=True)
    body = SDFGrid3D(torch.tensor(one["pose"][0]), float(one["prm"][0, 3]), sdf)
    for step in range(2):
        r = _prepare(one)["ref"]
        sdf.grad = None
        loss, count = body.pointcloud_loss(one["pts"])
        loss.backward()
        assert sdf.grad is not None and float(count) == r["count"][0] > 0
        assert np.all(np.abs(sdf.grad.numpy() - r["grad"][0]) <= 1e-12 * r["abs_sum"][0])
        assert abs(float(loss.detach()) - r["loss"][0]) <= 1e-12 * r["loss"][0]
        with torch.no_grad():      # an optimiser's step: in place, the body keeps the tensor
            sdf.data += 0.05 * torch.cos(torch.arange(sdf.numel(), dtype=torch.float64)).reshape(sdf.shape)
        one["grids"] = [sdf.detach().numpy().copy()]
    # a body whose samples need no gradient keeps its table
    still = SDFGrid3D(torch.tensor(one["pose"][0]), float(one["prm"][0, 3]), one["grids"][0])
    still.pointcloud_loss(one["pts"])
    assert still._grid_table is not None and getattr(body, "_grid_table", None) is None


@pytest.mark.parametrize("observe", ["vertices", "depth"])
def test_driver_lowers_every_scenes_loss(observe):
    from diffsdfsim_amd import experiments
    res = experiments.fit_pointcloud_grid("sphere", target_rad=[0.8, 1.0], start_rad=[1.1, 0.75], res=17, max_iter=30, max_points=300, observe=observe)
    for s in range(2):
        print("fit_pointcloud_grid [%s] scene %d: loss %.4e -> %.4e (ratio %.3f), chamfer %.4e -> %.4e" %
              (observe, s, res["loss_start"][s], res["loss_final"][s], res["loss_final"][s] / res["loss_start"][s], res["chamfer_start"][s],
               res["chamfer_final"][s]))
    for key in ("loss_start", "loss_final", "chamfer_start", "chamfer_final"):
        assert np.all(np.isfinite(res[key])), key
    assert np.all(res["loss_final"] < res["loss_start"])
    assert len(res["history"]) == 31 and np.isfinite(res["sdf"]).all()
    assert len(res["observations"]["scene"]) == 6 and np.diff(res["observations"]["seg_off"]).max() <= 300
