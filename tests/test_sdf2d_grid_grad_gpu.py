"""GPU: dss_sdf2d_contacts_backward_grids on the device library and the 2-D world on it: the golden comparisons, the table
seams, the shared-grid sum, determinism, and the gradient of a rollout with respect to a grid's samples against central
differences (bounds and scenes of test_sdf2d_grid_grad_cpu.py and sdf2d_grid_grad_helpers.py)."""
import pytest
import torch

import sdf2d_grid_grad_helpers as GH
import test_sdf2d_grid_grad_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_kernel_against_the_reference_autograd():
    worst = C.GH_golden_contacts(None, DEV)
    print("kernel g_vals, g_grads chained to the samples, largest error relative to the pair's largest gradient: %.3e" % worst)


@pytest.mark.parametrize("name", sorted(GH.seam_scenes()))
def test_table_seams_and_the_shared_grid_sum(name, monkeypatch):
    from diffsdfsim_amd.physics2d import world as world2d
    monkeypatch.setattr(world2d.Defaults, "DEVICE", torch.device("cpu"))      # (the restatement's bodies are built on the host)
    C.GH_seam(None, name, DEV)


def test_a_pair_flagged_over_cap_contributes_nothing():
    from diffsdfsim_amd.physics2d import sdf_contacts
    C.GH_over_cap(sdf_contacts.DEVICE_KERNELS, DEV)


def test_two_calls_are_bit_identical_and_the_pose_gradients_are_those_of_the_old_entry():
    pairs, samples = GH.seam_scenes()["two_grids"]
    pairs = pairs[:2]      # grid 1 in pair 0, grid 0 in pair 1: no grid shared
    runs = [GH.run_scene(None, pairs, samples, DEV) for _ in range(2)]
    for x, y in zip(GH.table_grads(runs[0][1]), GH.table_grads(runs[1][1])):
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and max(float(u.abs().max()) for u in x) > 0.0
    a = runs[0][0]
    a0, _, _, _ = GH.run_scene(None, pairs, samples, DEV, grad_tab=False)      # the table needs no grad: the old entry
    assert all(torch.equal(a[k].grad, a0[k].grad) for k in ("pose", "prm", "scale")) and float(a["pose"].grad.abs().max()) > 0.0


def test_world_rollout_leaves_a_gradient_on_the_samples():
    """The scene, the finite differences and the bound of the CPU test of the same name, on the device."""
    GH.world_gradient_check(DEV)


def test_fit_grid_lowers_the_loss():
    GH.fit_check(DEV)
