"""GPU: the 2-D SDF contact kernels on the device library (csrc/sdf2d_contacts.hip) against what the reference produced
(tests/golden/sdf2d_contacts.npz, sdf2d_contacts_grad.npz; bounds of sdf2d_helpers.py) and against the emulator build of the
same source (counts and (direction, edge) bit-equal), in one launch and in launches of 1, 63, 64 and 65 pairs."""
import numpy as np
import pytest
import torch

import sdf2d_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_forward_against_the_reference_in_one_launch():
    from diffsdfsim_amd.physics2d import sdf_contacts2d
    g = H.golden("sdf2d_contacts")
    idx = np.arange(len(g["count"]))
    cap, ccap = int(g["count"].max()), int(g["ncand"].max()) + 1
    out, count, tag, tpar, ncand, cand, cand_tag = sdf_contacts2d(eps=float(g["eps"]), cap=cap, candidates=ccap, **H.inputs(g, idx, DEV))
    worst = H.compare_contacts(g, idx, out, count, tag, ncand.cpu(), cand.cpu(), cand_tag.cpu())
    print("largest tuple error over the coordinate magnitude: %.3e" % worst)
    again = sdf_contacts2d(eps=float(g["eps"]), cap=cap, candidates=ccap, **H.inputs(g, idx, DEV))
    assert all(torch.equal(x, y) for x, y in zip((out, count, tag, tpar, ncand, cand, cand_tag), again))


@pytest.mark.parametrize("P", [1, 63, 64, 65])
def test_launches_of_few_pairs_and_the_emulator_bit_for_bit(P):
    from diffsdfsim_amd.physics2d import sdf_contacts, sdf_contacts2d
    from emu import emu
    g = H.golden("sdf2d_contacts")
    idx = (np.arange(P) * 5 + P) % len(g["count"])
    out, count, tag, tpar = sdf_contacts2d(eps=float(g["eps"]), cap=40, **H.inputs(g, idx, DEV))
    H.compare_contacts(g, idx, out, count, tag)
    e_out, e_count, e_tag, e_tpar = sdf_contacts2d(eps=float(g["eps"]), cap=40, kernels=sdf_contacts.host_kernels(emu.lib()), **H.inputs(g, idx))
    assert torch.equal(count.cpu(), e_count) and torch.equal(tag.cpu(), e_tag)
    assert (out.cpu() - e_out).abs().max() <= 1e-12 * max(H.magnitude(g, p) for p in idx)
    # the grad file at the same launch size: forward and backward against the reference's autograd
    gg = H.golden("sdf2d_contacts_grad")
    ix = (np.arange(P) * 3 + P) % len(gg["count"])
    a = H.inputs(gg, ix, DEV, grad=True)
    out, count, tag, tpar = sdf_contacts2d(eps=float(gg["eps"]), cap=gg["out"].shape[1], **a)
    H.compare_contacts(gg, ix, out, count, tag)
    (out * torch.tensor(H.gout_in_kernel_order(gg, ix, count, tag), device=DEV)).sum().backward()
    H.compare_gradients(gg, ix, a, nontrivial=P >= 63)


def test_backward_against_the_reference_autograd():
    from diffsdfsim_amd.physics2d import sdf_contacts2d
    g = H.golden("sdf2d_contacts_grad")
    idx = np.arange(len(g["count"]))
    a = H.inputs(g, idx, DEV, grad=True)
    out, count, tag, tpar = sdf_contacts2d(eps=float(g["eps"]), cap=g["out"].shape[1], **a)
    H.compare_contacts(g, idx, out, count, tag)
    gout = H.gout_in_kernel_order(g, idx, count, tag)
    (out * torch.tensor(gout, device=DEV)).sum().backward()
    worst = H.compare_gradients(g, idx, a)
    print("largest gradient error, relative to the pair's largest gradient: %.3e" % worst)


def test_capacity_error_and_cpu_tensors_are_refused():
    from diffsdfsim_amd import _lib
    from diffsdfsim_amd.physics2d import sdf_contacts2d
    g = H.golden("sdf2d_contacts")
    big = int(np.argmax(g["count"]))
    idx = np.array([0, big, 1])
    with pytest.raises(RuntimeError, match="capacity"):
        sdf_contacts2d(eps=float(g["eps"]), cap=int(g["count"][big]) - 1, **H.inputs(g, idx, DEV))
    out, count, tag, _ = sdf_contacts2d(eps=float(g["eps"]), cap=int(g["count"][big]), **H.inputs(g, idx, DEV))
    H.compare_contacts(g, idx, out, count, tag)
    with pytest.raises(_lib.HipLibraryError):
        sdf_contacts2d(eps=float(g["eps"]), **H.inputs(g, idx))


def _scene(name):
    from diffsdfsim_amd.physics2d import Gravity, SDFCircle, SDFGrid, SDFRect
    kw = dict(restitution=0.5, fric_coeff=0.9)
    floor = SDFRect([500, 600], [1000, 50], **kw)
    if name == "circle_on_rect":
        leaf = torch.tensor(20.0, dtype=torch.double, requires_grad=True)
        mover = SDFCircle([500, 480], leaf, vel=[0, 30, 0], **kw)
        loss = lambda: (mover.pos ** 2).sum()      # noqa: E731
    elif name == "tilted_rect":
        leaf = torch.tensor(80.0, dtype=torch.double, requires_grad=True)
        mover = SDFRect([0.3, 420, 520], torch.stack([leaf, leaf.new_tensor(50.0)]), **kw)
        loss = lambda: (mover.p ** 2).sum()      # noqa: E731
    else:
        leaf = torch.tensor(100.0, dtype=torch.double, requires_grad=True)
        mover = SDFGrid([500, 520], leaf, H.golden("sdf2d_rollouts")["grid_disc_samples"], vel=[2.0, 20, 0], **kw)
        loss = lambda: (mover.p ** 2).sum()      # noqa: E731
    mover.add_force(Gravity(g=100))
    return [floor, mover], leaf, loss


@pytest.mark.parametrize("name,nsteps", [("circle_on_rect", 50), ("tilted_rect", 40), ("grid_disc", 30)])
def test_rollouts_against_the_reference_world(name, nsteps):
    """physics2d.World with SDF bodies against the reference's World with its SDFContactHandler (sdf2d_rollouts.npz): the same
    contact pairs every step, the same number of sub-steps, poses to 1e-7 along the way and 1e-8 at the end, loss to 1e-8,
    gradient to 1e-5 -- the bounds tests/test_contacts2d_gpu.py holds its 2-D worlds to."""
    from diffsdfsim_amd.physics2d import TotalConstraint, World
    g = H.golden("sdf2d_rollouts")
    bodies, leaf, loss = _scene(name)
    w = World(bodies, [TotalConstraint(bodies[0])], dt=1.0 / 30)
    for k in range(nsteps):
        w.step()
        want = [tuple(r) for r in g[name + "_pairs"][k] if r[0] >= 0]
        assert [(c[1], c[2]) for c in w.contacts] == want, (k, want)
        p = torch.cat([b.p for b in bodies]).detach().cpu().numpy()
        assert np.abs(p - g[name + "_traj_p"][k]).max() < 1e-7 * np.abs(g[name + "_traj_p"][k]).max(), k
    assert np.abs(p - g[name + "_traj_p"][-1]).max() < 1e-8 * np.abs(p).max()
    assert len(w.trajectory) == int(g[name + "_n_substeps"])
    total = loss()
    (gr,) = torch.autograd.grad(total, [leaf])
    print("%s: loss %.9f (reference %.9f), gradient %.9f (reference %.9f)" % (name, float(total), g[name + "_loss"], float(gr), g[name + "_grad"]))
    assert abs(float(total) - float(g[name + "_loss"])) < 1e-8 * abs(float(g[name + "_loss"]))
    assert abs(float(gr) - float(g[name + "_grad"])) < 1e-5 * abs(float(g[name + "_grad"])), (float(gr), float(g[name + "_grad"]))


def _bowl_world(rad):
    import math
    from diffsdfsim_amd.physics2d import Gravity, SDFBowl, SDFCircle, TotalConstraint, World
    kw = dict(restitution=0.5, fric_coeff=0.9)
    bowl, ball = SDFBowl([math.pi, 500, 500], 100.0, 10.0, **kw), SDFCircle([470, 505], rad, **kw)
    ball.add_force(Gravity(g=100))
    return World([bowl, ball], [TotalConstraint(bowl)], dt=1.0 / 30), bowl, ball


def test_circle_dropped_into_a_pinned_bowl_against_the_reference_world():
    """The non-convex body in a world: a circle dropped off-centre into a pinned bowl, 45 steps.  The reference can step this
    world only without grad (its hull refuses tensors that require grad and the pair's contacts span two dimensions), so contact
    pairs, sub-steps, poses (1e-7 along the way, 1e-8 at the end) and loss (1e-8) are the reference's, and d loss / d rad of
    this build is held to central differences of this build.  Bound of that comparison, h = 1e-3: rounding 1e-12 x loss / h =
    5e-7, truncation h^2 x loss / rad^3 = 6e-5, both absolute: 1e-4 absolute, or 1e-4 of the gradient where that is larger."""
    g = H.golden("sdf2d_rollouts")
    name = "circle_in_bowl"
    rad = torch.tensor(20.0, dtype=torch.double, requires_grad=True)
    w, bowl, ball = _bowl_world(rad)
    touched = 0
    for k in range(45):
        w.step()
        want = [tuple(r) for r in g[name + "_pairs"][k] if r[0] >= 0]
        assert [(c[1], c[2]) for c in w.contacts] == want, (k, want)
        touched += bool(want)
        p = torch.cat([bowl.p, ball.p]).detach().cpu().numpy()
        assert np.abs(p - g[name + "_traj_p"][k]).max() < 1e-7 * np.abs(g[name + "_traj_p"][k]).max(), k
    assert touched >= 5 and len(w.trajectory) == int(g[name + "_n_substeps"])
    assert np.abs(p - g[name + "_traj_p"][-1]).max() < 1e-8 * np.abs(p).max()
    loss = (ball.pos ** 2).sum()
    assert abs(float(loss.detach()) - float(g[name + "_loss"])) < 1e-8 * abs(float(g[name + "_loss"]))
    # the ball's position alone does not feel its radius in this world (measured: d / d rad = 1e-8, differences 0); its spin
    # does, through the arm of the friction force, so the differentiated loss adds the angle, weighted to the positions' size
    (ad,) = torch.autograd.grad(loss + 1e4 * ball.p[0] ** 2, [rad])
    vals = []
    for h in (1e-3, -1e-3):
        w2, _, ball2 = _bowl_world(torch.tensor(20.0 + h, dtype=torch.double))
        with torch.no_grad():
            for _ in range(45):
                w2.step()
        vals.append(float((ball2.pos ** 2).sum() + 1e4 * ball2.p[0] ** 2))
    fd = (vals[0] - vals[1]) / 2e-3
    print("circle_in_bowl: d loss / d rad %.9f, central differences %.9f" % (float(ad), fd))
    assert fd != 0.0 and abs(float(ad) - fd) < 1e-4 * max(1.0, abs(fd)), (float(ad), fd)


def test_world_of_sdf_bodies_steps_on_the_device():
    """A ball of SDFCircle dropped on an SDFRect slab in physics2d.World: the pair goes to the SDF kernel, the ball comes to
    rest on the slab (its lowest point within eps of the slab's top), and the loss has a gradient with respect to the radius."""
    from diffsdfsim_amd.physics2d import Gravity, SDFCircle, SDFRect, TotalConstraint, World
    rad = torch.tensor(20.0, dtype=torch.double, requires_grad=True)
    floor = SDFRect([500, 600], [1000, 50], restitution=0.5, fric_coeff=0.9)
    ball = SDFCircle([500, 480], rad, vel=[0, 30, 0], restitution=0.5, fric_coeff=0.9)
    ball.add_force(Gravity(g=100))
    w = World([floor, ball], [TotalConstraint(floor)], dt=1.0 / 30)
    seen = 0
    for _ in range(50):
        w.step()
        seen = max(seen, len(w.contacts))
        assert all((c[1], c[2]) == (0, 1) for c in w.contacts)
    assert seen >= 1 and w.lcp_calls > 0
    assert float(ball.pos[1]) + 20.0 <= 575.0 + 0.1 and float(ball.pos[1]) > 480.0
    assert np.abs(floor.p.detach().cpu().numpy() - np.array([0.0, 500.0, 600.0])).max() < 1e-9
    (g,) = torch.autograd.grad((ball.pos ** 2).sum(), [rad])
    assert np.isfinite(float(g)) and abs(float(g)) > 1.0
