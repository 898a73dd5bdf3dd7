"""Fit the samples of a 2-D grid body to an observation: a plain Adam loop over rollouts of `physics2d.World`.

The gradient reaches the samples through the contacts (query path and outline path, `sdf_contacts`) and through the inertia
(`sdf_bodies`).  The body is rebuilt from the current samples every iteration, so the outline's topology (which grid sides are
crossed, which vertices are snapped) follows the samples; within one iteration it is a constant, as `sdf_bodies` defines."""
import torch


def fit_grid(make_world, sdf0, target, steps, iters, lr=1e-3):
    """make_world(sdf) -> (world, observe): a fresh world one of whose bodies is `SDFGrid(..., sdf=sdf)`, and a function that
    returns the observation of that world (a tensor shaped like `target`) after the rollout.  Every iteration steps a fresh
    world `steps` times, takes the squared error of the observation against `target` and one Adam step on the samples.
    Returns the loss history (one number per iteration, taken before its step) and the final samples [n0, n1]."""
    sdf = torch.as_tensor(sdf0).detach().clone().to(torch.float64).requires_grad_(True)
    target = torch.as_tensor(target)
    opt = torch.optim.Adam([sdf], lr=lr)
    history = []
    for _ in range(iters):
        opt.zero_grad()
        world, observe = make_world(sdf)
        for _ in range(steps):
            world.step()
        seen = observe()
        loss = ((seen - target.to(seen)) ** 2).sum()
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    return history, sdf.detach().clone()
