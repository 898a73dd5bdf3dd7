"""How the seed of tests/test_igr_shapenet_gpu.py was chosen (TEST INFRASTRUCTURE, numpy only: tests/implicit_net.py).

MeshSDF's rule -- the reference's (sdf_physics/physics3d/bodies.py:687-694) and this project's -- moves a vertex of the
level-set mesh by -n d phi / d latent.  That is the derivative of the zero level set of a DISTANCE function.  For a general
phi the surface moves by -n (d phi / d latent) / |grad phi|, which is what central differences of the whole pipeline see.
A geometric-init network is no distance function (|grad phi| on its surface ranges over 0.5 .. 1.3, differently for every
seed), so a check of the rule's implementation against central differences means something only for weights on which
the two agree.  ``rule_vs_true`` evaluates both as surface integrals, for the two losses the GPU tests differentiate:

    d trace(J) / d latent         J = inertia of the solid {phi < 0} at mass 1 about its centre of mass
    d |omega|^2 / d latent        omega = J^-1 tau T: the spin scene's angular velocity (gyroscopic term left out)

A shape derivative is  d/d theta int_Omega f dV = int_S f v_n dS  with the normal velocity v_n = -(d phi / d theta) /
|grad phi| (true) or -(d phi / d theta) (the rule).  The surface is sampled along rays from the origin (the solids are
star-shaped about it; bisection to phi = 0), dS = R^2 d Omega / (n . d), the volume integrals are sums over the same rays.

``python tests/igr_seed_choice.py [first] [last]`` prints the table the choice was made from: seed 126 has the smallest
largest relative disagreement of seeds 0 .. 159 (tests/test_igr_seed_choice_cpu.py pins it)."""
import sys

import numpy as np

import implicit_net as IN

LATENT = (0.05, -0.08, 0.06, -0.04)
TORQUE = (0.3, 0.5, -0.2)


def rule_vs_true(seed, latent=LATENT, torque=TORQUE, radius_init=0.6, rays=3000):
    """-> {loss: (true [4], rule [4])} for loss in ("trace", "spin"), or None if the surface leaves the unit cube."""
    lat, tau = np.asarray(latent, np.float64), np.asarray(torque, np.float64)
    Ws, bs = IN.geometric_init(seed=seed, radius_init=radius_init, **IN.SHAPENET)
    d = np.random.default_rng(0).standard_normal((rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dO = 4 * np.pi / rays
    lo, hi = np.full(rays, 0.02), np.full(rays, 1.7)
    for _ in range(36):
        mid = 0.5 * (lo + hi)
        inside = IN.query(d * mid[:, None], lat, Ws, bs, jacobian=False) < 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    R = 0.5 * (lo + hi)
    if R.max() > 0.97:
        return None
    x = d * R[:, None]
    _, gl, gx = IN.query(x, lat, Ws, bs)
    gn = np.linalg.norm(gx, axis=1)
    dS = R ** 2 * dO / np.abs((gx / gn[:, None] * d).sum(1))
    V = (R ** 3 / 3).sum() * dO
    c = (d * (R ** 4 / 4)[:, None]).sum(0) * dO / V
    S2 = np.einsum("ni,nj,n->ij", d, d, R ** 5 / 5) * dO / V - np.outer(c, c)
    J = np.trace(S2) * np.eye(3) - S2
    y = x - c
    om = np.linalg.solve(J, tau)
    a = np.linalg.solve(J, om)
    weight = {"trace": (2 * (y ** 2).sum(1) - np.trace(J)) / V,
              "spin": -2 * ((y ** 2).sum(1) * (om @ a) - (y @ om) * (y @ a) - om @ J @ a) / V}
    return {k: (-(w[:, None] * gl / gn[:, None] * dS[:, None]).sum(0), -(w[:, None] * gl * dS[:, None]).sum(0))
            for k, w in weight.items()}


def disagreement(res):
    """Largest |rule - true| / |true| over both losses and the four latent coordinates."""
    return max(float((np.abs(t - r) / np.abs(t)).max()) for t, r in res.values())


if __name__ == "__main__":
    first, last = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (0, 160)
    for seed in range(first, last):
        res = rule_vs_true(seed)
        if res is None:
            print(seed, "surface leaves the cube")
            continue
        print(seed, "disagreement %.3f" % disagreement(res), "d trace J: true", np.round(res["trace"][0], 4), "rule",
              np.round(res["trace"][1], 4), flush=True)
