"""Generate tests/golden/mesh_chain.npz: the reference's autograd through get_ang_inertia and through the MeshSDF backward.

Run in the build container only:  python -m oracle.gen.gen_mesh_chain_golden

(a) Inertia, for every mesh of tests/mesh_cases.py (the meshes themselves are rebuilt by the tests, never stored):
    <name>_J      get_ang_inertia(verts, faces, mass) (`sdf_physics/physics3d/bodies.py:380-395`), float64
    <name>_g      d(sum gJ * J)/d verts by torch autograd, at the rows <name>_rows (all rows of a small mesh)
    <name>_dref   max|g_perm - g| / max|g| with the face rows in a seeded random permutation: the same value
                  mathematically, so the reference's own sensitivity to the order of its sums
    <name>_vol    the volume by signed tetrahedra in exact rational arithmetic (mesh_cases.exact_volume; not the
                  reference's code)
(b) MeshSDF backward (`bodies.py:653-704`), for every body type whose level-set mesh the reference builds through
    _diff_marching_cubes: on a strided subset of 600 of the reference's unit vertices that keeps KINK_MARGIN away from the
    kinks of the SDF,
    <type>_prm    unit parameters as dss_meshsdf_backward takes them (dims/scale ... and fourth the corner radius/scale)
    <type>_verts  the subset, <type>_gbar a seeded cotangent on it
    <type>_g      [prefixes, 4] the reference's parameter gradient of sum gbar * verts with gbar zero outside the first nv
                  subset vertices, nv in mesh_cases.PREFIXES, in the parameter order of <type>_prm
    <type>_S      [prefixes, 4] sum_v |dl_v * d phi / d theta_i (v)|, the scale of the tolerance
    The bowl is not stored: bowl_sdf shifts its points in place, and MeshSDF.backward hands it the saved vertices as a
    leaf that requires grad, so the reference's own backward raises for it (the run prints the error).
    The reference groups the rounded box's parameters as (r/scale, (dims - 2 r)/scale) = (r', e'); the kernel takes
    (dims/scale, r/scale) = (e' + 2 r', r'), so d/d dims' = d/d e' and d/d r' at fixed dims' = d/d r' - 2 sum_i d/d e'_i.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
from sdf_physics.physics3d.bodies import (SDF3D, SDFBowl, SDFBox, SDFBoxRounded, SDFBrick, SDFCylinder, SDFSphere,  # noqa: E402
                                          get_ang_inertia)
from torch.nn.functional import normalize  # noqa: E402

import mesh_cases as MC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mesh_chain.npz")
T = lambda a: torch.tensor(a, dtype=torch.double)


def inertia_grad(v, f, mass, gJ):
    vt = T(v).requires_grad_()
    J = get_ang_inertia(vt, torch.tensor(f), T(mass))
    (J * T(gJ)).sum().backward()
    return J.detach().numpy(), vt.grad.numpy()


def inertia_cases(out):
    for name in MC.NAMES:
        v, f, mass, gJ = MC.case(name)
        J, g = inertia_grad(v, f, mass, gJ)
        perm = np.random.default_rng(3000 + MC.NAMES.index(name)).permutation(len(f))
        _, gp = inertia_grad(v, f[perm], mass, gJ)
        dref = np.abs(gp - g).max() / np.abs(g).max()
        rows = MC.stored_rows(name, v, f)
        out[name + "_J"], out[name + "_g"], out[name + "_rows"] = J, g[rows], rows.astype(np.int32)
        out[name + "_dref"], out[name + "_vol"] = dref, MC.exact_volume(v, f)
        print("%-12s nf %5d  d_ref %.2e  vol %.15g" % (name, len(f), dref, out[name + "_vol"]))


def to_kernel_order(name, cols):
    """cols: one [..] array per reference parameter entry, flattened in the reference's order -> the kernel's order."""
    if name == "rounded":           # reference (r', e'[3]) -> kernel (dims'[3], r')
        r, e = cols[0], cols[1:4]
        return list(e) + [r - 2.0 * (e[0] + e[1] + e[2])]
    return list(cols)


def meshsdf_cases(out):
    dt = lambda x: torch.tensor(x, dtype=torch.double)
    bodies = [("box", lambda: SDFBox([0, 0, 0], dt([0.9, 1.1, 1.3]), custom_mesh=False, custom_inertia=True)),
              ("sphere", lambda: SDFSphere([0, 0, 0], dt(0.55), custom_mesh=False, custom_inertia=True)),
              ("cylinder", lambda: SDFCylinder([0, 0, 0], dt(0.4), dt(1.2), custom_mesh=False, custom_inertia=True)),
              ("rounded", lambda: SDFBoxRounded([0, 0, 0], dt([0.9, 1.1, 1.3]), 0.2)),
              ("brick", lambda: SDFBrick([0, 0, 0], dt([1.0, 0.8, 0.6]), 0.15)),
              ("bowl", lambda: SDFBowl([0, 0, 0], dt(0.8), dt(0.1), custom_mesh=False))]
    done = []
    for k, (name, make) in enumerate(bodies):
        try:
            body = make()
            params = [torch.as_tensor(p).detach().clone().double().requires_grad_() for p in body.params]
            verts, _ = SDF3D._diff_marching_cubes(body.sdf_func)(*params)
            V = verts.detach().numpy()
            flat = np.concatenate([p.detach().numpy().reshape(-1) for p in params])
            if name == "rounded":       # (r', e') -> (dims' = e' + 2 r', r')
                flat = np.concatenate([flat[1:4] + 2.0 * flat[0], flat[:1]])
            prm = np.zeros(4)
            prm[: len(flat)] = flat
            kd = MC.kink_distance(name, prm, V)
            ok = np.nonzero(kd >= MC.KINK_MARGIN)[0]
            stride = len(ok) // MC.N_SUBSET
            sub = ok[::stride][: MC.N_SUBSET]
            assert stride >= 1 and len(sub) == MC.N_SUBSET and (kd[sub] >= MC.KINK_MARGIN).all(), (name, len(ok))
            gbar = MC.gbar_field(MC.N_SUBSET, 4000 + k)
            G, S = np.zeros((len(MC.PREFIXES), 4)), np.zeros((len(MC.PREFIXES), 4))
            # per-vertex terms on the subset (for the scale S): dl_v = -gbar_v . n_v, d phi / d theta_i (v)
            vs = T(V[sub]).requires_grad_()
            phi = body.sdf_func(vs, *params)
            nrm = normalize(torch.autograd.grad(phi.sum(), vs)[0], dim=1).numpy()
            dl = -(gbar * nrm).sum(1)
            jac = torch.autograd.functional.jacobian(lambda *p: body.sdf_func(T(V[sub]), *p), tuple(params))
            cols = to_kernel_order(name, [c for j in jac for c in j.reshape(MC.N_SUBSET, -1).numpy().T])
            for a, nv in enumerate(MC.PREFIXES):
                gfull = torch.zeros_like(verts)
                gfull[sub[:nv]] = T(gbar[:nv])
                for p in params:
                    p.grad = None
                (verts * gfull).sum().backward(retain_graph=True)
                g = to_kernel_order(name, list(np.concatenate([p.grad.numpy().reshape(-1) for p in params])))
                G[a, : len(g)] = g
                for i, c in enumerate(cols):
                    S[a, i] = np.abs(dl[:nv] * c[:nv]).sum()
        except Exception as e:  # noqa: BLE001 -- a type the reference cannot differentiate is reported, not stored
            print("%-9s the reference cannot do it: %s: %s" % (name, type(e).__name__, str(e).split("\n")[0]))
            continue
        out[name + "_prm"], out[name + "_verts"], out[name + "_gbar"] = prm, V[sub], gbar
        out[name + "_g"], out[name + "_S"] = G, S
        done.append(name)
        print("%-9s verts %6d admissible %6d stride %3d  g[600] %s" % (name, len(V), len(ok), stride, G[-1]))
    out["sdf_types"] = np.array(done)


def main():
    out = {}
    inertia_cases(out)
    meshsdf_cases(out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
