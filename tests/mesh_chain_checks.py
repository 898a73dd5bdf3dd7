"""The assertions of the mesh-chain tests, stated once on numpy arrays: test_emu_mesh_chain.py runs them on the CPU
emulation of the kernels, test_mesh_chain_gpu.py on the device through the product bindings.  A backend is an object with

    mc(phi, iso) -> verts [V,3], faces [F,3]               inertia(v, f, mass) -> J [3,3], vol
    inertia_batch(vs, fs, masses) -> J [n,3,3], vol [n]    inertia_bwd(v, f, mass, gJ) -> g [V,3]
    meshsdf_bwd(type, prm, verts, gbar) -> g [len(prm)]    grid_query(G, scale, pts) -> sdf, grad, mask

Tolerances.  Inertia backward: max|g - g_ref| / max|g_ref| over the stored rows <= 16 * max(d_ref, 2^-50), d_ref being
the reference's autograd against itself under a permutation of the face rows (the kernel differentiates with dual numbers
in another operation order and adds the contributions of the faces around a vertex atomically, in any order).  MeshSDF
backward: |g_i - g_ref,i| / S_i <= 3 * 1e-13 + nv * 2^-52 with S_i = sum_v |dl_v d phi / d theta_i (v)| (the per-component
tolerance the suite holds for SDF gradients, over three components, plus the reordering of nv terms).  J: 1e-11 max|J|,
volume 1e-13 relative (the same reduction), grid gradient 1e-12: the tolerances the suite already holds for them.
"""
import functools
import os

import numpy as np

import mesh_cases as MC
from diffsdfsim_amd import mc_tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_chain.npz")


@functools.lru_cache(None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(None)
def case(name):
    return MC.case(name)


@functools.lru_cache(None)
def mc_reference(key):
    """The numpy restatement's mesh of a named field, computed once."""
    phi, iso = field(key)
    return mc_tables.marching_cubes_numpy_vec(phi, iso)


@functools.lru_cache(None)
def field(key):
    kind = key[0]
    if kind == "noise":
        return MC.noise(key[1], seed=sum(key[1])), 0.0
    if kind == "noise_iso":
        return MC.noise((11, 12, 13), seed=3), 0.37
    if kind == "lattice":
        return MC.lattice_field(), 0.0
    if kind == "cube":
        return MC.cube_case_field(key[1]), 0.0
    if kind == "sparse":
        return MC.sparse_sign_field(key[1]), 0.0
    raise KeyError(key)


# ---- marching cubes ---------------------------------------------------------------------------------------------------
def check_mc_equals_restatement(be, key):
    phi, iso = field(key)
    v, f = be.mc(phi, iso)
    v0, f0 = mc_reference(key)
    assert v.shape == v0.shape and f.shape == f0.shape, (v.shape, v0.shape, f.shape, f0.shape)   # the scan totals
    assert np.array_equal(f, f0) and np.array_equal(v, v0)
    return v, f


def check_mc_cube_cases(be, cases=range(256)):
    for c in cases:
        v, f = check_mc_equals_restatement(be, ("cube", c))
        assert MC.triangles_point_outwards(field(("cube", c))[0], v, f), c
        assert (len(f) == 0) == (c in (0, 255))


def check_mc_lattice(be):
    """phi == iso exactly at grid points: `<` is strict, a zero sample is outside; t is exactly 0 or 1 on its edges."""
    phi, _ = field(("lattice",))
    v, f = check_mc_equals_restatement(be, ("lattice",))
    assert np.isfinite(v).all() and (phi == 0.0).sum() > 50
    ins = phi < 0.0
    cut = [ins[1:] != ins[:-1], ins[:, 1:] != ins[:, :-1], ins[:, :, 1:] != ins[:, :, :-1]]
    zero_end = [(phi[1:] == 0) | (phi[:-1] == 0), (phi[:, 1:] == 0) | (phi[:, :-1] == 0), (phi[:, :, 1:] == 0) | (phi[:, :, :-1] == 0)]
    assert len(v) == sum(int(c.sum()) for c in cut)                     # `<=` would cut other edges
    at_node = (v == np.round(v)).all(1)                                  # t in {0, 1}: the vertex sits on the zero sample
    assert at_node.sum() == sum(int((c & z).sum()) for c, z in zip(cut, zero_end)) > 0
    assert (phi[tuple(np.round(v[at_node]).astype(int).T)] == 0.0).all()


def check_mc_empty(be):
    v, f = be.mc(np.full((4, 5, 6), 0.25), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ---- inertia ----------------------------------------------------------------------------------------------------------
def inertia_bound(name):
    return 16.0 * max(float(golden()[name + "_dref"]), 2.0 ** -50)


def inertia_bwd_error(name, g):
    G = golden()
    ref = G[name + "_g"]
    return np.abs(g[G[name + "_rows"]] - ref).max() / np.abs(ref).max()


def check_inertia_forward(be, name):
    G = golden()
    v, f, mass, _ = case(name)
    J, vol = be.inertia(v, f, mass)
    assert np.abs(J - G[name + "_J"]).max() < 1e-11 * np.abs(G[name + "_J"]).max()
    assert abs(vol - G[name + "_vol"]) < 1e-13 * abs(G[name + "_vol"]), (vol, G[name + "_vol"])
    return J, vol


def check_inertia_pooled_bitwise(be):
    """All meshes in one table, distinct masses, non-zero offsets: each mesh goes through the same reduction tree as alone."""
    cs = [case(n) for n in MC.NAMES]
    J, vol = be.inertia_batch([c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs])
    for k, n in enumerate(MC.NAMES):
        J1, v1 = be.inertia(cs[k][0], cs[k][1], cs[k][2])
        assert np.array_equal(J[k], J1) and vol[k] == v1, n


def check_inertia_backward(be, name, report=None):
    v, f, mass, gJ = case(name)
    g = be.inertia_bwd(v, f, mass, gJ)
    err, bound = inertia_bwd_error(name, g), inertia_bound(name)
    if report is not None:
        report("%-12s nf %5d  d_ref %.2e  bound %.2e  measured %.2e" % (name, len(f), float(golden()[name + "_dref"]), bound, err))
    assert np.isfinite(g).all() and err <= bound, (name, err, bound)
    return g


# ---- MeshSDF backward --------------------------------------------------------------------------------------------------
def sdf_types():
    return [str(t) for t in golden()["sdf_types"]]


def check_meshsdf_backward(be, ty, report=None):
    G = golden()
    prm = G[ty + "_prm"]
    k = {"box": 3, "sphere": 1, "cylinder": 2, "rounded": 4, "brick": 4}[ty]
    for a, nv in enumerate(MC.PREFIXES):
        g = be.meshsdf_bwd(MC.SDF_TYPES[ty], prm[:max(k, 3)] if k < 4 else prm, G[ty + "_verts"][:nv], G[ty + "_gbar"][:nv])
        S, ref = G[ty + "_S"][a, :k], G[ty + "_g"][a, :k]
        # a parameter that none of the nv vertices depends on (one vertex on one face of the box): every term is zero
        assert (g[:k][S == 0] == 0.0).all() and (ref[S == 0] == 0.0).all() and (S > 0).any()
        err = np.abs(g[:k] - ref) / np.where(S > 0, S, 1.0)
        bound = 3 * 1e-13 + nv * 2.0 ** -52
        if report is not None:
            report("%-9s nv %3d  bound %.2e  measured %.2e" % (ty, nv, bound, err.max()))
        assert (err <= bound).all(), (ty, nv, err, bound)


# ---- voxel-grid query --------------------------------------------------------------------------------------------------
def check_grid_query(be):
    G, scale, pts = MC.grid_query_case()
    sdf, grad, mask = be.grid_query(G, scale, pts)
    exact = MC.grid_value_exact(G, pts)
    inside = np.array([e is not None for e in exact])
    assert np.array_equal(mask, inside) and inside.sum() == len(pts) - 4
    for t, e in enumerate(exact):
        if e is None:
            assert sdf[t] == scale and (grad[t] == 0.0).all()
        else:
            assert float(e) == e                      # representable: the kernel's sum has nothing to round
            assert sdf[t] == float(e), (t, sdf[t], float(e))
    ref = MC.grid_grad_longdouble(G, pts)
    assert np.abs(grad - ref).max() < 1e-12
    assert np.abs(ref).max() > 0.5


def check_grid_query_all_boundary(be):
    G = np.arange(8.0).reshape(2, 2, 2) - 3.0
    pts = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 1.0], [-1.0, -1.0, -1.0]])
    sdf, grad, mask = be.grid_query(G, 1.0, pts)
    assert mask.all() and np.isfinite(sdf).all() and (grad == 0.0).all()
    assert sdf[0] == 0.5 and sdf[2] == -3.0
