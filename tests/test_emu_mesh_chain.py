"""CPU: the level-set mesh chain (csrc/marching_cubes.hip, csrc/sdf_mesh.hip) through the emulator at its launch
boundaries: marching cubes against the numpy restatement bit for bit (scan chunks, all 256 cube cases, samples equal to
the iso value), mesh inertia and its backward against the reference's autograd (tests/golden/mesh_chain.npz,
oracle/gen/gen_mesh_chain_golden.py), the MeshSDF backward per body type against the reference's, the voxel-grid query
against exact rational arithmetic.  The assertions and their tolerances are in mesh_chain_checks.py; the emulator does
not model atomics contention or the device's division / square-root sequences: test_mesh_chain_gpu.py repeats all of it
on the device."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_chain_checks as CK
from diffsdfsim_amd import mc_tables
from emu import emu

DSS_E_BADARG, DSS_E_WORKSPACE = -1, -2


class Emu:
    mc = staticmethod(emu.marching_cubes)
    inertia = staticmethod(emu.mesh_inertia)
    inertia_batch = staticmethod(emu.mesh_inertia_batch)
    inertia_bwd = staticmethod(emu.mesh_inertia_backward)
    meshsdf_bwd = staticmethod(emu.meshsdf_backward)
    grid_query = staticmethod(emu.grid_sdf_query)


BE = Emu()


# ---- marching cubes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.NOISE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_marching_cubes_dense_noise_across_scan_chunks(shape):
    v, f = CK.check_mc_equals_restatement(BE, ("noise", shape))
    assert len(v) > 1000 and len(f) > 1000


@pytest.mark.parametrize("block", range(8))
def test_marching_cubes_every_cube_case(block):
    """One 2 x 2 x 2 grid per sign pattern (an emulated launch costs the same whatever the grid: 32 patterns per test)."""
    CK.check_mc_cube_cases(BE, range(32 * block, 32 * block + 32))


def test_marching_cubes_samples_equal_to_iso():
    CK.check_mc_lattice(BE)


def test_marching_cubes_nonzero_iso():
    CK.check_mc_equals_restatement(BE, ("noise_iso",))


def test_marching_cubes_empty_mesh_and_totals():
    CK.check_mc_empty(BE)
    tot = _count(np.full((4, 5, 6), 0.25))[1]
    assert tuple(tot) == (0, 0)


@pytest.mark.parametrize("key", [("noise", (7, 9, 11)), ("lattice",)], ids=["noise", "lattice"])
def test_vectorised_restatement_equals_the_slow_one(key):
    phi, iso = CK.field(key)
    v, f = mc_tables.marching_cubes_numpy_vec(phi, iso)
    v0, f0 = mc_tables.marching_cubes_numpy(phi, iso)
    assert len(v) > 100 and np.array_equal(v, v0) and np.array_equal(f, f0)


def _count(phi, short=0, n0=None):
    L = emu.lib()
    ntri = np.ascontiguousarray(mc_tables.tables()[0], np.int32)
    n = list(phi.shape)
    if n0 is not None:
        n[0] = n0
    nb = L.dss_mc_workspace_bytes(*phi.shape)
    ws = np.zeros(nb, np.uint8); tot = np.full(2, -7, np.int32)
    rc = L.dss_mc_count(phi.ctypes.data, n[0], n[1], n[2], 0.0, ntri.ctypes.data, ws.ctypes.data, nb - short, tot.ctypes.data, None)
    return rc, tot


def test_marching_cubes_return_codes():
    phi = np.ascontiguousarray(MC.noise((5, 6, 7)))
    assert _count(phi)[0] == 0
    assert _count(phi, short=1)[0] == DSS_E_WORKSPACE
    assert _count(phi, n0=1)[0] == DSS_E_BADARG
    assert emu.lib().dss_mc_workspace_bytes(1, 6, 7) == 0


# ---- inertia ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.NAMES)
def test_mesh_inertia_and_volume(name):
    CK.check_inertia_forward(BE, name)


def test_mesh_inertia_pooled_table_is_bitwise_the_single_calls():
    CK.check_inertia_pooled_bitwise(BE)


@pytest.mark.parametrize("name", MC.NAMES)
def test_mesh_inertia_backward_matches_reference_autograd(name):
    CK.check_inertia_backward(BE, name, report=print)


def test_mesh_inertia_backward_clears_its_output():
    """The output buffer arrives full of NaN: the row of a vertex that no face uses is exactly 0, the rest is finite."""
    v, f, mass, gJ = CK.case("ico2_orphan")
    g = emu.mesh_inertia_backward(v, f, mass, gJ, fill=np.nan)
    assert np.isfinite(g).all() and (g[-1] == 0.0).all() and np.abs(g[:-1]).min(0).max() > 0
    assert CK.inertia_bwd_error("ico2_orphan", g) <= CK.inertia_bound("ico2_orphan")


def test_mesh_inertia_backward_bad_sizes():
    L = emu.lib()
    v, f, mass, gJ = CK.case("tetra")
    F = np.ascontiguousarray(f, np.int32); g = np.ascontiguousarray(gJ).reshape(9); out = np.zeros_like(v)
    call = lambda nv, nf: L.dss_mesh_inertia_backward(v.ctypes.data, F.ctypes.data, nv, nf, mass, g.ctypes.data, out.ctypes.data, None)
    assert call(4, 4) == 0 and call(4, 0) == DSS_E_BADARG and call(0, 4) == DSS_E_BADARG


# ---- MeshSDF backward, voxel-grid query --------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", CK.sdf_types())
def test_meshsdf_backward_matches_reference(ty):
    CK.check_meshsdf_backward(BE, ty, report=print)


def test_meshsdf_backward_types_of_the_golden():
    assert CK.sdf_types() == ["box", "sphere", "cylinder", "rounded", "brick"]      # the reference's bowl has no backward


def test_grid_query_exact_on_a_noncubic_grid():
    CK.check_grid_query(BE)


def test_grid_query_all_boundary_layers():
    CK.check_grid_query_all_boundary(BE)
