"""GPU: the level-set mesh chain on the device through the product bindings (meshsdf.marching_cubes,
mass_properties.mesh_inertia / mesh_inertia_diff / grid_sdf_query, dss_meshsdf_backward, dss_mesh_inertia_backward):
everything test_emu_mesh_chain.py checks in the emulator (mesh_chain_checks.py holds the assertions and the tolerances),
plus what only the device can afford or show: scan carries across 256 / 257 / 514 chunks, atomics onto shared vertices
from up to 32 workgroups, run-to-run bit equality of the kernels without atomics.

Measured on an MI355X (inertia backward: max|g - g_ref| / max|g_ref| over the stored rows; bound = 16 max(d_ref, 2^-50)):
    tetra        nf     4  d_ref 1.87e-15  bound 2.99e-14  measured 2.29e-15
    ico2         nf   320  d_ref 8.87e-15  bound 1.42e-13  measured 1.04e-14
    ico2_orphan  nf   320  d_ref 3.66e-15  bound 5.86e-14  measured 8.61e-15
    bipyr254     nf   254  d_ref 9.80e-16  bound 1.57e-14  measured 1.54e-15
    bipyr256     nf   256  d_ref 3.01e-15  bound 4.81e-14  measured 3.39e-15
    bipyr258     nf   258  d_ref 3.07e-15  bound 4.92e-14  measured 3.57e-15
    ico4         nf  5120  d_ref 2.59e-13  bound 4.14e-12  measured 1.28e-13
    bipyr8190    nf  8190  d_ref 4.54e-13  bound 7.27e-12  measured 4.20e-13
    bipyr8192    nf  8192  d_ref 8.85e-14  bound 1.42e-12  measured 9.76e-14
    bipyr8194    nf  8194  d_ref 1.53e-13  bound 2.45e-12  measured 1.47e-13
    bipyr8194 twice more in one test: 1.46e-13, 1.48e-13 (the order of the atomic adds is not fixed)
MeshSDF backward, max over parameters of |g_i - g_ref,i| / S_i (bound = 3e-13 + nv 2^-52):
    box       nv   1  bound 3.00e-13  measured 0.00e+00
    box       nv 255  bound 3.57e-13  measured 0.00e+00
    box       nv 256  bound 3.57e-13  measured 0.00e+00
    box       nv 257  bound 3.57e-13  measured 0.00e+00
    box       nv 600  bound 4.33e-13  measured 0.00e+00
    sphere    nv   1  bound 3.00e-13  measured 0.00e+00
    sphere    nv 255  bound 3.57e-13  measured 1.63e-17
    sphere    nv 256  bound 3.57e-13  measured 1.62e-17
    sphere    nv 257  bound 3.57e-13  measured 3.21e-17
    sphere    nv 600  bound 4.33e-13  measured 3.63e-18
    cylinder  nv   1  bound 3.00e-13  measured 0.00e+00
    cylinder  nv 255  bound 3.57e-13  measured 2.55e-18
    cylinder  nv 256  bound 3.57e-13  measured 2.55e-18
    cylinder  nv 257  bound 3.57e-13  measured 2.55e-18
    cylinder  nv 600  bound 4.33e-13  measured 1.17e-17
    rounded   nv   1  bound 3.00e-13  measured 5.88e-16
    rounded   nv 255  bound 3.57e-13  measured 7.84e-17
    rounded   nv 256  bound 3.57e-13  measured 7.84e-17
    rounded   nv 257  bound 3.57e-13  measured 6.71e-17
    rounded   nv 600  bound 4.33e-13  measured 1.70e-16
    brick     nv   1  bound 3.00e-13  measured 9.99e-16
    brick     nv 255  bound 3.57e-13  measured 2.10e-16
    brick     nv 256  bound 3.57e-13  measured 2.10e-16
    brick     nv 257  bound 3.57e-13  measured 2.86e-16
    brick     nv 600  bound 4.33e-13  measured 5.72e-17
"""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_chain_checks as CK

pytestmark = pytest.mark.gpu
DSS_E_BADARG, DSS_E_WORKSPACE = -1, -2


def _np(t):
    return t.detach().cpu().numpy()


def _inertia_bwd_raw(v, f, mass, gJ, nv=None, nf=None):
    """dss_mesh_inertia_backward into a buffer full of NaN -> return code, gradient."""
    from diffsdfsim_amd import _lib
    V = torch.tensor(v, dtype=torch.float64, device="cuda"); F = torch.tensor(f, dtype=torch.int32, device="cuda")
    g = torch.tensor(np.asarray(gJ).reshape(9), dtype=torch.float64, device="cuda")
    out = torch.full_like(V, float("nan"))
    rc = _lib.lib().dss_mesh_inertia_backward(_lib.ptr(V), _lib.ptr(F), len(v) if nv is None else nv, len(f) if nf is None else nf,
                                              float(mass), _lib.ptr(g), _lib.ptr(out), _lib.stream_ptr(V.device))
    return rc, _np(out)


class Device:
    @staticmethod
    def mc(phi, iso=0.0):
        from diffsdfsim_amd.meshsdf import marching_cubes
        v, f = marching_cubes(torch.tensor(phi), iso)
        return _np(v), _np(f)

    @staticmethod
    def inertia(v, f, mass):
        from diffsdfsim_amd.mass_properties import mesh_inertia
        J, vol = mesh_inertia(v, f, mass, return_volume=True)
        return _np(J), float(vol)

    @staticmethod
    def inertia_batch(vs, fs, masses):
        from diffsdfsim_amd.mass_properties import mesh_inertia
        J, vol = mesh_inertia(list(vs), list(fs), list(masses), return_volume=True)
        return _np(J), _np(vol)

    @staticmethod
    def inertia_bwd(v, f, mass, gJ):
        rc, g = _inertia_bwd_raw(v, f, mass, gJ)
        assert rc == 0
        return g

    @staticmethod
    def meshsdf_bwd(ty, prm, verts, gbar):
        from diffsdfsim_amd import _lib
        V = torch.tensor(verts, dtype=torch.float64, device="cuda"); Gb = torch.tensor(gbar, dtype=torch.float64, device="cuda")
        out = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
        p = np.zeros(4); p[: len(prm)] = prm
        _lib.check(_lib.lib().dss_meshsdf_backward(int(ty), p.ctypes.data, _lib.ptr(V), _lib.ptr(Gb), len(verts), _lib.ptr(out),
                                                   _lib.stream_ptr(V.device)), "dss_meshsdf_backward")
        return _np(out)

    @staticmethod
    def grid_query(G, scale, pts):
        from diffsdfsim_amd.mass_properties import grid_sdf_query
        sdf, grad, mask = grid_sdf_query(G, scale, pts, True, True)
        return _np(sdf), _np(grad), _np(mask)


BE = Device()


# ---- marching cubes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.NOISE_SHAPES + ((64, 64, 257),), ids=lambda s: "x".join(map(str, s)))
def test_marching_cubes_dense_noise_across_scan_chunks(shape):
    v, f = CK.check_mc_equals_restatement(BE, ("noise", shape))
    assert len(v) > 1000 and len(f) > 1000


@pytest.mark.parametrize("n2", [262144, 262145, 525313])
def test_marching_cubes_scan_of_the_chunk_sums(n2):
    """2 x 2 x n2: 256 chunks (one trip of the 256-wide loop over the chunk sums, full), 257 and 514 (second and third
    trip: the running total carried between trips), a few thousand cuts spread over all chunks."""
    v, f = CK.check_mc_equals_restatement(BE, ("sparse", n2))
    assert 3000 < len(v) < 6000 and len(f) > 2000


def test_marching_cubes_every_cube_case():
    CK.check_mc_cube_cases(BE)


def test_marching_cubes_samples_equal_to_iso():
    CK.check_mc_lattice(BE)


def test_marching_cubes_nonzero_iso():
    CK.check_mc_equals_restatement(BE, ("noise_iso",))


def test_marching_cubes_empty_mesh():
    CK.check_mc_empty(BE)


def test_marching_cubes_return_codes():
    from diffsdfsim_amd import _lib, mc_tables
    L = _lib.lib()
    phi = torch.tensor(MC.noise((5, 6, 7)), device="cuda")
    ntri = torch.tensor(mc_tables.tables()[0], dtype=torch.int32, device="cuda")
    nb = L.dss_mc_workspace_bytes(5, 6, 7)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda"); tot = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda n0, nbytes: L.dss_mc_count(_lib.ptr(phi), n0, 6, 7, 0.0, _lib.ptr(ntri), _lib.ptr(ws), nbytes, _lib.ptr(tot),
                                             _lib.stream_ptr(phi.device))
    assert call(5, nb) == 0 and call(5, nb - 1) == DSS_E_WORKSPACE and call(1, nb) == DSS_E_BADARG
    torch.cuda.synchronize()


def test_marching_cubes_and_inertia_are_bitwise_repeatable():
    """No atomics in either: two calls give the same bits."""
    phi, _ = CK.field(("noise", (17, 17, 17)))
    (v1, f1), (v2, f2) = BE.mc(phi), BE.mc(phi)
    assert np.array_equal(v1, v2) and np.array_equal(f1, f2)
    v, f, mass, _ = CK.case("bipyr8194")
    (J1, vol1), (J2, vol2) = BE.inertia(v, f, mass), BE.inertia(v, f, mass)
    assert np.array_equal(J1, J2) and vol1 == vol2


# ---- inertia ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.NAMES)
def test_mesh_inertia_and_volume(name):
    CK.check_inertia_forward(BE, name)


def test_mesh_inertia_pooled_table_is_bitwise_the_single_calls():
    CK.check_inertia_pooled_bitwise(BE)


@pytest.mark.parametrize("name", MC.NAMES)
def test_mesh_inertia_backward_matches_reference_autograd(name):
    CK.check_inertia_backward(BE, name, report=print)


def test_mesh_inertia_backward_twice_on_the_second_trip_of_the_stride_loop():
    """8194 faces: 32 workgroups, two faces on the second trip; 4097 atomic adds per apex in an order that is not
    fixed.  Both results are held to the golden; nothing is asserted about their equality."""
    for k in range(2):
        CK.check_inertia_backward(BE, "bipyr8194", report=print)


def test_mesh_inertia_backward_clears_its_output():
    """The output buffer arrives full of NaN: the row of a vertex that no face uses is exactly 0, the rest is finite."""
    v, f, mass, gJ = CK.case("ico2_orphan")
    rc, g = _inertia_bwd_raw(v, f, mass, gJ)
    assert rc == 0 and np.isfinite(g).all() and (g[-1] == 0.0).all() and np.abs(g[:-1]).min(0).max() > 0
    assert CK.inertia_bwd_error("ico2_orphan", g) <= CK.inertia_bound("ico2_orphan")


def test_mesh_inertia_backward_bad_sizes():
    v, f, mass, gJ = CK.case("tetra")
    assert _inertia_bwd_raw(v, f, mass, gJ, nf=0)[0] == DSS_E_BADARG
    assert _inertia_bwd_raw(v, f, mass, gJ, nv=0)[0] == DSS_E_BADARG


def test_mesh_inertia_diff_gradients_and_devices():
    """The autograd wrapper: vertex gradient against the golden and back on the device of `verts` (the CPU here), mass
    gradient = sum gJ * J / mass (J is linear in the mass) from the golden J."""
    from diffsdfsim_amd.mass_properties import mesh_inertia_diff
    G = CK.golden()
    for name in ("ico2", "bipyr258"):
        v, f, mass, gJ = CK.case(name)
        vt = torch.tensor(v, requires_grad=True)
        mt = torch.tensor(mass, dtype=torch.float64, requires_grad=True)
        J = mesh_inertia_diff(vt, torch.tensor(f), mt)
        assert not J.is_cuda
        (J * torch.tensor(gJ)).sum().backward()
        assert not vt.grad.is_cuda and vt.grad.shape == vt.shape
        assert CK.inertia_bwd_error(name, vt.grad.numpy()) <= CK.inertia_bound(name)
        gm = (gJ * G[name + "_J"]).sum() / mass
        assert abs(float(mt.grad) - gm) < 1e-11 * np.abs(gJ * G[name + "_J"]).sum() / mass


# ---- MeshSDF backward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", CK.sdf_types())
def test_meshsdf_backward_matches_reference(ty):
    CK.check_meshsdf_backward(BE, ty, report=print)


@pytest.mark.parametrize("ty,prm", [("sphere", [0.6]), ("rounded", [0.9 / 0.975, 1.1 / 0.975, 1.3 / 0.975, 0.2 / 0.975])])
def test_primitive_mesh_autograd_is_the_direct_call(ty, prm):
    """The binding's slicing and reshaping, not the kernel's arithmetic: d(sum gbar(v) . v)/d prm through
    primitive_mesh(res=128) with gbar = a + B v taken from the device vertices, against dss_meshsdf_backward called
    directly on those vertices with that gbar.  Same kernel, same inputs, one workgroup with a fixed tree: 1e-15 of the
    largest entry."""
    from diffsdfsim_amd.meshsdf import primitive_mesh
    r = np.random.default_rng(31)
    a = torch.tensor(r.standard_normal(3), device="cuda"); B = torch.tensor(r.standard_normal((3, 3)), device="cuda")
    p = torch.tensor(prm, dtype=torch.float64, requires_grad=True)
    v, f = primitive_mesh(MC.SDF_TYPES[ty], p, res=128)
    gbar = a + v.detach() @ B.T
    (gbar * v).sum().backward()
    assert p.grad.shape == p.shape and not p.grad.is_cuda
    direct = BE.meshsdf_bwd(MC.SDF_TYPES[ty], prm, _np(v), _np(gbar))[: len(prm)]
    assert np.isfinite(direct).all() and np.abs(direct).min() > 0
    assert np.abs(p.grad.numpy() - direct).max() <= 1e-15 * np.abs(direct).max()


# ---- voxel-grid query --------------------------------------------------------------------------------------------------
def test_grid_query_exact_on_a_noncubic_grid():
    CK.check_grid_query(BE)


def test_grid_query_all_boundary_layers():
    CK.check_grid_query_all_boundary(BE)
