"""GPU: dss_mesh_grid_sdf through diffsdfsim_amd.mesh_grid, and SDFGrid3D.from_mesh on top of it, against the numpy restatement
of tests/mesh_grid_ref.py under its input conditions and bound (the sign at every sample, |kernel - reference| <= 1e-12 scale):
the face counts across the LDS tile on the 9^3 and 7 x 9 x 11 grids, the boxes and octaspheres, the two-mesh batch into a
GridTable, run-to-run bit equality, the status word; then the body: its trilinear field against the mesh's exact distance, its
scale rule, and a short drop onto the floor that has to take the very path of an SDFGrid3D given the same samples."""
import numpy as np
import pytest
import torch

import mesh_grid_ref as ref

pytestmark = pytest.mark.gpu


def check(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert np.array_equal(got < 0, want < 0), "%s: sign at %d samples" % (what, np.count_nonzero((got < 0) != (want < 0)))
    err = np.abs(got - want).max()      # (samples are phi / scale: the bound 1e-12 scale on phi is 1e-12 here)
    print("%s: max |kernel - reference| / scale = %.3e" % (what, err))
    assert err <= ref.BOUND, (what, err)


def T():
    from diffsdfsim_amd import mesh_grid
    return mesh_grid.TILE


@pytest.mark.parametrize("dims", [(9, 9, 9), (7, 9, 11)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("nf", ["T-2", "T", "T+2", "3T+6", "4"])
def test_face_counts_across_the_tile(nf, dims):
    from diffsdfsim_amd import mesh_grid
    n = eval(nf.replace("3T", "3*T"), {"T": T()})
    v, f, want, lo, off = ref.case(str(n), dims, 1.0)
    assert len(f) == n
    a, = mesh_grid.mesh_grid_sdf([v], [f], dims, 1.0)
    check(a, want, "%d faces on %s (min |phi| %.1e)" % (n, dims, lo))
    b, = mesh_grid.mesh_grid_sdf([torch.as_tensor(v).cuda()], [torch.as_tensor(f).cuda()], dims, 1.0, check=False)
    assert torch.equal(a, b)      # run to run, from device tensors as from arrays


@pytest.mark.parametrize("kind,scale,dims", [("box", 0.75, (9, 9, 9)), ("box_rot", 0.8, (9, 9, 9)), ("octa0", 1.0, (7, 7, 7)),
                                             ("octa2", 1.0, (9, 9, 9)), ("octa3", 1.0, (9, 9, 9))])
def test_boxes_and_octaspheres(kind, scale, dims):
    from diffsdfsim_amd import mesh_grid
    v, f, want, lo, off = ref.case(kind, dims, scale)
    got, = mesh_grid.mesh_grid_sdf([v], [f], dims, scale)
    check(got, want, "%s (min |phi| / scale %.1e, max |w - round w| %.1e)" % (kind, lo, off))
    if kind == "box":
        check(got, ref.box_sdf(ref.sample_points(dims, scale), (1.0, 0.7, 0.5)) / scale, "box against the analytic distance")
    inward, = mesh_grid.mesh_grid_sdf([v], [f[:, [0, 2, 1]]], dims, scale)      # (check=True turns it outward)
    assert torch.equal(inward, got)


def test_batch_of_two_meshes_into_a_grid_table():
    from diffsdfsim_amd import mesh_grid
    from diffsdfsim_amd.grids import GridTable
    a, b = ref.case("box_rot", (7, 9, 11), 0.8), ref.case(str(T() + 2), (9, 9, 9), 1.0)
    dims, data = mesh_grid.mesh_grid_sdf_pooled([a[0], b[0]], [a[1], b[1]], [(7, 9, 11), (9, 9, 9)], [0.8, 1.0])
    assert dims.tolist() == [[7, 9, 11], [9, 9, 9]] and data.shape == (693 + 729,) and data.is_cuda
    table = GridTable.from_pooled(dims, data)
    assert table.shapes == [(7, 9, 11), (9, 9, 9)] and table.off.tolist() == [0, 693] and torch.equal(table.data, data)
    check(data[:693].reshape(7, 9, 11), a[2], "batch: rotated box on 7x9x11")
    check(data[693:].reshape(9, 9, 9), b[2], "batch: %d faces on 9^3" % (T() + 2))
    _, again = mesh_grid.mesh_grid_sdf_pooled([a[0], b[0]], [a[1], b[1]], [(7, 9, 11), (9, 9, 9)], [0.8, 1.0])
    assert torch.equal(again, data)
    alone, = mesh_grid.mesh_grid_sdf([b[0]], [b[1]], (9, 9, 9), 1.0)
    assert torch.equal(alone.reshape(-1), data[693:])


def test_bad_face_index_raises_and_names_the_mesh():
    from diffsdfsim_amd import _lib, mesh_grid
    v, f = ref.octasphere(1)
    for bad in (len(v), -1):
        worse = f.copy(); worse[7, 2] = bad
        with pytest.raises(ValueError, match="mesh 1: a face index out of range"):
            mesh_grid.mesh_grid_sdf([v, v], [f, worse], (5, 5, 5), 1.0)
        with pytest.raises(_lib.HipLibraryError, match="mesh 1 has a face index outside"):
            mesh_grid.mesh_grid_sdf([v, v], [f, worse], (5, 5, 5), 1.0, check=False)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        mesh_grid.mesh_grid_sdf([v], [f], (5, 5, 5), 1.0, device="cpu")


def test_from_mesh_field_is_within_a_cell_diagonal_of_the_exact_distance():
    """The trilinear value at p is a convex combination of the eight corner samples of p's cell; the exact distance is
    1-Lipschitz and every corner is within one cell diagonal sqrt(3) h of p, so |query(p) - phi(p)| <= sqrt(3) h (and the
    samples' own error, 1e-12 scale)."""
    from diffsdfsim_amd.physics3d import SDFGrid3D
    v, f = ref.box()
    body = SDFGrid3D.from_mesh([0.0, 0.0, 0.0], v, f, res=17)
    scale = float(body.scale)
    assert scale == 1.25 * np.abs(v).max() and tuple(body.sdf.shape) == (17, 17, 17)
    p = np.random.default_rng(5).uniform(-scale, scale, (200, 3))
    got = body.query_sdfs(torch.as_tensor(p), return_grads=False).cpu().numpy()
    phi, _ = ref.signed_distance(p, v, f)
    h = 2.0 * scale / 16
    err = np.abs(got - phi).max()
    print("from_mesh box at res 17: max |query - exact| = %.3e, bound %.3e" % (err, np.sqrt(3.0) * h))
    assert err <= np.sqrt(3.0) * h * (1.0 + 1e-12)
    assert (phi < 0).sum() > 10 and (got[phi < -0.1] < 0).all()


def test_from_mesh_scale_rule_recentring_and_refusals():
    from diffsdfsim_amd import mesh_grid
    from diffsdfsim_amd.physics3d import SDFGrid3D
    v, f = ref.octasphere(2)
    own, = mesh_grid.mesh_grid_sdf([v], [f], (17, 17, 17), 1.0)
    direct = SDFGrid3D([0.0, 1.0, 0.0], 1.0, own.cpu())
    body = SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f, res=17, scale=1.0, recenter=False, mass=2.0)
    assert float(body.scale) == 1.0 and float(body.mass) == 2.0
    assert float((body.sdf - direct.sdf).abs().max()) <= 1e-12      # (1e-12 scale on phi)
    assert np.array_equal(body.verts_np, direct.verts_np) and np.array_equal(body.faces_np, direct.faces_np)
    # recentring: the same mesh moved away comes back to its centroid; the default scale is 1.25 of the recentred extent
    shift = np.array([0.3, -0.2, 0.1])
    moved = SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v + shift, f, res=17)
    c = mesh_grid.centroid(v, f)
    assert float(moved.scale) == 1.25 * np.abs(v + shift - mesh_grid.centroid(v + shift, f)).max()
    home = SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v - c, f, res=17, recenter=False, scale=float(moved.scale))
    assert float((moved.sdf - home.sdf).abs().max()) <= 1e-12
    # one full cell between the surface and the cube's faces: 0.6 <= scale (1 - 2 / 16)
    r = np.abs(v).max()
    SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f, res=17, scale=r / 0.875 * (1 + 1e-9), recenter=False)
    with pytest.raises(ValueError, match="raise scale or res"):
        SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f, res=17, scale=r / 0.875 * (1 - 1e-9), recenter=False)
    with pytest.raises(ValueError, match="raise scale or res"):
        SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f, res=9)      # the default scale holds the mesh from res 11 on
    with pytest.raises(ValueError, match="not watertight"):
        SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f[:-1], res=17)


def test_from_mesh_box_dropped_on_the_floor_steps_like_the_grid_it_is():
    from diffsdfsim_amd.physics3d import Gravity3D, SDFBox, SDFGrid3D, TotalConstraint3D, World3D
    v, f = ref.box()
    first = SDFGrid3D.from_mesh([0.0, 1.0, 0.0], v, f, res=17)
    y0 = 0.002 - float(first.verts_np[:, 1].min())      # the mesh's lowest vertex 2 mm above the floor
    runs = []
    for make in (lambda: SDFGrid3D.from_mesh([0.0, y0, 0.0], v, f, res=17, vel=(0.0, -0.5, 0.0)),
                 lambda: SDFGrid3D([0.0, y0, 0.0], float(first.scale), first.sdf.clone(), vel=(0.0, -0.5, 0.0))):
        floor = SDFBox([0, -0.5, 0], [4.0, 1.0, 4.0], custom_mesh=True, custom_inertia=True)
        body = make()
        body.add_force(Gravity3D())
        w = World3D([floor, body], [TotalConstraint3D(floor)])
        poses, touched = [], 0
        for _ in range(10):
            w.step(fixed_dt=True)
            poses.append(body.p.detach().cpu().clone())
            touched += len(w.contacts)
        assert touched >= 1
        runs.append(torch.stack(poses))
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
