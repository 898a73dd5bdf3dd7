"""CPU: csrc/mesh_grid.hip through the emulator (the kernel, its launch shape and LDS tiles as on the device) against the numpy
restatement of tests/mesh_grid_ref.py, whose docstring states the input conditions and the value bound: at every sample the
kernel's sign, and |kernel - reference| <= 1e-12 scale.  With T = DSS_MESH_GRID_TILE the face counts T - 2, T, T + 2, 3 T + 6 and 4
cross the tile's seams, the grids 2^3, 8^3 (two full workgroups), 9^3 (a ragged third) and 7 x 9 x 11 (unequal axes) the
workgroup's.  Also here: the host-side checks of diffsdfsim_amd.mesh_grid.check_mesh and meshes.load_obj.
tests/emu/check_mesh_grid.cpp walks the same seams as a program of its own under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_grid_ref as ref
from diffsdfsim_amd import mesh_grid, meshes
from emu import emu

HERE = os.path.dirname(os.path.abspath(__file__))
T = mesh_grid.TILE
GUARD = -7.0


def voxelise(mesh_list, dims, scales, front=2):
    """dss_mesh_grid_sdf on host arrays with guards: `front` NaN vertex rows and unreadable face rows before the first mesh (so
    vert_off and face_off start above 0) and two after the last, a guard word after every grid (so grid_off is not the running
    sum) and after the pool, one after the status words.  -> (grids, status)"""
    L = emu.lib()
    nm = len(mesh_list)
    nanrows, badrows = np.full((front, 3), np.nan), np.full((front, 3), 2 ** 30, np.int32)
    V = np.ascontiguousarray(np.concatenate([nanrows] + [v for v, _ in mesh_list] + [nanrows]), dtype=np.float64)
    F = np.ascontiguousarray(np.concatenate([badrows] + [f for _, f in mesh_list] + [badrows]), dtype=np.int32)
    voff = (front + np.cumsum([0] + [len(v) for v, _ in mesh_list])).astype(np.int32)
    foff = (front + np.cumsum([0] + [len(f) for _, f in mesh_list])).astype(np.int32)
    dims = np.ascontiguousarray(np.broadcast_to(np.asarray(dims, np.int32), (nm, 3)))
    sizes = dims.astype(np.int64).prod(1)
    goff = (np.cumsum(np.concatenate([[0], sizes[:-1]])) + np.arange(nm)).astype(np.int32)
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, np.float64), (nm,)))
    pool, status = np.full(int(sizes.sum()) + nm + 1, GUARD), np.full(nm + 1, -7, np.int32)
    rc = L.dss_mesh_grid_sdf(nm, V.ctypes.data, F.ctypes.data, voff.ctypes.data, foff.ctypes.data, dims.ctypes.data, goff.ctypes.data,
                             sc.ctypes.data, int(sizes.max()), max(len(f) for _, f in mesh_list), pool.ctypes.data, status.ctypes.data, None)
    assert rc == 0 and status[-1] == -7 and pool[-1] == GUARD
    grids = []
    for m in range(nm):
        assert pool[goff[m] + sizes[m]] == GUARD      # the word after the grid
        grids.append(pool[goff[m]:goff[m] + sizes[m]].reshape(dims[m]).copy())
    return grids, status[:nm].copy()


reference = ref.case


def check(got, want, what):
    assert np.isfinite(got).all(), what
    assert np.array_equal(got < 0, want < 0), "%s: sign at %d samples" % (what, np.count_nonzero((got < 0) != (want < 0)))
    err = np.abs(got - want).max()      # (samples are phi / scale: the bound 1e-12 scale on phi is 1e-12 here)
    print("%s: max |kernel - reference| / scale = %.3e" % (what, err))
    assert err <= ref.BOUND, (what, err)


def test_python_constants_are_the_headers():
    text = open(os.path.join(HERE, "..", "diffsdfsim_amd", "csrc", "mesh_grid.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define DSS_MESH_GRID_(\w+) (\d+)", text)}
    assert got == dict(TILE=mesh_grid.TILE, MALFORMED=mesh_grid.MALFORMED)


@pytest.mark.parametrize("dims", [(2, 2, 2), (8, 8, 8), (9, 9, 9), (7, 9, 11)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("nf", [T - 2, T, T + 2, 3 * T + 6, 4])
def test_face_counts_across_the_tile_on_grids_across_the_workgroup(nf, dims):
    v, f, want, lo, off = reference(str(nf), dims, 1.0)
    assert len(f) == nf
    (got,), status = voxelise([(v, f)], dims, 1.0)
    assert status[0] == 0
    check(got, want, "%d faces on %s (min |phi| %.1e)" % (nf, dims, lo))


@pytest.mark.parametrize("kind,scale,dims", [("box", 0.75, (9, 9, 9)), ("box_rot", 0.8, (9, 9, 9)), ("octa0", 1.0, (7, 7, 7)),
                                             ("octa2", 1.0, (9, 9, 9)), ("octa3", 1.0, (9, 9, 9))])
def test_boxes_and_octaspheres(kind, scale, dims):
    v, f, want, lo, off = reference(kind, dims, scale)
    (got,), status = voxelise([(v, f)], dims, scale)
    assert status[0] == 0
    check(got, want, "%s (min |phi| / scale %.1e, max |w - round w| %.1e)" % (kind, lo, off))
    if kind == "box":
        exact = ref.box_sdf(ref.sample_points(dims, scale), (1.0, 0.7, 0.5)) / scale
        assert np.abs(want - exact).max() <= 1e-15
        check(got, exact, "box against the analytic distance")
    assert (got < 0).any() and (got > 0).any()


def test_batch_of_two_meshes_with_offsets_and_guards_twice():
    a, b = reference("box_rot", (7, 9, 11), 0.8), reference(str(T + 2), (9, 9, 9), 1.0)
    grids, status = voxelise([a[:2], b[:2]], [(7, 9, 11), (9, 9, 9)], [0.8, 1.0], front=3)
    assert not status.any()
    check(grids[0], a[2], "batch: rotated box on 7x9x11")
    check(grids[1], b[2], "batch: %d faces on 9^3" % (T + 2))
    again, _ = voxelise([a[:2], b[:2]], [(7, 9, 11), (9, 9, 9)], [0.8, 1.0], front=3)
    assert all(np.array_equal(x, y) for x, y in zip(grids, again))
    # the other order: the longer face list and the larger grid first
    swapped, _ = voxelise([b[:2], a[:2]], [(9, 9, 9), (7, 9, 11)], [1.0, 0.8])
    assert np.array_equal(swapped[0], grids[1]) and np.array_equal(swapped[1], grids[0])


def test_inward_copy_through_the_check_is_the_outward_grid():
    v, f, want, _, _ = reference("octa2", (9, 9, 9), 1.0)
    vi, fi = mesh_grid.check_mesh(v, f[:, [0, 2, 1]].astype(np.int32))
    assert fi.dtype == np.int64 and np.array_equal(fi, f)
    (out,), _ = voxelise([(v, f)], (9, 9, 9), 1.0)
    (inw,), _ = voxelise([(vi, fi)], (9, 9, 9), 1.0)
    assert np.array_equal(out, inw)
    (raw,), _ = voxelise([(v, f[:, [0, 2, 1]])], (9, 9, 9), 1.0)      # unchecked, the inward mesh has winding number -1 inside: positive everywhere
    assert (raw > 0).all() and np.abs(raw - np.abs(want)).max() <= ref.BOUND


@pytest.mark.parametrize("bad", ["nv", "-1"])
def test_face_index_out_of_range_sets_the_status_and_is_left_out(bad):
    v, f = ref.mesh_of(T + 2)
    worse = np.concatenate([f[:T - 1], [[0, 1, len(v) if bad == "nv" else -1]], f[T - 1:]])      # in the first tile; index nv names a NaN guard row
    (got,), status = voxelise([(v, worse)], (9, 9, 9), 1.0)
    assert status[0] == mesh_grid.MALFORMED and np.isfinite(got).all()
    dist = ref.distance(ref.sample_points((9, 9, 9), 1.0).reshape(-1, 3), v, f).reshape(9, 9, 9)      # (the bad face was an extra one)
    assert np.abs(np.abs(got) - dist).max() <= ref.BOUND
    # a second mesh in the same call keeps its own status word
    grids, status = voxelise([(v, worse), ref.box()], (7, 7, 7), 1.0)
    assert status.tolist() == [mesh_grid.MALFORMED, 0]


def test_coincident_zero_area_pair_changes_nothing():
    v, f, want, _, _ = reference("octa0", (7, 7, 7), 1.0)
    a, b = f[0, 0], f[0, 1]
    v2 = np.concatenate([v, [0.5 * (v[a] + v[b])]])
    f2 = np.concatenate([f, [[a, b, len(v)], [b, a, len(v)]]])
    (got,), status = voxelise([(v2, f2)], (7, 7, 7), 1.0)
    assert status[0] == 0
    check(got, want, "octahedron with a coincident zero-area pair")
    # three equal corners: a triangle that is one point, on the surface
    f3 = np.concatenate([f, [[a, a, a]]])
    (got,), _ = voxelise([(v, f3)], (7, 7, 7), 1.0)
    check(got, want, "octahedron with a one-point triangle")


def test_return_codes_leave_the_outputs_untouched():
    L = emu.lib()
    v, f = ref.box()
    V, F = np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int32)
    voff, foff = np.array([0, 8], np.int32), np.array([0, 12], np.int32)
    dims, goff, sc = np.array([3, 3, 3], np.int32), np.zeros(1, np.int32), np.ones(1)
    out, status = np.full(27, GUARD), np.full(1, -7, np.int32)
    A = dict(nmesh=1, verts=V.ctypes.data, faces=F.ctypes.data, vert_off=voff.ctypes.data, face_off=foff.ctypes.data, dims=dims.ctypes.data,
             grid_off=goff.ctypes.data, scale=sc.ctypes.data, max_samples=27, max_faces=12, out=out.ctypes.data, status=status.ctypes.data)
    call = lambda **kw: L.dss_mesh_grid_sdf(*{**A, **kw}.values(), None)
    for bad in [dict(nmesh=0), dict(nmesh=-1), dict(max_samples=0), dict(max_faces=0)] + \
            [{k: None} for k in A if k not in ("nmesh", "max_samples", "max_faces")]:
        assert call(**bad) == -1, bad                               # DSS_E_BADARG
    assert call(nmesh=2 ** 23, max_samples=256) == -3               # DSS_E_UNSUPPORTED: 2^31 lanes
    assert call(max_samples=2 ** 31 - 1) == -3                      # one grid whose padded sample count passes an int
    assert np.all(out == GUARD) and status[0] == -7
    assert call() == 0 and status[0] == 0 and np.isfinite(out).all()


def test_check_mesh_refusals():
    v, f = ref.octasphere(1)
    assert np.array_equal(mesh_grid.check_mesh(v, f)[1], f)
    with pytest.raises(ValueError, match="not watertight"):
        mesh_grid.check_mesh(v, f[:-1])
    flipped = f.copy(); flipped[3] = flipped[3, [0, 2, 1]]
    with pytest.raises(ValueError, match="not consistently oriented"):
        mesh_grid.check_mesh(v, flipped)
    for bad in (len(v), -1):
        worse = f.copy(); worse[5, 1] = bad
        with pytest.raises(ValueError, match="out of range"):
            mesh_grid.check_mesh(v, worse)
    with pytest.raises(ValueError, match="zero volume"):
        mesh_grid.check_mesh(v[:3] + 5.0, np.array([[0, 1, 2], [0, 2, 1]]))
    with pytest.raises(ValueError, match="integers"):
        mesh_grid.check_mesh(v, f.astype(np.float64))
    with pytest.raises(ValueError, match="twice"):
        mesh_grid.check_mesh(v, np.concatenate([f, [[0, 0, 1]]]))
    c = mesh_grid.centroid(*ref.box(at=(0.3, -0.2, 0.1)))
    assert np.abs(c - [0.3, -0.2, 0.1]).max() <= 1e-15


def test_load_obj_on_the_fixture():
    v, f = meshes.load_obj(os.path.join(HERE, "golden", "mesh_grid_cube.obj"))
    assert v.dtype == np.float64 and f.dtype == np.int64 and v.shape == (8, 3) and f.shape == (12, 3)
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
    assert f[:4].tolist() == [[0, 3, 2], [0, 2, 1], [4, 5, 6], [4, 6, 7]] and f[-2:].tolist() == [[1, 2, 6], [1, 6, 5]]
    v2, f2 = mesh_grid.check_mesh(v, f)      # closed, consistently oriented, outward as written
    assert np.array_equal(f2, f) and np.abs(mesh_grid.centroid(v2, f2) - 0.5).max() <= 1e-15


def test_stand_alone_program_under_the_sanitizers():
    out = os.path.join(HERE, "emu", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "check_mesh_grid")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(HERE, "..", "diffsdfsim_amd", "csrc"),
           "-o", exe, os.path.join(HERE, "emu", "check_mesh_grid.cpp")]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        # only a link without the sanitizers' runtimes may fall back to a plain build; any other failure is the program's
        assert "cannot find" in san.stderr and ("asan" in san.stderr or "ubsan" in san.stderr), san.stderr[-2000:]
        subprocess.check_call(cmd)
    print("check_mesh_grid built %s the sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    w = r.stdout.split()
    assert int(w[0]) == 24 and int(w[2]) > 0, r.stdout      # calls walked, samples checked
