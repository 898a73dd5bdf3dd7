"""GPU: dss_pointcloud_loss_igr (csrc/pointcloud_loss_igr.hip) on the device against tests/golden/pointcloud_loss_igr.npz, the
reference's match_pointcloud arithmetic over SDF3D.query_sdfs and decode_igr with torch autograd
(tools/gen_pointcloud_igr_golden.py).  Cases, tolerance and its derivation: tests/pointcloud_igr_cases.py; the emulator twin is
tests/test_emu_pointcloud_loss_igr.py.  Here every golden segment of both networks runs, the central differences are taken on
mixed_257, and a dense 4133-point segment is compared against igr.igr_query plus torch double arithmetic on the device.

Measured / bound on the MI355X (bound = max(16 d_ref, 1e-12 abs_sum); worst output of the segment):
    128-wide, latent 2   mixed_257 0.001  one_point 0.011  sparse_4133 0.003  nonunit_quat 0.001  pair_a 0.002  pair_b 0.002
                         shared_a 0.001  shared_b 0.001  mixed_33 0.002  nonunit_25 0.002  fd_nonunit_6 0.002  dense_4133 0.002
                         (empty, all_outside: exactly 0)
    256-wide, latent 4   mixed_257 0.001  pair_a 0.002  pair_b 0.002  one_point 0.085  mixed_12 0.005  small_a 0.010  small_b 0.003
                         dense_4133 0.003
Central differences (h = 1e-6) on mixed_257: worst |fd - Jacobian| / abs_sum 2.6e-10 (128-wide), 4.2e-10 (256-wide), bound 1e-5.
"""
import numpy as np
import pytest
import torch

import igr_helpers as H
import pointcloud_igr_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from diffsdfsim_amd.engine import TorchBackend
    return TorchBackend("cuda:0")


@pytest.fixture(scope="module")
def packed(backend):
    return {k: H.packed_on(backend, *C.weights(k)) for k in (0, 1)}


@pytest.fixture(scope="module")
def full(backend, packed):
    """One call per network over all of its golden segments, shared by the tests below and left unchanged."""
    return {k: C.launch(backend, packed[k], k, C.segments_of(k)) for k in (0, 1)}


@pytest.mark.parametrize("k", [0, 1])
def test_every_segment_matches_the_reference_golden(full, k):
    C.check_against_golden(full[k], C.segments_of(k), "MI355X")


@pytest.mark.parametrize("k", [0, 1])
def test_every_slot_is_written_and_the_zeros_are_exact(full, k):
    C.check_exact_zeros(full[k], C.segments_of(k), k)


@pytest.mark.parametrize("k", [0, 1])
def test_a_subset_of_segments_returns_the_rows_of_the_full_call_and_two_calls_the_same_bits(backend, packed, full, k):
    ids = C.segments_of(k)
    pick = ids[::-2] if k == 0 else ids[1:]      # other offsets in the list, other tile mates, another launch shape
    sub = C.launch(backend, packed[k], k, pick)
    for row, s in zip(sub, pick):
        assert np.array_equal(row, full[k][ids.index(s)]), C.golden()["names"][s]
    assert np.array_equal(C.launch(backend, packed[k], k, pick), sub)
    assert np.array_equal(C.launch(backend, packed[k], k, ids), full[k])


def test_only_empty_segments_need_no_workspace_and_give_zeros(backend, packed):
    c = C.Call(backend, packed[0], 0, [C.index_of(0, "empty")] * 2)
    assert c.nbytes == 0 and c.run() == 0 and np.all(c.result() == 0.0)


def test_257_workgroups_carry_the_scan_over_a_tile(backend, packed, full):
    ids = C.many_segments()
    out = C.launch(backend, packed[0], 0, ids)
    C.check_against_golden(out[:5], ids[:5], "gpu 257")
    C.check_exact_zeros(out, ids, 0)
    for row, s in zip(out, ids):      # a segment's row does not depend on where the list puts its points
        assert np.array_equal(row, full[0][C.segments_of(0).index(s)]), C.golden()["names"][s]


@pytest.mark.parametrize("k", [0, 1])
def test_central_differences_in_pose_and_latent(backend, packed, full, k):
    ids, pose, table, rows = C.central_difference_segments(k)
    out = C.launch(backend, packed[k], k, ids, pose=pose, table=table, lat_rows=rows)
    C.check_central_differences(out, full[k][C.segments_of(k).index(ids[0])], k)


@pytest.mark.parametrize("k", [0, 1])
def test_return_codes(backend, packed, k):
    C.check_return_codes(backend, packed[k], k)


def built_segment(backend, packed, k, r, pb, scale):
    """One segment built here from body-frame points pb (each 1e-6 scale or more from the cube's faces; a random pose from r): the
    terms of the points inside from igr.igr_query (the same network kernel on the uncompacted points) and torch double arithmetic
    on the device.  d_ref = the distance between torch's sum over the points in index order (cumsum) and its own tree (sum): the
    bound is max(16 d_ref, 1e-12 abs_sum) as for the golden.  -> out [13], tree, bound, inside [n] (bool), the workspace's ints."""
    from diffsdfsim_amd import igr
    g, L = C.golden(), C.latent_size(k)
    dev = backend.device
    q = r.standard_normal(4); q *= 1.1 / np.linalg.norm(q)
    pos = r.uniform(-1, 1, 3)
    z = g["latents_%d" % k][1]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)
    qt, post = t(q), t(pos)
    rr, i, j, kk = qt
    s2 = 2.0 / (qt @ qt)
    N = torch.stack([torch.stack([-(j * j + kk * kk), i * j - kk * rr, i * kk + j * rr]), torch.stack([i * j + kk * rr, -(i * i + kk * kk), j * kk - i * rr]),
                     torch.stack([i * kk - j * rr, j * kk + i * rr, -(i * i + j * j)])])
    R = torch.eye(3, dtype=torch.float64, device=dev) + s2 * N
    x = (t(pb(r) if callable(pb) else pb) @ R.T + post).contiguous()
    n = len(x)
    d_all = x - post
    p_all = d_all @ R
    inside = (p_all.abs() < scale * (1 - 1e-6)).all(1)
    assert bool((inside | (p_all.abs() > scale * (1 + 1e-6)).any(1)).all())      # nobody near a face
    d, p = d_all[inside], p_all[inside]
    u = (p / scale).contiguous()
    phi, gu = igr.igr_query(u, t(z), packed[k])
    _phi, gz = igr.igr_query(u, t(z), packed[k], wrt="latent")
    gp = (2 * scale * phi)[:, None] * gu
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    dN = [torch.stack([torch.stack([zero, -kk, j]), torch.stack([kk, zero, -i]), torch.stack([-j, i, zero])]),
          torch.stack([torch.stack([zero, j, kk]), torch.stack([j, -2 * i, -rr]), torch.stack([kk, rr, -2 * i])]),
          torch.stack([torch.stack([-2 * j, i, rr]), torch.stack([i, zero, kk]), torch.stack([-rr, kk, -2 * j])]),
          torch.stack([torch.stack([-2 * kk, -rr, i]), torch.stack([rr, -2 * kk, j]), torch.stack([i, j, zero])])]
    T = torch.zeros(len(u), C.OUT, dtype=torch.float64, device=dev)
    T[:, 0] = (scale * phi) ** 2
    T[:, 1] = 1
    for m in range(4):
        T[:, 2 + m] = torch.einsum("nj,ji,ni->n", d, s2 * dN[m] - s2 * s2 * qt[m] * N, gp)
    T[:, 6:9] = -gp @ R.T
    T[:, 9:9 + L] = (2 * scale * scale * phi)[:, None] * gz[:, :L]
    tree, serial, abs_sum = T.sum(0).cpu().numpy(), T.cumsum(0)[-1].cpu().numpy(), T.abs().sum(0).cpu().numpy()
    bound = np.maximum(16 * np.abs(tree - serial), 1e-12 * abs_sum)
    table = np.zeros((2, C.LAT_STRIDE)); table[1, :L] = z
    up = backend.from_numpy
    lib = backend.lib
    nbytes = lib.dss_pointcloud_loss_igr_workspace_bytes(1, n, n)
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    out = up(np.full((1, C.OUT), C.SENTINEL))
    arrs = [up(np.array([0, n], np.int32)), x, up(np.concatenate([q, pos])[None]), up(np.array([scale])), up(np.array([1], np.int32)), up(table)]
    rc = C.raw_call(backend, H.net_struct(backend, packed[k]), 1, n, *arrs, C.LAT_STRIDE, n, out, ws, nbytes)
    assert rc == 0
    nwg = (n + 2047) // 2048      # the workspace (pointcloud_loss_igr.hip: pci_layout): doubles, then counts, offs, total[2], qlat, qsrc
    ints = ws[nwg * C.OUT + 11 * n:].view(torch.int32).cpu().numpy()
    return backend.to_numpy(out)[0], tree, bound, inside.cpu().numpy(), ints


@pytest.mark.parametrize("k", [0, 1])
def test_dense_4133_points_all_inside_against_igr_query_and_torch(backend, packed, k):
    """Three chunks, every point inside."""
    r = np.random.default_rng(5 + k)
    n, scale = 4096 + 37, 0.9
    got, tree, bound, inside, _ints = built_segment(backend, packed, k, r, lambda r: r.uniform(-0.97 * scale, 0.97 * scale, (n, 3)), scale)
    err = np.abs(got - tree)
    print("MI355X net %d dense_4133 measured / bound %.3f" % (k, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0)))))
    assert inside.all() and got[1] == n and np.all(err <= bound), (got, tree, bound)


def seam_points(shape, r, scale):
    """2049: every point inside (a full chunk of all-ones ballots, then a chunk whose only live lane is thread 0 of its first
    iteration); 64_64: 64 points inside, then 64 outside (an all-ones and an all-zero ballot, lane 63 the last one in)."""
    n, n_in = (2049, 2049) if shape == "2049" else (128, 64)
    pb = r.uniform(-0.97 * scale, 0.97 * scale, (n, 3))
    axis = r.integers(0, 3, n - n_in)
    pb[np.arange(n_in, n), axis] = r.choice([-1.0, 1.0], n - n_in) * r.uniform(1.03 * scale, 1.5 * scale, n - n_in)
    return pb


@pytest.mark.parametrize("shape", ["2049", "64_64"])
@pytest.mark.parametrize("k", [0, 1])
def test_full_and_empty_ballots_and_a_chunk_of_one_point(backend, packed, k, shape):
    """The compaction's edges on a segment built here: counts, offsets, total and the order of the emitted source rows are exact,
    the sums within built_segment's bound."""
    r = np.random.default_rng(11 + k)
    scale = 0.9
    pb = seam_points(shape, r, scale)
    got, tree, bound, inside, ints = built_segment(backend, packed, k, r, pb, scale)
    n, nwg = len(pb), (len(pb) + 2047) // 2048
    want = np.array([64] if shape == "64_64" else [2048, 1])
    assert np.array_equal(inside, np.arange(n) < want.sum())
    counts, offs, total, qsrc = ints[:nwg], ints[nwg:2 * nwg], ints[2 * nwg], ints[2 * nwg + 2 + n:2 * nwg + 2 + 2 * n]
    assert np.array_equal(counts, want) and np.array_equal(offs, np.cumsum(want) - want) and total == want.sum()
    assert np.array_equal(qsrc[:total], np.nonzero(inside)[0])
    err = np.abs(got - tree)
    print("MI355X net %d %s measured / bound %.3f" % (k, shape, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0)))))
    assert got[1] == want.sum() and np.all(err <= bound), (got, tree, bound)
