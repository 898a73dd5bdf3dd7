"""Shared launch and assertions of dss_pointcloud_loss_igr (csrc/pointcloud_loss_igr.hip) against
tests/golden/pointcloud_loss_igr.npz (tools/gen_pointcloud_igr_golden.py): used by tests/test_emu_pointcloud_loss_igr.py with
emu.EmuBackend (the CPU emulator) and by tests/test_pointcloud_loss_igr_gpu.py with engine.TorchBackend (the device library).

The golden holds two networks (seeded geometric-init weights, rebuilt here from the seeds): 0 = 128 wide, latent 2; 1 = 256 wide,
latent 4.  The entry point takes one network per call, so a call covers (a subset of) one network's segments.

Tolerance.  Counts are exact (the generator keeps every point 1e-6 scale from its cube's faces).  Every other output is held to
max(16 d_ref, 1e-12 abs_sum): d_ref is the distance of the reference's own float64 result from the long-double restatement of the
same terms, and 16 x is the margin over the reference's rounding that tests/test_mesh_chain_gpu.py gives a second float64
evaluation with a different operation order (here: the MFMA accumulation order, the hand-written softplus, forward-mode tangents
where the reference runs a reverse sweep, and another summation tree); 1e-12 abs_sum is the floor of the sibling point-cloud tests,
some 2^12 ulp of the summands, for outputs whose reference happened to round almost exactly.
"""
import ctypes
import functools
import os

import numpy as np

import igr_helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointcloud_loss_igr.npz")
OUT = 13
SENTINEL = H.SENTINEL
LAT_STRIDE = 5          # wider than either latent size: the stride is an argument of its own


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    g["names"] = [str(n) for n in g["names"]]
    return g


@functools.lru_cache(maxsize=None)
def weights(k):
    from diffsdfsim_amd.scenes import geometric_init_weights
    g = golden()
    return geometric_init_weights(int(g["net_seed"][k]), float(g["net_radius"][k]), int(g["net_width"][k]), int(g["net_latent"][k]))


def latent_size(k):
    return int(golden()["net_latent"][k])


def segments_of(k):
    """Golden rows of network k, in file order."""
    return [int(s) for s in np.nonzero(golden()["net"] == k)[0]]


def index_of(k, name):
    g = golden()
    return next(s for s in segments_of(k) if g["names"][s] == name)


def latent_table(k, poison=True):
    """[rows + 1][LAT_STRIDE]: the golden's codes in the first L columns; the columns past L and one row no segment names are NaN."""
    z = golden()["latents_%d" % k]
    T = np.full((len(z) + 1, LAT_STRIDE), np.nan if poison else 0.0)
    T[:len(z), :z.shape[1]] = z
    return T


def inputs(ids, pose=None, lat_rows=None):
    """Host arrays of a call over golden rows `ids` (of one network): the segments' points packed in that order."""
    g = golden()
    off = g["seg_off"]
    pts = np.concatenate([g["pts"][off[s]:off[s + 1]] for s in ids] + [np.zeros((0, 3))])
    lens = [int(off[s + 1] - off[s]) for s in ids]
    return dict(pts=np.ascontiguousarray(pts), seg_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), max_len=max(lens),
                pose=np.ascontiguousarray(g["pose"][ids] if pose is None else pose, dtype=np.float64),
                scale=np.ascontiguousarray(g["scale"][ids]), lat_idx=np.ascontiguousarray(g["lat_row"][ids] if lat_rows is None else lat_rows, dtype=np.int32))


def raw_call(backend, net, nseg, max_len, seg_off, pts, pose, scale, lat_idx, latents, stride, n_pts, out, ws, nbytes):
    """The bare call: `net` a DssIgrNet or None, every array one of `backend`'s or None (NULL).  -> the return code."""
    a = lambda x: None if x is None else backend.ptr(x)
    return backend.lib.dss_pointcloud_loss_igr(None if net is None else ctypes.byref(net), int(nseg), int(max_len), a(seg_off), a(pts), a(pose),
                                               a(scale), a(lat_idx), a(latents), int(stride), int(n_pts), a(out), a(ws), int(nbytes),
                                               backend.stream())


class Call:
    """Arrays of one call on `backend`, kept so that the return-code tests can knock single arguments out."""

    def __init__(self, backend, packed, k, ids, pose=None, table=None, lat_rows=None):
        self.backend, self.k, self.ids = backend, k, list(ids)
        I = inputs(self.ids, pose, lat_rows)
        self.nseg, self.max_len, self.n_pts = len(self.ids), I["max_len"], len(I["pts"])
        up = backend.from_numpy
        self.net = H.net_struct(backend, packed)
        self.arr = dict(seg_off=up(I["seg_off"]), pts=up(I["pts"]) if self.n_pts else None, pose=up(I["pose"]), scale=up(I["scale"]),
                        lat_idx=up(I["lat_idx"]), latents=up(latent_table(k) if table is None else table))
        self.stride = LAT_STRIDE if table is None else int(np.shape(table)[1])
        self.nbytes = backend.lib.dss_pointcloud_loss_igr_workspace_bytes(self.nseg, self.max_len, self.n_pts)
        assert self.nbytes % 8 == 0
        self.ws = up(np.zeros(self.nbytes // 8)) if self.nbytes else None      # exactly the advertised size
        self.out = up(np.full((self.nseg, OUT), SENTINEL))

    def run(self, **over):
        """-> return code; over: net, nseg, max_len, stride, n_pts, nbytes, or an array's name (None = NULL)."""
        A = dict(self.arr, out=self.out, ws=self.ws)
        A.update({n: v for n, v in over.items() if n in A})
        s = lambda n: over.get(n, getattr(self, n))
        return raw_call(self.backend, s("net"), s("nseg"), s("max_len"), A["seg_off"], A["pts"], A["pose"], A["scale"], A["lat_idx"],
                        A["latents"], s("stride"), s("n_pts"), A["out"], A["ws"], s("nbytes"))

    def result(self):
        return np.array(self.backend.to_numpy(self.out))


def launch(backend, packed, k, ids, **kw):
    c = Call(backend, packed, k, ids, **kw)
    rc = c.run()
    assert rc == 0, rc
    return c.result()


def bound(s):
    g = golden()
    return np.maximum(16.0 * g["d_ref"][s], 1e-12 * g["abs_sum"][s])


def check_against_golden(out, ids, label):
    """Counts exact, every other output within max(16 d_ref, 1e-12 abs_sum); prints measured / bound per segment."""
    g = golden()
    worst = []
    for row, s in zip(out, ids):
        b = bound(s)
        err = np.abs(row - g["out"][s])
        ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))
        print("%s net %d %-13s inside %4d  measured / bound %.3f" % (label, int(g["net"][s]), g["names"][s], int(g["out"][s, 1]), ratio))
        worst.append((ratio, g["names"][s]))
    for row, s, (ratio, name) in zip(out, ids, worst):
        assert row[1] == g["out"][s, 1], (name, row[1], g["out"][s, 1])
        assert ratio <= 1.0, (name, ratio, row, g["out"][s])


def check_exact_zeros(out, ids, k):
    """Segments without a point inside are exactly 0 everywhere; latent slots past L are exactly 0; no slot keeps the sentinel."""
    g = golden()
    L = latent_size(k)
    assert not np.any(out == SENTINEL) and np.all(np.isfinite(out))
    for row, s in zip(out, ids):
        if g["out"][s, 1] == 0:
            assert np.all(row == 0.0), g["names"][s]
        assert np.all(row[9 + L:] == 0.0), g["names"][s]


def named(k, names):
    return [index_of(k, n) for n in names]


def many_segments(n=257):
    """n golden segments (network 0) of a handful of points each (an empty one among them), cycled: one chunk per segment, so the
    call has n workgroups and the scan of their counts carries over a tile of 256."""
    pick = named(0, ["one_point", "fd_nonunit_6", "empty", "pair_a", "nonunit_25"])
    return [pick[i % len(pick)] for i in range(n)]


def central_difference_segments(k, name="mixed_257", h=1e-6):
    """2 (7 + L) copies of one golden segment, each with one pose component or one latent coordinate moved by +-h: one call gives
    every value the central differences need.  -> ids, pose [n][7], latent table, lat_rows."""
    g = golden()
    s, L = index_of(k, name), latent_size(k)
    n = 2 * (7 + L)
    pose = np.repeat(g["pose"][s][None], n, 0)
    table = np.zeros((n, LAT_STRIDE))
    table[:, :L] = g["latents_%d" % k][g["lat_row"][s]]
    for j in range(7 + L):
        for sign, row in ((1.0, 2 * j), (-1.0, 2 * j + 1)):
            if j < 7:
                pose[row, j] += sign * h
            else:
                table[row, j - 7] += sign * h
    return [s] * n, pose, table, np.arange(n, dtype=np.int32)


def check_central_differences(out_fd, out0, k, name="mixed_257", h=1e-6):
    """(loss(+h) - loss(-h)) / 2h against the kernel's Jacobian, to 1e-5 of abs_sum of the differentiated output."""
    g = golden()
    s, L = index_of(k, name), latent_size(k)
    fd = (out_fd[0::2, 0] - out_fd[1::2, 0]) / (2 * h)
    an = np.concatenate([out0[2:9], out0[9:9 + L]])
    scale = np.concatenate([g["abs_sum"][s][2:9], g["abs_sum"][s][9:9 + L]])
    print("central differences net %d: worst |fd - jac| / abs_sum %.3e" % (k, float(np.max(np.abs(fd - an) / scale))))
    assert np.all(out_fd[:, 1] == out0[1])      # no point crossed a face
    assert np.all(np.abs(fd - an) <= 1e-5 * scale), (fd, an)


def check_return_codes(backend, packed, k):
    """Workspace one byte short, lat_stride < L, null pointers, a network shape that is not built: nothing is written."""
    ids = [index_of(k, "one_point")] * 2      # (short: the call that succeeds at the end runs the network)
    c = Call(backend, packed, k, ids)
    L = latent_size(k)
    assert c.nbytes > 0
    assert c.run(nbytes=c.nbytes - 1) == -2 and c.run(ws=None) == -2                     # DSS_E_WORKSPACE
    assert c.run(stride=L - 1) == -1                                                     # DSS_E_BADARG
    for name in ("seg_off", "pts", "pose", "scale", "lat_idx", "latents", "out"):
        assert c.run(**{name: None}) == -1, name
    assert c.run(net=None) == -1 and c.run(nseg=0) == -1 and c.run(max_len=-1) == -1 and c.run(n_pts=-1) == -1
    from diffsdfsim_amd import world_abi
    holes = world_abi.DssIgrNet(*[getattr(c.net, f) for f in world_abi.IGR_NET_POINTERS[:-1]], None, c.net.width, c.net.latent)
    assert c.run(net=holes) == -1
    assert c.run(net=H.net_struct(backend, packed, width=192)) == -3                     # DSS_E_UNSUPPORTED
    assert np.all(c.result() == SENTINEL)
    lib = backend.lib
    assert lib.dss_pointcloud_loss_igr_workspace_bytes(0, 5, 5) == 0 and lib.dss_pointcloud_loss_igr_workspace_bytes(1, 0, 5) == 0
    assert c.run() == 0 and not np.any(c.result() == SENTINEL)                           # a workspace of exactly the advertised size
