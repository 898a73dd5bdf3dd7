"""CPU: dss_igr_grid_adjoint (csrc/igr_grid_adjoint.hip: count, scan, ordered compaction of the non-zero nodes, the MFMA network
over the compacted list, reduction per latent row) through the emulator.

1. Against the long-double restatement: tests/implicit_net.py (igr_helpers.reference, dtype=np.longdouble) at the lattice nodes
   u_k = -1 + 2 i_k / (n_k - 1), contracted with g_grid in long double, for scenes.geometric_init_weights of both network shapes.
   Bound per latent component: GTOL = 1e-11, the per-point bound tests/test_emu_igr_lists.py holds MODE_LATENT to, times sum |g_i|,
   plus n eps sum |g_i d f / d z_l| for the summation of n terms.  measured / bound is printed.
2. The seams: grids of 5^3 (under one chunk), 13^3 = 2197 (one chunk and a ragged one) and (3, 4, 17) samples; no node, one node,
   every node, list lengths at the network's tile (4 points with tangents) and one off; grids that share a latent row, a grid that
   is not a neural one with an all-NaN adjoint, a NaN code that no grid names; the list's capacity at the need and one below;
   guard words behind every output; two calls bit-equal; every refused call leaves outputs and workspace as they were.
   "Every node" is walked on all three grids, the 13^3 one included (2197 points of the 128-wide network, the emulated network's
   longest walk here: full ballots in every iteration of a chunk, more than 256 entries per chunk in the reduction); the scan's
   carry over more than 256 chunks is walked on the device (test_depth_latent_gpu.py).
3. Central differences in the latent code of sum_i w_i f(x_i; z), f from the emulated dss_igr_query_list(DSS_IGR_VALUE), h = 1e-5.
   Tolerance per component: twice the error that the long-double reference's own central difference at that h shows against its
   own analytic Jacobian, plus 4 eps sum |w_i f_i| / h -- measured from the reference, never from the kernel.
4. tests/emu/check_igr_grid_adjoint.cpp, the seams as a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import igr_helpers as H
from emu import emu

HERE = os.path.dirname(os.path.abspath(__file__))
OK, BADARG, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3      # DSS_* (include/diffsdfsim_hip.h)
LMAX = 4                                                # DSS_IGR_LATENT_MAX
GTOL = 1e-11                                            # tests/test_emu_igr_lists.py, MODE_LATENT per point
EPS = np.finfo(np.float64).eps
SENT, NSENT, WSBYTE, TAIL = -7.25, -77, 0xA5, 64        # what outputs, n_nodes and the workspace (and TAIL bytes behind it) hold before a call
NETS = {"bob_spot": (128, 2, 3), "shapenet": (256, 4, 5)}      # width, latent size, seed
STRIDE = 7


@functools.lru_cache(None)
def backend():
    return emu.EmuBackend()


@functools.lru_cache(None)
def network(name):
    from diffsdfsim_amd import scenes
    width, latent, seed = NETS[name]
    Ws, bs = scenes.geometric_init_weights(seed, 0.5, width, latent)
    return Ws, bs, H.packed_on(backend(), Ws, bs)


def codes_for(name, nrow, seed=21, dead=()):
    """[nrow][STRIDE]: columns L.. are NaN (a read past the code shows), rows `dead` are NaN altogether."""
    latent = NETS[name][1]
    c = np.full((nrow, STRIDE), np.nan)
    c[:, :latent] = np.random.default_rng(seed).normal(0, 0.1, (nrow, latent))
    c[list(dead)] = np.nan
    return c


def lattice(dims, idx, dtype):
    """The lattice points of the flat sample indices idx of a grid of `dims` (x slowest): u_k = -1 + 2 i_k / (n_k - 1) in dtype."""
    ijk = np.unravel_index(np.asarray(idx, np.int64), tuple(int(d) for d in dims))
    return np.stack([dtype(-1) + dtype(2) * i.astype(dtype) / dtype(int(n) - 1) for i, n in zip(ijk, dims)], 1)


class Call:
    """One dss_igr_grid_adjoint call on host arrays.  gs: one adjoint [n0,n1,n2] per grid."""

    def __init__(self, name, dims, rows, codes, gs, cap=None):
        self.name = name
        self.dims = np.ascontiguousarray(np.asarray(dims, np.int32).reshape(-1, 3))
        self.rows = np.ascontiguousarray(rows, np.int32)
        self.codes = np.ascontiguousarray(codes, np.float64)
        self.gs = [np.asarray(g, np.float64).reshape(-1) for g in gs]
        sizes = self.dims.astype(np.int64).prod(1)
        assert [len(g) for g in self.gs] == list(sizes)
        self.off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
        self.g = np.ascontiguousarray(np.concatenate(self.gs))
        self.need = sum(int(np.count_nonzero(~(g == 0.0))) for g, r in zip(self.gs, self.rows) if r >= 0)
        self.cap = max(self.need, 1) if cap is None else cap
        self.nlat = len(self.codes)
        self.nbytes = emu.lib().dss_igr_grid_adjoint_workspace_bytes(int(sizes.sum()), self.cap, self.nlat)

    def run(self, **over):
        """-> the return code; .out [nlat][4], .n_nodes and .ws hold what the call left.  over: net=, or a replacement (None = NULL)
        for one of off, dims, rows, codes, g, out, nn, ws, or ngrid, nlat, cap, stride, nbytes."""
        B = backend()
        net = over.pop("net", H.net_struct(B, network(self.name)[2]))
        self.out = np.full(self.nlat * LMAX + 2, SENT)
        self.nn = np.full(3, NSENT, np.int32)
        self.ws = np.full(self.nbytes + TAIL, WSBYTE, np.uint8)
        a = dict(off=self.off, dims=self.dims, rows=self.rows, codes=self.codes, g=self.g, out=self.out, nn=self.nn, ws=self.ws,
                 ngrid=len(self.dims), nlat=self.nlat, cap=self.cap, stride=self.codes.shape[1], nbytes=self.nbytes)
        a.update(over)
        p = lambda x: None if x is None else x.ctypes.data
        rc = emu.lib().dss_igr_grid_adjoint(None if net is None else ctypes.byref(net), a["ngrid"], p(a["off"]), p(a["dims"]), p(a["rows"]),
                                            p(a["codes"]), a["stride"], a["nlat"], p(a["g"]), a["cap"], p(a["out"]), p(a["nn"]), p(a["ws"]),
                                            a["nbytes"], None)
        # the guard words behind g_latent, n_nodes and the workspace, whatever the call returned
        assert np.all(self.out[self.nlat * LMAX:] == SENT) and np.all(self.nn[1:] == NSENT) and np.all(self.ws[self.nbytes:] == WSBYTE)
        return rc

    def result(self):
        return self.out[:self.nlat * LMAX].reshape(self.nlat, LMAX)

    def untouched(self, n_nodes_too=True):
        return bool(np.all(self.out == SENT) and (not n_nodes_too or self.nn[0] == NSENT))

    def restate(self, dtype):
        """-> (g_latent [nlat][L], bound [nlat][L]) in `dtype`: the sum over the non-zero nodes of the row's grids, and the bound of
        the module's text."""
        Ws, bs, _P = network(self.name)
        latent = NETS[self.name][1]
        val, absg, terms, n = np.zeros((self.nlat, latent), dtype), np.zeros(self.nlat), np.zeros((self.nlat, latent)), np.zeros(self.nlat)
        for dims, r, g in zip(self.dims, self.rows, self.gs):
            nz = np.nonzero(~(g == 0.0))[0]
            if r < 0 or not len(nz):
                continue
            J = H.reference(Ws, bs, lattice(dims, nz, dtype), self.codes[r:r + 1], dtype=dtype)[1]
            w = g[nz].astype(dtype)[:, None]
            val[r] += (w * J).sum(0)
            absg[r] += np.abs(g[nz]).sum(); terms[r] += np.abs(w * J).sum(0).astype(np.float64); n[r] += len(nz)
        return val, GTOL * absg[:, None] + n[:, None] * EPS * terms

    def check(self, dtype=np.float64, what=""):
        """Runs, and holds every row to the restatement in `dtype`; -> the result."""
        assert self.run() == OK
        assert self.nn[0] == self.need
        got, latent = self.result(), NETS[self.name][1]
        want, bound = self.restate(dtype)
        assert np.all(got[:, latent:] == 0.0)                          # slots >= L are exact zeros
        named = np.isin(np.arange(self.nlat), self.rows[self.rows >= 0])
        live = np.array([any(r == k and np.any(g != 0.0) for r, g in zip(self.rows, self.gs)) for k in range(self.nlat)])
        assert np.all(got[~named] == 0.0) and np.all(got[named & ~live] == 0.0)      # exact zeros: a row nobody names, a row without a node
        err = np.abs(got[:, :latent] - want).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            print("%s %s: measured / bound per row and component\n%s" % (self.name, what, np.where(bound > 0, err / bound, 0.0)))
        assert np.all(np.isfinite(got)) and np.all(err[live] <= bound[live])
        return got


def sparse(dims, idx, seed=0):
    """An adjoint of `dims` that is zero but for random weights at the flat indices idx."""
    g = np.zeros(int(np.prod(dims)))
    g[np.asarray(idx, int)] = np.random.default_rng(seed).normal(0, 1.0, len(idx))
    assert np.all(g[np.asarray(idx, int)] != 0.0)
    return g


# ---- 1: against the long-double restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nodes", [("bob_spot", 24), ("shapenet", 9)])
def test_kernel_matches_the_long_double_restatement(name, nodes):
    """A 13^3 grid (two chunks) with `nodes` non-zero samples, among them the last of the first chunk, the first of the second and
    the grid's last, and a second grid of (3, 4, 17) on another latent row."""
    r = np.random.default_rng(31)
    idx = np.unique(np.concatenate([[2047, 2048, 2196], r.choice(2197, nodes - 3, replace=False)]))
    c = Call(name, [(13, 13, 13), (3, 4, 17)], [1, 0], codes_for(name, 2),
             [sparse((13, 13, 13), idx, 1), sparse((3, 4, 17), [0, 67, 203], 2)])
    c.check(np.longdouble, "long double")


# ---- 2: the seams --------------------------------------------------------------------------------------------------------------
GRIDS = {"5": (5, 5, 5), "13": (13, 13, 13), "3x4x17": (3, 4, 17)}
PATTERNS = {"none": 0, "one": 1, "tile-1": 3, "tile": 4, "tile+1": 5}      # list lengths; the tangent tile of a short list is 4 points


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_list_lengths_around_the_network_tile(grid, pattern):
    dims, n = GRIDS[grid], PATTERNS[pattern]
    size = int(np.prod(dims))
    # the grid's last sample first (its corner u = +1), then samples spread over the grid: on the 13^3 grid over both chunks
    idx = [size - 1, 0, size // 2 + 1, size - 2 - size // 16, size // 3][:n]
    c = Call("bob_spot", [dims], [0], codes_for("bob_spot", 1), [sparse(dims, idx, 3)])
    got = c.check(what="%s %s" % (grid, pattern))
    if n == 0:
        assert np.all(got == 0.0)
    else:
        assert np.abs(got[0, :2]).min() > 1e-6      # (nothing passes by being zero)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_every_node(grid):
    dims = GRIDS[grid]
    g = np.random.default_rng(4).normal(0, 1.0, dims)
    Call("bob_spot", [dims], [0], codes_for("bob_spot", 1), [g]).check(what="%s every node" % grid)


@functools.lru_cache(None)
def combination():
    """Four grids: 0 and 2 share latent row 0, 1 is not a neural grid (lat_idx -1) and its adjoint is all NaN, 3 names row 2; row 1,
    which nobody names, is a NaN code."""
    dims = [(5, 5, 5), (3, 4, 17), (13, 13, 13), (5, 5, 5)]
    gs = [sparse(dims[0], [3, 77, 124], 5), np.full(dims[1], np.nan), sparse(dims[2], [5, 2047, 2048, 2100, 2196], 6), sparse(dims[3], [0, 62], 7)]
    return Call("shapenet", dims, [0, -1, 0, 2], codes_for("shapenet", 3, dead=[1]), gs)


def test_shared_rows_a_skipped_nan_grid_and_an_unnamed_nan_code():
    c = combination()
    got = c.check(what="combination")
    assert np.all(got[1] == 0.0) and np.all(np.isfinite(got[[0, 2]])) and np.abs(got[[0, 2]]).min() > 1e-6
    # row 0 is the sum of its two grids, each alone, to the rounding of one addition per component
    alone = [Call("shapenet", [c.dims[k]], [0], c.codes, [c.gs[k]]).check(what="grid %d alone" % k)[0] for k in (0, 2)]
    assert np.all(np.abs(got[0] - (alone[0] + alone[1])) <= 2 * EPS * (np.abs(alone[0]) + np.abs(alone[1])))
    # two calls return the same bits
    first = got.copy()
    assert c.run() == OK and np.array_equal(c.result(), first)


def test_a_nan_weight_propagates():
    g = sparse((5, 5, 5), [7, 30], 8)
    g[30] = np.nan
    c = Call("bob_spot", [(5, 5, 5)], [0], codes_for("bob_spot", 1), [g])
    assert c.run() == OK and c.nn[0] == 2 and np.all(np.isnan(c.result()[0, :2])) and np.all(c.result()[0, 2:] == 0.0)


def test_capacity_at_the_need_and_one_below():
    dims, idx = (13, 13, 13), [1, 2047, 2048, 2049, 2196]
    exact = Call("bob_spot", [dims], [0], codes_for("bob_spot", 1), [sparse(dims, idx, 9)], cap=5)
    got = exact.check(what="cap = need").copy()
    roomy = Call("bob_spot", [dims], [0], exact.codes, exact.gs, cap=64)
    assert roomy.run() == OK and np.array_equal(roomy.result(), got)      # (the capacity does not reach the bits)
    short = Call("bob_spot", [dims], [0], exact.codes, exact.gs, cap=4)
    assert short.run() == WORKSPACE and short.nn[0] == 5 and short.untouched(n_nodes_too=False)


def test_every_refused_call_leaves_outputs_and_workspace_untouched():
    c = combination()
    B = backend()
    P = network("shapenet")[2]
    bad_dims = c.dims.copy(); bad_dims[2, 1] = 1
    bad_rows = c.rows.copy(); bad_rows[3] = 3
    refused = [(BADARG, dict(net=None)), (BADARG, dict(ngrid=0)), (BADARG, dict(nlat=0)), (BADARG, dict(cap=0)), (BADARG, dict(cap=-3)),
               (BADARG, dict(stride=3)), (BADARG, dict(dims=bad_dims)), (BADARG, dict(rows=bad_rows)),
               (UNSUPPORTED, dict(net=H.net_struct(B, P, width=192))), (UNSUPPORTED, dict(net=H.net_struct(B, P, latent=2))),
               (WORKSPACE, dict(nbytes=64))]      # (the size function is a bound for any split into grids: far below it)
    refused += [(BADARG, {k: None}) for k in ("off", "dims", "rows", "codes", "g", "out", "nn", "ws")]
    from diffsdfsim_amd import world_abi
    for k in world_abi.IGR_NET_POINTERS:
        broken = H.net_struct(B, P)
        setattr(broken, k, None)
        refused.append((BADARG, dict(net=broken)))
    for want, over in refused:
        assert c.run(**over) == want, over
        assert c.untouched() and np.all(c.ws == WSBYTE), over
    assert emu.lib().dss_igr_grid_adjoint_workspace_bytes(0, 8, 1) == 0 and emu.lib().dss_igr_grid_adjoint_workspace_bytes(8, 0, 1) == 0
    assert emu.lib().dss_igr_grid_adjoint_workspace_bytes(8, 8, 0) == 0


# ---- 3: central differences in the latent code ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_central_differences_in_the_latent_code(name):
    Ws, bs, P = network(name)
    latent, h = NETS[name][1], 1e-5
    dims, idx = (5, 5, 5), [4, 31, 62, 90, 124]
    c = Call(name, [dims], [0], codes_for(name, 1), [sparse(dims, idx, 10)])
    assert c.run() == OK
    got = c.result()[0, :latent]
    w, z = c.gs[0][idx], c.codes[0, :latent]
    pts64, ptsld = lattice(dims, idx, np.float64), lattice(dims, idx, np.longdouble)
    wl = w.astype(np.longdouble)

    def ref_sum(code):
        return (wl * H.reference(Ws, bs, ptsld, code[None], dtype=np.longdouble)[0]).sum()

    analytic = (wl[:, None] * H.reference(Ws, bs, ptsld, z.astype(np.longdouble)[None], dtype=np.longdouble)[1]).sum(0)
    f0 = H.query_list(backend(), P, pts64, c.codes, 2)[0]
    for l in range(latent):
        e = np.zeros(STRIDE); e[l] = h
        table = lambda s: np.where(np.isnan(c.codes), np.nan, c.codes + s * e)
        cd = ((w * H.query_list(backend(), P, pts64, table(+1), 2)[0]).sum() - (w * H.query_list(backend(), P, pts64, table(-1), 2)[0]).sum()) / (2 * h)
        el = e[:latent].astype(np.longdouble)
        ref_cd = (ref_sum(z.astype(np.longdouble) + el) - ref_sum(z.astype(np.longdouble) - el)) / (2 * np.longdouble(h))
        tol = 2 * abs(float(ref_cd - analytic[l])) + 4 * EPS * np.abs(w * f0).sum() / h
        print("%s latent %d: kernel %.12e  central difference %.12e  |diff| %.3e  tolerance %.3e" % (name, l, got[l], cd, abs(got[l] - cd), tol))
        assert abs(got[l] - cd) <= tol


# ---- 4: the sanitizer program --------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_the_sanitizers():
    out = os.path.join(HERE, "emu", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "check_igr_grid_adjoint")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w", "-DDSS_EMU", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(HERE, "..", "diffsdfsim_amd", "csrc"),
           "-o", exe, os.path.join(HERE, "emu", "check_igr_grid_adjoint.cpp")]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        # only a link without the sanitizers' runtimes may fall back to a plain build; any other failure is the program's
        assert "cannot find" in san.stderr and ("asan" in san.stderr or "ubsan" in san.stderr), san.stderr[-2000:]
        subprocess.check_call(cmd)
    print("check_igr_grid_adjoint built %s the sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    w = r.stdout.split()
    assert int(w[0]) >= 8 and int(w[2]) > 0, r.stdout      # calls walked, nodes compacted
