"""Contacts between 2-D SDF bodies on the device, behind the reference's contact-handler seam.

`sdf_physics.physics.contacts.SDFContactHandler` walks every edge of one body's outline with a Frank-Wolfe search over the
other body's SDF, in both directions, and thins what it finds by a PCA and a convex hull.  `csrc/sdf2d_contacts.hip`
(``dss_sdf2d_contacts_forward`` / ``_backward``, include/sdf2d_contacts.h) does that for P pairs per launch, one wavefront per
pair; `sdf_contacts2d` is the batched, differentiable operator, `SDFContactHandler` the class for the reference's
``World(..., contact_callback=SDFContactHandler)``, and `physics2d.World` sends its pairs of SDF bodies here.

Gradients reach poses, shape parameters and scales of both bodies, and a grid body's samples: `GridTable` pools samples,
central differences and outline vertices without detaching them, ``dss_sdf2d_contacts_backward_grids`` returns the gradient
with respect to those three arrays as independent inputs (the reference's graph: `sdf`, `sdf_grads`, `verts` are separate
tensors there), and autograd chains them back to the samples (`sdf_bodies`: the central differences; the outline derivative
this build defines).  A foreign grid body without `unit_verts` (the reference's own SDFGrid behind this handler) keeps `sdf`
and `sdf_grads` connected and its outline detached.  Pairs of one launch that share a grid add into its gradient with
atomics: such gradients agree between two calls to round-off, not to the bit.
Within a pair the contacts come in candidate order (body 1's edges in order, then body 2's), not in the order Qhull lists hull
vertices in."""
import ctypes

import torch

from .. import _lib
from ..world_abi import (SDF2D_BOWL, SDF2D_CIRCLE, SDF2D_GRID, SDF2D_GRID_FIELDS, SDF2D_MAXCAND, SDF2D_MALFORMED, SDF2D_OVER_CAND,
                         SDF2D_RECT, DssSdf2dGrids)

DEFAULT_CAP = 16


class GridTable:
    """The grid bodies of a set of pairs pooled into the arrays of DssSdf2dGrids on one device (the manner of grids.GridTable).
    `sources`: objects with `sdf` [n0, n1], `sdf_grads` [n0, n1, 2], outline vertices at unit scale and `edges`.  The float
    arrays (`tensors["vals" | "grads" | "verts"]`) are torch.cat's of the sources' own tensors and stay on their graph."""

    def __init__(self, sources, device):
        self.ids = {}
        dims, val_off, vert_off, edge_off, vals, grads, verts, edges = [], [], [0], [0], [], [], [], []
        for b in sources:
            if id(b) in self.ids:
                continue
            self.ids[id(b)] = len(dims) // 2
            # the three float arrays stay on the graph of the samples.  A body without `unit_verts` (the reference's own
            # SDFGrid) gives its outline detached: the reference's graph cannot carry that gradient (unique(dim=0))
            sdf = b.sdf
            unit = b.unit_verts if hasattr(b, "unit_verts") else b.verts.detach() / b.scale.detach()
            dims += [sdf.shape[0], sdf.shape[1]]
            val_off.append(sum(v.numel() for v in vals))
            vals.append(sdf.reshape(-1)); grads.append(b.sdf_grads.reshape(-1))
            verts.append(unit.reshape(-1)); edges.append(b.edges.reshape(-1))
            vert_off.append(vert_off[-1] + len(unit)); edge_off.append(edge_off[-1] + len(b.edges))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(device)      # noqa: E731
        f64 = lambda v: (torch.cat([x.to("cpu", torch.float64) for x in v]) if v else torch.zeros(0, dtype=torch.float64)).to(device).contiguous()   # noqa: E731
        self.tensors = dict(dims=i32(dims), val_off=i32(val_off), vert_off=i32(vert_off), edge_off=i32(edge_off),
                            edges=(torch.cat([e.to("cpu", torch.int32) for e in edges]) if edges else torch.zeros(0, dtype=torch.int32)).to(device).contiguous(),
                            vals=f64(vals), grads=f64(grads), verts=f64(verts))
        self.struct = DssSdf2dGrids(len(dims) // 2, *[self.tensors[k].data_ptr() for k in SDF2D_GRID_FIELDS])

    def address(self):
        return ctypes.c_void_p(ctypes.addressof(self.struct))


def _kernels(get_lib, on_device):
    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)

    def stream(t):
        return _lib.stream_ptr(t.device) if on_device else ctypes.c_void_p(0)

    def forward(kind, pose, prm, scale, grid_id, grids, eps, cap, cand_cap):
        if on_device:
            _lib.require_device(kind, pose, prm, scale, grid_id)
        P, dev = pose.shape[1], pose.device
        out = torch.empty(P, cap, 7, dtype=torch.float64, device=dev)
        count, status = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(2))
        tag, tpar = torch.empty(P, cap, 2, dtype=torch.int32, device=dev), torch.empty(P, cap, dtype=torch.float64, device=dev)
        ncand = cand = cand_tag = None
        if cand_cap:
            ncand = torch.empty(P, dtype=torch.int32, device=dev)
            cand, cand_tag = torch.empty(P, cand_cap, 7, dtype=torch.float64, device=dev), torch.empty(P, cand_cap, 2, dtype=torch.int32, device=dev)
        rc = get_lib().dss_sdf2d_contacts_forward(
            P, cap, ptr(kind), ptr(pose), ptr(prm), ptr(scale), ptr(grid_id), grids.address() if grids is not None else None, eps,
            ptr(out), ptr(count), ptr(status), ptr(tag), ptr(tpar), cand_cap, ptr(ncand), ptr(cand), ptr(cand_tag), stream(pose))
        _lib.check(rc, "dss_sdf2d_contacts_forward")
        return out, count, status, tag, tpar, ncand, cand, cand_tag

    def backward(kind, pose, prm, scale, grid_id, grids, cap, count, tag, tpar, gout):
        P = pose.shape[1]
        g_pose, g_prm, g_scale = torch.zeros_like(pose), torch.zeros_like(prm), torch.zeros_like(scale)
        rc = get_lib().dss_sdf2d_contacts_backward(
            P, cap, ptr(kind), ptr(pose), ptr(prm), ptr(scale), ptr(grid_id), grids.address() if grids is not None else None,
            ptr(count), ptr(tag), ptr(tpar), ptr(gout), ptr(g_pose), ptr(g_prm), ptr(g_scale), stream(pose))
        _lib.check(rc, "dss_sdf2d_contacts_backward")
        return g_pose, g_prm, g_scale

    def backward_grids(kind, pose, prm, scale, grid_id, grids, cap, count, tag, tpar, gout):
        """The same and the gradient with respect to the table's vals, grads and verts (shaped like them)."""
        P = pose.shape[1]
        g_pose, g_prm, g_scale = torch.zeros_like(pose), torch.zeros_like(prm), torch.zeros_like(scale)
        # (one element at least: a table whose grids have no outline is no null argument)
        g_tab = [torch.zeros(max(grids.tensors[k].numel(), 1), dtype=torch.float64, device=pose.device) for k in ("vals", "grads", "verts")]
        rc = get_lib().dss_sdf2d_contacts_backward_grids(
            P, cap, ptr(kind), ptr(pose), ptr(prm), ptr(scale), ptr(grid_id), grids.address(), ptr(count), ptr(tag), ptr(tpar), ptr(gout),
            ptr(g_pose), ptr(g_prm), ptr(g_scale), ptr(g_tab[0]), ptr(g_tab[1]), ptr(g_tab[2]), stream(pose))
        _lib.check(rc, "dss_sdf2d_contacts_backward_grids")
        return (g_pose, g_prm, g_scale) + tuple(g[:grids.tensors[k].numel()] for g, k in zip(g_tab, ("vals", "grads", "verts")))

    return forward, backward, backward_grids


DEVICE_KERNELS = _kernels(_lib.lib, True)


def host_kernels(L):
    """The same entry points of a library that runs on host memory (the CPU emulator build of the tests), held to the
    headers like the product's."""
    _lib.bind_or_raise(L)
    return _kernels(lambda: L, False)


def check_status(status):
    """The per-pair status words of a launch -> the capacity error; nothing is raised for a clean launch."""
    st = status.cpu()
    if not bool(st.any()):
        return
    p = int(torch.nonzero(st)[0])
    s = int(st[p])
    if s & SDF2D_MALFORMED:
        raise ValueError("pair %d: unknown body kind, grid id outside the table or an edge outside its outline" % p)
    what = "more than %d contacts before thinning (DSS_SDF2D_MAXCAND)" % SDF2D_MAXCAND if s & SDF2D_OVER_CAND else \
        "more contacts than cap"
    raise RuntimeError("2-D SDF contact detection exceeded a capacity in pair %d (%s): raise the limit (the `cap` argument of "
                       "sdf_contacts2d and make_handler, the `sdf_cap` attribute of physics2d.World)" % (p, what))


class _SdfContacts2D(torch.autograd.Function):
    """vals, grads, verts: the table's three float arrays as differentiable inputs of their own (None without a table); the
    kernels read them through `grids`, whose struct points at the same memory."""

    @staticmethod
    def forward(ctx, pose, prm, scale, vals, grads, verts, kind, grid_id, grids, eps, cap, cand_cap, kernels):
        pose, prm, scale = pose.contiguous(), prm.contiguous(), scale.contiguous()
        out, count, status, tag, tpar, ncand, cand, cand_tag = kernels[0](kind, pose, prm, scale, grid_id, grids, eps, cap, cand_cap)
        ctx.status = status
        check_status(status)
        ctx.save_for_backward(pose, prm, scale, kind, grid_id, count, tag, tpar)
        ctx.grids, ctx.cap, ctx.kernels = grids, cap, kernels
        extra = (ncand, cand, cand_tag) if cand_cap else ()
        ctx.mark_non_differentiable(count, tag, tpar, *extra)
        return (out, count, tag, tpar) + extra

    @staticmethod
    def backward(ctx, gout, *_):
        pose, prm, scale, kind, grid_id, count, tag, tpar = ctx.saved_tensors
        args = (kind, pose, prm, scale, grid_id, ctx.grids, ctx.cap, count, tag, tpar, gout.contiguous())
        if ctx.grids is not None and any(ctx.needs_input_grad[3:6]):
            g = ctx.kernels[2](*args)
            tab = tuple(x if need else None for x, need in zip(g[3:], ctx.needs_input_grad[3:6]))
            return g[:3] + tab + (None,) * 7
        return ctx.kernels[1](*args) + (None,) * 10


def sdf_contacts2d(pose, prm, scale, kind, grid_id, eps, grids=None, cap=DEFAULT_CAP, candidates=0, kernels=DEVICE_KERNELS):
    """Contacts of P pairs of SDF bodies.  pose [2, P, 3] = (angle, x, y), prm [2, P, 2], scale [2, P] (float64,
    differentiable); kind, grid_id [2, P] (int32: DSS_SDF2D_<kind>, row of `grids`, a GridTable, for grid bodies).
    Returns out [P, cap, 7] = (normal, p1, p2, penetration) per contact, count [P], tag [P, cap, 2] = (direction, edge),
    tpar [P, cap]; with candidates = n also ncand [P], cand [P, n, 7], cand_tag [P, n, 2], the contacts before thinning.
    A pair with more contacts than `cap`, or more than DSS_SDF2D_MAXCAND before thinning, raises RuntimeError.
    Where the table's samples, central differences or outline vertices (`grids.tensors`) require grad, the backward pass is
    ``dss_sdf2d_contacts_backward_grids`` and their gradients flow on to whatever the table was pooled from; where none
    does, it is ``dss_sdf2d_contacts_backward`` as before."""
    tab = [grids.tensors[k] for k in ("vals", "grads", "verts")] if grids is not None else [None] * 3
    return _SdfContacts2D.apply(pose, prm, scale, *tab, kind, grid_id, grids, float(eps), int(cap), int(candidates), kernels)


def is_sdf(body):
    return hasattr(body, "query_sdfs")


def _describe(b):
    zero = b.pos.new_zeros(())
    if hasattr(b, "sdf"):
        return SDF2D_GRID, torch.stack([zero, zero])
    if hasattr(b, "dims"):
        return SDF2D_RECT, b.dims.reshape(2)
    if hasattr(b, "rad"):
        return SDF2D_CIRCLE, torch.stack([b.rad.reshape(()), zero])
    if hasattr(b, "r") and hasattr(b, "d"):
        return SDF2D_BOWL, torch.stack([b.r.reshape(()), b.d.reshape(())])
    raise TypeError("%s is not a 2-D SDF body this package knows" % type(b).__name__)


def pair_inputs(pairs, device, grids=None):
    """[(body1, body2), ...] -> the arguments of sdf_contacts2d as a dict (pose, prm, scale, kind, grid_id, grids)."""
    for pr in pairs:
        for b in pr:
            if not is_sdf(b):
                raise TypeError("a pair of an SDF body and a %s: the SDF contact handler takes SDF bodies only" % type(b).__name__)
    if grids is None:
        grids = GridTable([b for pr in pairs for b in pr if hasattr(b, "sdf")], device)
    desc = {id(b): _describe(b) for pr in pairs for b in pr}
    side = lambda f: torch.stack([torch.stack([f(pr[s]) for pr in pairs]) for s in range(2)]).to(device)      # noqa: E731
    meta = lambda f: torch.tensor([[f(pr[s]) for pr in pairs] for s in range(2)], dtype=torch.int32).to(device)      # noqa: E731
    return dict(pose=side(lambda b: torch.cat([b.rot.reshape(1), b.pos.reshape(2)])), prm=side(lambda b: desc[id(b)][1]),
                scale=side(lambda b: b.scale.reshape(())), kind=meta(lambda b: desc[id(b)][0]),
                grid_id=meta(lambda b: grids.ids.get(id(b), 0)), grids=grids if grids.ids else None)


def make_handler(kernels=DEVICE_KERNELS, device=None, cap=DEFAULT_CAP):
    """The handler class for a pair of kernel entry points (the product's are the device library's)."""

    class Handler:
        def __call__(self, args, geom1, geom2):
            if geom1 in geom2.no_contact:
                return
            world = args[0]
            b1, b2 = world.bodies[geom1.body], world.bodies[geom2.body]
            dev = b1.pos.device if device is None else torch.device(device)
            out, count, _tag, _t = sdf_contacts2d(eps=float(world.eps), cap=cap, kernels=kernels, **pair_inputs([(b1, b2)], dev))
            out = out.to(b1.pos.device)
            for q in range(int(count[0])):
                c = out[0, q]
                world.contacts.append(((c[0:2], c[2:4], c[4:6], c[6]), geom1.body, geom2.body))

    Handler.__name__ = Handler.__qualname__ = "SDFContactHandler"
    return Handler


SDFContactHandler = make_handler()
