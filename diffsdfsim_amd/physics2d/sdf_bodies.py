"""The reference's 2-D SDF bodies (`sdf_physics/physics/bodies.py`: SDF, SDFGrid, SDFRect, SDFCircle, SDFBowl) as bodies of the
2-D world of this package: `get_surface()` (the outline whose edges the contact search walks) and `query_sdfs(pts)` (value
and unit gradient of the signed distance at world points) in torch, differentiable in pose, shape parameters and scale as
the reference's are.  The contact search itself runs on the device (`sdf_contacts`, csrc/sdf2d_contacts.hip); the torch code
here is the public interface of the bodies and the restatement the kernels are tested against.

Restated with the reference's semantics, quirks included:
  query     points go to the body frame; outside |p| < scale / 2 the value is the scale and the gradient zero (a grid: 1 times
            its scale, the same number); rect: the face of largest distance inside, the clamped offset outside, sign(0) = +1;
            bowl: a half ring of radius r and half thickness d, shifted by r / 2 along y; grid: bilinear interpolation of the
            samples and of their central differences (zero on the border), the latter normalised where it is not zero
  outline   rect 4 vertices, circle 64, bowl 2 x 32 (inner arc, outer arc back); grid: marching squares over the samples with
            vertices snapped to a corner whose value is below 1e-5 in magnitude, vertices made unique in lexicographic order,
            degenerate edges dropped.  In a cell with two crossings (classes 5 and 10) the reference writes both edges to one
            slot, so only the second survives; that is kept
  inertia   rect m (w^2 + h^2) / 12, circle m r^2 / 2, bowl and grid the outline sum of SDF._get_ang_inertia
  scale     rect 1.5 max(dims), circle 2.6666 rad, bowl 2.6666 (r + d), grid as given
Not restated: pygame drawing, the ODE broad-phase box (the 2-D world here takes all pairs).

A grid is differentiable in its samples too: `SDFGrid(..., sdf=<tensor that requires grad>)` keeps the graph, so `query_sdfs`,
`get_surface`, `verts`, the inertia and, through `sdf_contacts` and `World`, a rollout's loss leave `sdf.grad`.
  query     plain autograd through the interpolation of the samples and of their central differences, as in the reference
  outline derivative   the reference has none (`marching_squares` ends in `unique(dim=0)`, whose derivative torch does not
            implement); this build defines it.  The topology (which sides are crossed, the edges, which vertices are merged)
            is a constant.  A vertex's derivative is that of its interpolation along its own grid side, p0 + mu (p1 - p0)
            with mu = -v0 / (v1 - v0) of the side's two samples.  A snapped vertex (|v0|, |v1| or |v0 - v1| below 1e-5: it sits
            on a sample) has zero derivative.  Vertices merged by `unique` are one grid side seen from its two cells, the
            same two samples, so nothing is summed over duplicates.  The forward values of `unit_verts` stay the bits
            `marching_squares` produces: the derivative rides on an added f - f.detach()."""
import math

import torch

from ..world_abi import SDF2D_BOWL, SDF2D_CIRCLE, SDF2D_GRID, SDF2D_RECT
from .world import Body, Defaults, _t


def _rotation(rot):
    c, s = torch.cos(rot).reshape(()), torch.sin(rot).reshape(())
    return torch.stack([torch.stack([c, -s]), torch.stack([s, c])])


def _ring(n):
    return torch.stack([torch.arange(n), (torch.arange(n) + 1) % n], 1)


class SDF(Body):
    kind = 2              # an SDF body to the world's pair dispatch (0: circle, 1: convex polygon)
    sdf_kind = -1         # DSS_SDF2D_<kind> of include/sdf2d_contacts.h

    def __init__(self, pos, scale, vel=(0, 0, 0), mass=1, restitution=Defaults.RESTITUTION, fric_coeff=Defaults.FRIC_COEFF,
                 eps=Defaults.EPSILON, col=(255, 0, 0), thickness=1):
        self.scale = _t(scale)
        self.eps, self.col, self.thickness = eps, col, thickness
        super().__init__(pos, vel=vel, mass=mass, restitution=restitution, fric_coeff=fric_coeff, eps=eps)

    def shape_params(self):
        """The two numbers the kernel knows the shape by (rad | dims | r, d | nothing), as a differentiable tensor [2]."""
        raise NotImplementedError

    def _local_surface(self):
        raise NotImplementedError

    def _inner_query(self, loc):
        raise NotImplementedError

    def get_surface(self):
        """Outline in world coordinates: vertices [nv, 2], edges [ne, 2] (vertex numbers)."""
        verts, edges = self._local_surface()
        return verts @ _rotation(self.rot).t() + self.pos, edges

    def query_sdfs(self, pts):
        """Signed distance (world units) and its unit gradient (world frame) at the world points pts [n, 2]."""
        R = _rotation(self.rot)
        loc = (pts - self.pos) @ R
        inside = (loc.abs() < self.scale / 2).all(1)
        sdfs = self.scale.reshape(()).expand(len(pts)).clone()
        grads = loc.new_zeros(loc.shape)
        if inside.any():
            phi, g = self._inner_query(loc[inside])
            sdfs = sdfs.index_put((inside,), phi)
            grads = grads.index_put((inside,), g)
        return sdfs, grads @ R.t()

    def _ang_inertia(self):
        verts, edges = self.get_surface()
        verts = (verts - self.pos) @ _rotation(self.rot)
        v1, v2 = verts[edges[:, 0]], verts[edges[:, 1]]
        nc = (v2[:, 0] * v1[:, 1] - v2[:, 1] * v1[:, 0]).abs()
        num = (nc * ((v1 * v1).sum(1) + (v1 * v2).sum(1) + (v2 * v2).sum(1))).sum()
        return 1 / 6 * self.mass * num / nc.sum()


class SDFRect(SDF):
    sdf_kind = SDF2D_RECT

    def __init__(self, pos, dims, **kw):
        self.dims = _t(dims)
        super().__init__(pos, torch.max(self.dims) * 1.5, **kw)

    def shape_params(self):
        return self.dims

    def _local_surface(self):
        h = self.dims / 2
        corner = h.new_tensor([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]])
        return corner * h, _ring(4).to(h.device)

    def _inner_query(self, loc):
        dist = loc.abs() - self.dims / 2
        zero = dist.new_zeros(())
        sign = torch.where(loc < 0, -1.0, 1.0).to(dist)
        deepest, face = dist.max(1)
        q = torch.max(dist, zero)
        phi = q.norm(dim=1) + torch.min(deepest, zero)
        normal = torch.nn.functional.one_hot(face, 2).to(dist)
        g = torch.where((dist > 0).any(1, keepdim=True), q, normal) * sign
        return phi, g / g.norm(dim=1, keepdim=True)

    def _ang_inertia(self):
        return self.mass * (self.dims ** 2).sum() / 12


class SDFCircle(SDF):
    sdf_kind = SDF2D_CIRCLE
    NUM_VERTS = 64

    def __init__(self, pos, rad, **kw):
        self.rad = _t(rad)
        super().__init__(pos, self.rad * 2 * 1.3333, **kw)

    def shape_params(self):
        return torch.stack([self.rad.reshape(()), self.rad.new_zeros(())])

    def _local_surface(self):
        n = self.NUM_VERTS
        ang = torch.linspace(0, (2 * math.pi / n) * (n - 1), n, dtype=self.rad.dtype, device=self.rad.device)
        return torch.stack([torch.cos(ang), torch.sin(ang)], 1) * self.rad, _ring(n).to(ang.device)

    def _inner_query(self, loc):
        n = loc.norm(dim=1)
        return n - self.rad, loc / n[:, None]

    def _ang_inertia(self):
        return self.mass * self.rad * self.rad / 2


class SDFBowl(SDF):
    sdf_kind = SDF2D_BOWL
    NUM_VERTS = 64

    def __init__(self, pos, r, d, **kw):
        self.r, self.d = _t(r), _t(d)
        super().__init__(pos, (self.r + self.d) * 2 * 1.3333, **kw)

    def shape_params(self):
        return torch.stack([self.r.reshape(()), self.d.reshape(())])

    def _local_surface(self):
        n = self.NUM_VERTS // 2
        ang = torch.linspace(-math.pi, 0, n, dtype=self.r.dtype, device=self.r.device)
        arc = torch.stack([torch.cos(ang), torch.sin(ang)], 1)
        verts = torch.cat([arc * (self.r - self.d), (arc * (self.r + self.d)).flip(0)])
        shift = torch.stack([self.r.new_zeros(()), self.r.reshape(()) / 2])
        return verts + shift, _ring(2 * n).to(ang.device)

    def _inner_query(self, loc):
        r, d = self.r, self.d
        zero = loc.new_zeros(())
        p = loc - torch.stack([zero, r.reshape(()) / 2])
        ax, py = p[:, 0].abs(), p[:, 1]
        pn = torch.stack([ax, py], 1).norm(dim=1)
        a = ((torch.where(py < 0, pn, ax)) - r).abs() - d
        ps = torch.stack([a, py], 1)
        m = torch.max(ps, zero)
        phi = m.norm(dim=1) + torch.min(zero, ps.max(1)[0])
        below = p * torch.sign(pn - r).detach()[:, None]
        flip = (torch.sign(p[:, 0]) * torch.sign(p[:, 0].abs() - r)).detach()
        above = m * torch.stack([flip, torch.ones_like(flip)], 1)
        g = torch.where((py >= 0)[:, None], above, below)
        return phi, g / g.norm(dim=1, keepdim=True)


def _bilinear(vol, ind):
    """vol [n0, n1] or [n0, n1, 2] at the index positions ind [n, 2]; corners and weights from the clamped cell."""
    n0, n1 = vol.shape[0], vol.shape[1]
    x0, y0 = torch.floor(ind[:, 0]).long(), torch.floor(ind[:, 1]).long()
    x1, y1 = (x0 + 1).clamp(0, n0 - 1), (y0 + 1).clamp(0, n1 - 1)
    x0, y0 = x0.clamp(0, n0 - 1), y0.clamp(0, n1 - 1)
    ux, vx = x1.to(ind) - ind[:, 0], ind[:, 0] - x0.to(ind)
    uy, vy = y1.to(ind) - ind[:, 1], ind[:, 1] - y0.to(ind)
    w = [ux * uy, ux * vy, vx * uy, vx * vy]
    c = [vol[x0, y0], vol[x0, y1], vol[x1, y0], vol[x1, y1]]
    if vol.dim() > 2:
        w = [x[:, None] for x in w]
    return c[0] * w[0] + c[1] * w[1] + c[2] * w[2] + c[3] * w[3]


def central_differences(sdf):
    """[n0, n1, 2]: (s[i + 1, j] - s[i - 1, j]) / 2 and (s[i, j + 1] - s[i, j - 1]) / 2, zero on the border they cross."""
    g = sdf.new_zeros(sdf.shape + (2,))
    g[1:-1, :, 0] = (sdf[2:, :] - sdf[:-2, :]) / 2
    g[:, 1:-1, 1] = (sdf[:, 2:] - sdf[:, :-2]) / 2
    return g


def marching_squares(sdf, sides=False):
    """Outline of the zero level set of the samples sdf [n0, n1] over [-0.5, 0.5]^2 (host, float64): vertices [nv, 2] unique
    and in lexicographic order, edges [ne, 2] in cell order.  Side k of a cell runs from corner k to corner k + 1 of (top
    left, top right, bottom right, bottom left); a cell's edge joins its crossed sides in ascending order.
    sides=True: also, per unique vertex, the flat numbers [nv, 2] of the two samples at the ends of its grid side and whether it
    was snapped [nv] (one of the two values, or their difference, below 1e-5 in magnitude: the vertex sits on a sample)."""
    s, with_sides = sdf.detach().to("cpu", torch.float64), sides
    n0, n1 = s.shape
    gx = torch.linspace(-0.5, 0.5, n0, dtype=torch.float64)
    gy = torch.linspace(-0.5, 0.5, n1, dtype=torch.float64)
    pos = torch.stack(torch.meshgrid(gx, gy, indexing="ij"), 2)
    win = [(slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None)), (slice(1, None), slice(1, None)), (slice(1, None), slice(0, -1))]
    P = [pos[a, b].reshape(-1, 2) for a, b in win]
    V = [s[a, b].reshape(-1) for a, b in win]
    inside = [v < 0 for v in V]
    ncell = len(V[0])
    cls = 8 * inside[0].long() + 4 * inside[1].long() + 2 * inside[2].long() + inside[3].long()
    crossed = torch.stack([inside[k] != inside[(k + 1) % 4] for k in range(4)], 1)          # [ncell, 4]
    slot = torch.cumsum(crossed.long().reshape(-1), 0).reshape(ncell, 4) - crossed.long()     # vertex number of (cell, side)
    verts = torch.zeros(int(crossed.sum()), 2, dtype=torch.float64)
    number = torch.arange(n0 * n1).reshape(n0, n1)
    I = [number[a, b].reshape(-1) for a, b in win]
    ends, snapped = torch.zeros(len(verts), 2, dtype=torch.long), torch.zeros(len(verts), dtype=torch.bool)
    for k in range(4):
        p0, p1, v0, v1 = P[k], P[(k + 1) % 4], V[k], V[(k + 1) % 4]
        near0, near1, flat = v0.abs() < 1e-5, v1.abs() < 1e-5, (v0 - v1).abs() < 1e-5
        mu = -v0 / (v1 - v0)
        at = torch.where((near0 | flat)[:, None], p0, torch.zeros_like(p0))
        at = torch.where(near1[:, None], p1, at)
        at = torch.where((~near0 & ~near1 & ~flat)[:, None], p0 + mu[:, None] * (p1 - p0), at)
        verts[slot[crossed[:, k], k]] = at[crossed[:, k]]
        ends[slot[crossed[:, k], k]] = torch.stack([I[k], I[(k + 1) % 4]], 1)[crossed[:, k]]
        snapped[slot[crossed[:, k], k]] = (near0 | near1 | flat)[crossed[:, k]]
    edges = []
    for c in torch.nonzero(crossed.any(1)).reshape(-1).tolist():
        sides = torch.nonzero(crossed[c]).reshape(-1).tolist()
        if len(sides) == 4:       # two crossings: the reference keeps the second edge only and leaves a degenerate one behind
            sides = [1, 2] if int(cls[c]) == 5 else [2, 3]
        edges.append([int(slot[c, sides[0]]), int(slot[c, sides[1]])])
    edges = torch.tensor(edges, dtype=torch.long).reshape(-1, 2)
    verts, inverse = verts.unique(dim=0, return_inverse=True)
    edges = inverse[edges]
    edges = edges[edges[:, 0] != edges[:, 1]]
    if not with_sides:
        return verts, edges
    # vertices that `unique` merged lie on one grid side seen from its two cells (the same two samples), or were snapped to
    # one sample: any of the merged records serves, and a vertex is snapped if one of them is
    uends = torch.zeros(len(verts), 2, dtype=torch.long)
    uends[inverse] = ends
    usnap = torch.zeros(len(verts), dtype=torch.long).index_add_(0, inverse, snapped.long()) > 0
    return verts, edges, uends, usnap


class SDFGrid(SDF):
    sdf_kind = SDF2D_GRID

    def __init__(self, pos, scale, sdf, **kw):
        self.sdf = _t(sdf)
        self.sdf_grads = central_differences(self.sdf)
        self.unit_verts, self.edges, self.vert_samples, self.vert_snapped = (x.to(self.sdf.device) for x in marching_squares(self.sdf, sides=True))
        if self.sdf.requires_grad:
            self.unit_verts = self.unit_verts + self._outline_tangent()
        self.scale = _t(scale)
        self.verts = self.unit_verts * self.scale
        super().__init__(pos, scale, **kw)

    def _outline_tangent(self):
        """Zeros [nv, 2] that carry the outline's derivative with respect to the samples (module docstring, "outline
        derivative"): f - f.detach() with f the interpolation of every vertex that was not snapped along its own grid side."""
        n0, n1 = self.sdf.shape
        free = ~self.vert_snapped
        i0, i1 = self.vert_samples[free, 0], self.vert_samples[free, 1]
        flat = self.sdf.reshape(-1).to(torch.float64)
        gx = torch.linspace(-0.5, 0.5, n0, dtype=torch.float64, device=flat.device)
        gy = torch.linspace(-0.5, 0.5, n1, dtype=torch.float64, device=flat.device)
        at = lambda i: torch.stack([gx[i // n1], gy[i % n1]], 1)      # noqa: E731
        p0, p1, v0, v1 = at(i0), at(i1), flat[i0], flat[i1]
        f = p0 + (-v0 / (v1 - v0))[:, None] * (p1 - p0)
        return self.unit_verts.new_zeros(self.unit_verts.shape).index_put((free,), (f - f.detach()).to(self.unit_verts.dtype))

    def shape_params(self):
        return self.sdf.new_zeros(2)

    def _local_surface(self):
        return self.unit_verts * self.scale, self.edges

    def _inner_query(self, loc):
        n = loc.new_tensor([self.sdf.shape[0] - 1, self.sdf.shape[1] - 1])
        ind = (loc / self.scale + 0.5) * n
        g = _bilinear(self.sdf_grads, ind)
        norm = g.norm(dim=1, keepdim=True)
        g = torch.where(norm != 0, g / torch.where(norm != 0, norm, torch.ones_like(norm)), g)
        return _bilinear(self.sdf, ind) * self.scale, g
