"""Time of the report's chamfer distance at the experiments' own shapes, two ways on the same inputs in one run:
  parent   the per-scene loop over experiments.chamfer (torch.cdist blocks in fp64) on host vertex arrays, with the host -> device
           moves it makes, as fit_inertia_latent / fit_inertia_primitive ran it;
  batch    chamfer.chamfer_batch on the fitted bodies' device vertices against a target packed once (csrc/chamfer.hip), with
           the packing of the fitted side and the read-back of the [B] values.
Shapes: B = 16 scenes of level-set sphere meshes (marching cubes of the analytic SDF, radius/scale 0.55 - 0.70 against targets
0.60 - 0.75) at res 128 and at res 64, and one scene of two clouds of ~10^5 points on a sphere, which the launcher splits.
Wall clock around each call with a device synchronisation, 2 warm-up and 7 timed calls each: median (min, max).  The two are
checked against each other first.  pairs/s is set against a DERIVED peak: the inner loop issues, per pair, 3 subtractions, 1
multiply, 2 fused multiply-adds and 1 compare in fp64 and 3 selects of 32 bits, 10 VALU issue slots of 4 cycles per
wavefront of 64 lanes, so a SIMD retires 64 pairs per 40 cycles: 256 CUs x 4 SIMDs x 1.6 pairs/cycle x 2.4 GHz = 3.9e12 pairs/s.
Writes profiles/chamfer_bench.json.  DESIGN.md section 4.

    python tools/bench_chamfer.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsdfsim_amd import chamfer, experiments as X, meshsdf  # noqa: E402
from diffsdfsim_amd import world_abi as abi  # noqa: E402

dev = torch.device("cuda:0")
PEAK = 256 * 4 * (64 / 40.0) * 2.4e9      # pairs/s, derived (see above)


def spheres(B, res, lo):
    with torch.no_grad():
        return [meshsdf.primitive_mesh(abi.SHAPE_SPHERE, torch.tensor([lo + 0.01 * s, 0.0, 0.0, 0.0], dtype=torch.float64), res=res)[0].detach().to(dev) for s in range(B)]


def ball(n, rad, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    x = torch.randn(n, 3, dtype=torch.float64, device=dev, generator=g)
    return rad * x / x.norm(dim=1, keepdim=True)


def timeit(f, reps=7, warm=2):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


shapes = [("16 sphere meshes, res 128", spheres(16, 128, 0.55), spheres(16, 128, 0.60)),
          ("16 sphere meshes, res 64", spheres(16, 64, 0.55), spheres(16, 64, 0.60)),
          ("1 scene of 10^5 points", [ball(100000, 1.0, 1)], [ball(99000, 1.1, 2)])]
rows = []
for name, fit, tgt in shapes:
    fit_h, tgt_h = [v.cpu().numpy() for v in fit], [v.cpu().numpy() for v in tgt]
    target = chamfer.pack(tgt)

    def parent():
        return np.array([float(X.chamfer(torch.as_tensor(a), torch.as_tensor(b))) for a, b in zip(fit_h, tgt_h)])

    def batch():
        a, a_off = chamfer.pack(fit)
        return chamfer.chamfer_packed(a, a_off, *target).cpu().numpy()

    def searches():      # the two nearest-neighbour calls alone, for the rate
        a, a_off = chamfer.pack(fit)
        chamfer.nearest(a, a_off, *target); chamfer.nearest(*target, a, a_off)

    p, b = parent(), batch()
    pairs = 2 * sum(len(x) * len(y) for x, y in zip(fit, tgt))
    tp, tb, ts = timeit(parent), timeit(batch), timeit(searches)
    row = dict(shape=name, scenes=len(fit), points=[int(sum(len(x) for x in fit)), int(sum(len(y) for y in tgt))], pairs=pairs,
               max_abs_difference=float(np.abs(p - b).max()), value_mean=float(b.mean()),
               splits=[chamfer.splits(len(fit), max(len(x) for x in fit), max(len(y) for y in tgt)),
                       chamfer.splits(len(fit), max(len(y) for y in tgt), max(len(x) for x in fit))],
               parent_ms=dict(median=tp[0], min=tp[1], max=tp[2]), batch_ms=dict(median=tb[0], min=tb[1], max=tb[2]),
               search_ms=dict(median=ts[0], min=ts[1], max=ts[2]), speedup=tp[0] / tb[0], faster_beyond_spread=bool(tb[2] < tp[1]),
               pairs_per_s=pairs / (1e-3 * ts[0]), fraction_of_derived_peak=pairs / (1e-3 * ts[0]) / PEAK)
    rows.append(row)
    print("%-26s %8d + %8d points  parent %9.3f ms (%.3f .. %.3f)  batch %8.3f ms (%.3f .. %.3f)  x%.1f  %.3g pairs/s = %.2f of the derived peak  |diff| %.1e"
          % (name, row["points"][0], row["points"][1], *tp, *tb, row["speedup"], row["pairs_per_s"], row["fraction_of_derived_peak"], row["max_abs_difference"]))
out = os.path.join(ROOT, "profiles", "chamfer_bench.json")
with open(out, "w") as f:
    json.dump(dict(device=torch.cuda.get_device_name(0), queries_per_workgroup=chamfer.QUERIES, tile=chamfer.TILE, derived_peak_pairs_per_s=PEAK,
                   rows=rows), f, indent=1)
print("wrote", out)
