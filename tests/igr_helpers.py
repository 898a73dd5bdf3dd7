"""Build BatchEngine specs / worlds of the neural-SDF goldens (tests/golden/rollout_igr_*.npz, oracle/gen/gen_igr_golden.py)."""
import ctypes

import numpy as np

import rollout_helpers as R


def seeded_weights(g):
    """The network the golden was recorded with: numpy-seeded geometric initialisation (oracle/igr_oracle.py)."""
    from oracle import igr_oracle
    return igr_oracle.geometric_init(int(g["igr_seed"]), float(g["igr_radius"]))


def spec_from_golden(g, copies=1, packed=None):
    from diffsdfsim_amd import igr, meshes, meshsdf
    if packed is None:
        packed = igr.pack_weights(*seeded_weights(g))
    nb = len(g["mass"])
    kind = g["kind"]
    ms = []
    for i in range(nb):
        prm = g["shape_prm"][i]
        if "verts_%d" % i in g:          # the neural body's level-set mesh as the reference built it
            ms.append((g["verts_%d" % i], g["faces_%d" % i]))
        elif g["custom_mesh"][i]:
            v, f, _tie = meshes.box_mesh(prm)
            ms.append((v, f))
        else:                            # level-set mesh of a primitive, rebuilt with the device mesher (same case tables)
            scale = max(prm[0], prm[1] / 2) * 1.5 if kind[i] == 2 else prm.max() * 1.5 / 2
            v, f = meshsdf.primitive_mesh(int(kind[i]), np.concatenate([prm, [0.0]]) / scale, res=128)
            assert (len(v), len(f)) == tuple(g["meshsize_%d" % i]), "device marching cubes and the golden's mesh differ in size"
            ms.append(((v * scale).cpu().numpy(), f.cpu().numpy()))
    rep = lambda a: np.repeat(np.asarray(a)[None], copies, axis=0)
    Je = np.zeros((6 * len(g["fixed"]), 6 * nb))
    for k, b in enumerate(g["fixed"]):
        Je[6 * k:6 * k + 6, 6 * b:6 * b + 6] = np.eye(6)
    aux = np.where(kind == 6, float(g["igr_scale"]), 0.0)
    return dict(pose=rep(g["pose0"]), vel=rep(g["vel0"]), mass=rep(g["mass"]), inertia=rep(g["inertia"]),
                restitution=rep(g["restitution"]), fric=rep(g["fric"]), fext=rep(g["fext"]), shape_type=rep(kind.astype(np.int32)),
                shape_prm=rep(g["shape_prm"]), shape_aux=rep(aux), mesh_id=rep(np.arange(nb)), meshes=ms, Je=rep(Je),
                no_contact=np.asarray(g["no_contact"], np.uint8), igr_net=packed)


def engine_kwargs(g, **over):
    kw = dict(dt=float(g["dt"]), eps=float(g["eps"]), tol=float(g["tol"]), fric_dirs=int(g["fric_dirs"]), toc_diff=True,
              strict_no_pen=bool(g["strict_no_pen"]), maxc=64, max_cand=4096, max_pc=64)
    kw.update(over)
    return kw


def torch_network(g):
    """An ImplicitNet-shaped torch module (layers lin0..lin8, as the IGR repository's class the reference loads) holding the
    golden's seeded weights: what a caller hands to decode_igr."""
    import torch
    Ws, bs = seeded_weights(g)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for l, (W, b) in enumerate(zip(Ws, bs)):
                lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
                with torch.no_grad():
                    lin.weight.copy_(torch.tensor(W)); lin.bias.copy_(torch.tensor(b))
                setattr(self, "lin%d" % l, lin)
    return Net()


# ---- dss_igr_query_list with every argument spelled out (the list forms of narrowphase_igr.hip and step_bwd_all.hip) ----
# `backend` is diffsdfsim_amd.engine.TorchBackend (device library, torch tensors) or emu.EmuBackend (emulator library, numpy
# arrays): both have lib, from_numpy, to_numpy, ptr and stream.

SENTINEL = -7.25      # what the outputs hold before a call that must leave part of them alone


def packed_on(backend, Ws, bs):
    """pack_weights' operand set as arrays of `backend`."""
    from diffsdfsim_amd import igr
    return {k: backend.from_numpy(v.numpy()) for k, v in igr.pack_weights(Ws, bs, device="cpu").items()}


def net_struct(backend, P, width=None, latent=None):
    """DssIgrNet of packed_on's arrays; width / latent override what W0's shape says (0, 0 = the header's default network)."""
    from diffsdfsim_amd import world_abi
    w, l = int(P["W0"].shape[0]), int(P["W0"].shape[1]) - 3
    return world_abi.DssIgrNet(*[backend.ptr(P[k]) for k in world_abi.IGR_NET_POINTERS], w if width is None else width,
                               l if latent is None else latent)


def grad_columns(latent, mode):
    from diffsdfsim_amd import igr
    return 4 if (mode == igr.MODE_LATENT and latent > 3) else 3


def call_query_list(backend, net, pts, lat_idx, codes, lat_stride, n_dev, n_cap, mode, sdf, grad):
    """The bare call: `net` a DssIgrNet or None, every array one of `backend`'s or None (NULL).  -> the return code."""
    a = lambda x: None if x is None else backend.ptr(x)
    return backend.lib.dss_igr_query_list(None if net is None else ctypes.byref(net), a(pts), a(lat_idx), a(codes), int(lat_stride),
                                          a(n_dev), int(n_cap), int(mode), a(sdf), a(grad), backend.stream())


def query_list(backend, P, pts, codes, mode, lat_idx=None, n_dev=None, fill=np.nan):
    """pts [n_cap][3], codes [ncodes][stride] (a point reads the first L entries of row lat_idx[i], or of row 0 when lat_idx
    is None), n_dev: the list's length in device memory, or None = n_cap.  Host arrays in; the outputs are pre-filled with
    `fill` and come back as `backend`'s arrays: sdf [n_cap], grad [n_cap][3 or 4] (None in MODE_VALUE)."""
    from diffsdfsim_amd import igr
    pts = np.ascontiguousarray(pts, np.float64); codes = np.ascontiguousarray(codes, np.float64)
    assert pts.ndim == 2 and pts.shape[1] == 3 and codes.ndim == 2
    n_cap, latent = len(pts), int(P["W0"].shape[1]) - 3
    if lat_idx is not None:
        lat_idx = np.ascontiguousarray(lat_idx, np.int32)
        assert lat_idx.shape == (n_cap,) and lat_idx.min() >= 0 and lat_idx.max() < len(codes)      # (poison by value, never by index)
    assert n_dev is None or 0 <= n_dev <= n_cap
    up = lambda x: None if x is None else backend.from_numpy(x)
    sdf = backend.from_numpy(np.full(n_cap, fill))
    grad = None if mode == igr.MODE_VALUE else backend.from_numpy(np.full((n_cap, grad_columns(latent, mode)), fill))
    rc = call_query_list(backend, net_struct(backend, P), up(pts), up(lat_idx), up(codes), codes.shape[1],
                         None if n_dev is None else up(np.array([n_dev], np.int32)), n_cap, mode, sdf, grad)
    assert rc == 0, rc
    return sdf, grad


def reference(Ws, bs, pts, codes, lat_idx=None, dtype=np.float64):
    """tests/implicit_net.py on the rows [latent_i, xyz_i]: value [n], d / d latent [n][L], d / d xyz [n][3] in `dtype`."""
    import implicit_net as IN
    latent = np.shape(Ws[0])[1] - 3
    idx = np.zeros(len(pts), int) if lat_idx is None else np.asarray(lat_idx)
    inp = np.concatenate([np.asarray(codes)[idx, :latent], np.asarray(pts)], 1)
    v, J = IN.forward(inp, Ws, bs, dtype=dtype)
    return v, J[:, :latent], J[:, latent:]


def expected_grad(ref, latent, mode):
    """The gradient array a mode returns, from reference()'s triple: d / d xyz, or d / d latent (two columns and a zero for L = 2)."""
    from diffsdfsim_amd import igr
    if mode == igr.MODE_XYZ:
        return ref[2]
    g = ref[1]
    return g if latent > 3 else np.concatenate([g, np.zeros((len(g), 3 - latent), g.dtype)], 1)


def poisoned_codes(rng, ncodes, latent, stride, dead_row):
    """A code table [ncodes][stride] whose columns latent.. and whose row `dead_row` are NaN: a read past L, or of a row no live
    point names, shows in the value.  Every index stays in range."""
    codes = np.full((ncodes, stride), np.nan)
    codes[:, :latent] = rng.normal(0, 0.1, (ncodes, latent))
    codes[dead_row] = np.nan
    return codes
