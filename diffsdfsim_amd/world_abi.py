"""The C ABI of include/*.h as ctypes sees it: constants, function prototypes, struct mirrors, array shapes.

The headers are the documentation and the check, the tables below are the binding: ``bind()`` gives every function of a
loaded library its ``argtypes`` / ``restype``, so callers pass plain Python ints, floats and pointers.  The field order of
``FIELDS`` IS the struct layout; ``dss_world_sizeof()`` is checked against it when the world is first bound to the library.
tests/test_abi.py checks constants, prototypes and field names and their order against the headers' text.
"""
import ctypes

import numpy as np

# the header's #defines (DSS_<name>)
ABI_VERSION = 4
CAND_FIELDS = 28
CSCR_ROWS = 56
N_ACTIVE_OVERFLOW = 1 << 30
SHAPE_BOX, SHAPE_SPHERE, SHAPE_CYLINDER, SHAPE_BOX_ROUNDED, SHAPE_BRICK, SHAPE_BOWL, SHAPE_IGR, SHAPE_GRID = 0, 1, 2, 3, 4, 5, 6, 7
IGR_HDR, IGR_ROUNDS = 16, 42
IGR_LATENT_MAX = 4

_I, _D, _P = ctypes.c_int, ctypes.c_double, ctypes.c_void_p

# name: (return kind, argument kinds): 'p' any pointer (tensor, struct by reference, stream; None = NULL), 'i' int, 'd' double,
# 'z' size_t, 'v' void.  In the headers' order, one section per line or two.
PROTOTYPES = {
    # diffsdfsim_hip.h
    "dss_abi_version": ("i", ""),
    "dss_lcp_dense_workspace_bytes": ("z", "iiii"), "dss_lcp_dense_forward": ("i", "pppppppiiiidiiipppppppzp"),
    "dss_lcp_dense_backward": ("i", "ppppiiiipppppppppppppzp"),
    "dss_lcp_contact_workspace_bytes": ("z", "iiiii"), "dss_lcp_contact_forward": ("i", "ppppppppiiiiidiipppppppzp"),
    "dss_lcp_contact_backward": ("i", "ppppppiiiiippppppppppp"),
    "dss_world_sizeof": ("z", ""), "dss_np_slots": ("i", "ii"), "dss_step_begin": ("i", "pp"), "dss_step_attempt": ("i", "ppzp"),
    "dss_solve_dynamics": ("i", "ppzp"), "dss_find_contacts": ("i", "pp"),
    "dss_adjoint_sizeof": ("z", ""), "dss_step_backward": ("i", "ppp"),
    "dss_igr_packed_doubles": ("z", ""), "dss_igr_query_list": ("i", "ppppipiippp"), "dss_igr_query": ("i", "ppppppppippp"),
    "dss_igr_query_latent_grad": ("i", "ppppppppippp"),
    "dss_sdf_query": ("i", "ippipppp"), "dss_mesh_inertia": ("i", "pppppipppp"), "dss_grid_sdf_query": ("i", "piiidpipppp"),
    "dss_mesh_inertia_backward": ("i", "ppiidppp"), "dss_selftest_div3": ("i", "ppipp"), "dss_selftest_sqrt": ("i", "pipp"),
    "dss_mc_workspace_bytes": ("z", "iii"), "dss_mc_count": ("i", "piiidppzpp"), "dss_mc_emit": ("i", "piiidppipppp"),
    "dss_meshsdf_backward": ("i", "ipppipp"),
    "dss_contacts2d_forward": ("i", "iippppppdpppp"), "dss_contacts2d_backward": ("i", "iippppppdppppp"),
    # pointcloud_loss.h
    "dss_pointcloud_loss_workspace_bytes": ("z", "ii"), "dss_pointcloud_loss": ("i", "iipppppppzp"),
    "dss_pointcloud_loss_grids": ("i", "iippppppipppppzp"), "dss_pointcloud_loss_grids_adjoint": ("i", "iippppppipppppp"),
    # pointcloud_loss_igr.h
    "dss_pointcloud_loss_igr_workspace_bytes": ("z", "iii"), "dss_pointcloud_loss_igr": ("i", "piippppppiippzp"),
    # depth_camera.h
    "dss_depth_render": ("i", "iippppddddiiddppp"), "dss_grid_block_min": ("i", "ippppipp"),
    "dss_depth_render_grids": ("i", "iippppddddiiddpipppppppp"), "dss_depth_points_count": ("i", "iiiipppp"),
    "dss_depth_points_emit": ("i", "iiiippppddddpp"),
    # shade_camera.h
    "dss_shade_render": ("i", "iippppddddiidpippppppppipdpidppppp"),
    # cloud_select.h
    "dss_cloud_select_count": ("i", "iiiipppp"), "dss_cloud_select_emit": ("i", "iiiippppp"),
    "dss_cloud_stats_workspace_bytes": ("z", "ii"), "dss_cloud_stats": ("i", "iippppzp"),
    # chamfer.h
    "dss_chamfer_nn_workspace_bytes": ("z", "iii"), "dss_chamfer_nn": ("i", "iiipppppppzp"), "dss_chamfer_segment_mean": ("i", "ipppp"),
    # sdf2d_contacts.h
    "dss_sdf2d_contacts_forward": ("i", "iippppppdpppppipppp"), "dss_sdf2d_contacts_backward": ("i", "iipppppppppppppp"),
    "dss_sdf2d_contacts_backward_grids": ("i", "iippppppppppppppppp"),
}
# outside the headers, bound where a library exports them: the diagnostic build (csrc/diag_stamps.h, csrc/diag_latency.hip)
# and the CPU emulator's test hooks (tests/emu/lcp_dense_wave.cpp); the mesh voxeliser, whose header lies beside its kernel
# (csrc/mesh_grid.h), the depth camera's adjoint (csrc/depth_adjoint.h) and the chain from a neural body's value grid to its
# latent code (csrc/igr_grid_adjoint.h)
OPTIONAL_PROTOTYPES = {
    "dss_mesh_grid_sdf": ("i", "ipppppppiippp"),
    "dss_depth_adjoint_workspace_bytes": ("z", "iiii"), "dss_depth_adjoint": ("i", "iippppddddiipppdpippppppppzp"),
    "dss_igr_grid_adjoint_workspace_bytes": ("z", "iii"), "dss_igr_grid_adjoint": ("i", "pippppiipipppzp"),
    "dss_diag_set_lcp_stamps": ("v", "pp"), "dss_diag_set_np_stamps": ("v", "pp"), "dss_diag_latency": ("v", "iiippppp"),
    "dss_emu_lcp_dense_wave_forward": PROTOTYPES["dss_lcp_dense_forward"], "dss_emu_lcp_dense_group_fits": ("i", "iii"),
}
_CTYPE = {"p": _P, "i": _I, "d": _D, "z": ctypes.c_size_t, "v": None}


def bind(L):
    """Set argtypes / restype of every function of the tables on the loaded library L; returns L.  A function of the
    header that L does not export raises AttributeError, an optional one is skipped."""
    for name, (ret, args) in {**PROTOTYPES, **{n: p for n, p in OPTIONAL_PROTOTYPES.items() if hasattr(L, n)}}.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[k] for k in args]
    return L


IGR_NET_POINTERS = ("W0", "b0", "Wp", "bh", "W8", "b8")
IGR_NET_FIELDS = IGR_NET_POINTERS + ("width", "latent")      # hidden width and latent size: 0, 0 = the 128 / 2 network


class DssIgrNet(ctypes.Structure):
    _fields_ = [(k, _P if k in IGR_NET_POINTERS else _I) for k in IGR_NET_FIELDS]


SDF2D_CIRCLE, SDF2D_RECT, SDF2D_BOWL, SDF2D_GRID = 0, 1, 2, 3      # DSS_SDF2D_<kind> (sdf2d_contacts.h)
SDF2D_MAXCAND = 256
SDF2D_OVER_CAP, SDF2D_OVER_CAND, SDF2D_MALFORMED = 1, 2, 4
SDF2D_GRID_FIELDS = ("dims", "val_off", "vert_off", "edge_off", "edges", "vals", "grads", "verts")


class DssSdf2dGrids(ctypes.Structure):
    _fields_ = [("ngrids", _I)] + [(k, _P) for k in SDF2D_GRID_FIELDS]


# (name, kind) kind: 'i' int scalar, 'd' double scalar, 'pd' double*, 'pi' int*, 'pb' uint8*
FIELDS = [
    ("B", "i"), ("nb", "i"), ("neq", "i"), ("maxc", "i"), ("fric_dirs", "i"), ("max_cand", "i"), ("max_pc", "i"),
    ("nmesh", "i"), ("strict_no_pen", "i"), ("toc_diff", "i"), ("lcp_max_iter", "i"), ("shape_rare", "i"), ("grad_flags", "i"),
    ("shape_box", "i"),
    ("eps", "d"), ("tol", "d"), ("dt", "d"),
    ("pose", "pd"), ("vel", "pd"),
    ("mass", "pd"), ("inertia", "pd"), ("restitution", "pd"), ("fric", "pd"), ("fext", "pd"),
    ("shape_type", "pi"), ("shape_prm", "pd"), ("shape_aux", "pd"), ("mesh_id", "pi"), ("no_contact", "pb"),
    ("grid_id", "pi"), ("grid_off", "pi"), ("grid_dims", "pi"), ("grid_data", "pd"),
    ("mesh_voff", "pi"), ("mesh_nv", "pi"), ("mesh_foff", "pi"), ("mesh_nf", "pi"),
    ("verts", "pd"), ("faces", "pi"), ("fcent", "pd"), ("frad", "pd"), ("vgrad", "pd"),
    ("fch_box", "pd"), ("vch_box", "pd"), ("mesh_fch_off", "pi"), ("mesh_vch_off", "pi"),
    ("Je", "pd"), ("b_eq", "pd"),
    ("t", "pd"), ("t_end", "pd"), ("dt_try", "pd"), ("last_dt", "pd"), ("dt_use", "pd"),
    ("active", "pi"), ("step_mask", "pi"), ("had_contacts", "pi"), ("steps_left", "pi"), ("toc", "pi"), ("nsub", "pi"), ("n_active", "pi"),
    ("nc", "pi"), ("c_body", "pi"), ("c_face", "pi"), ("c_abc", "pd"), ("c_geom", "pd"),
    ("n_nc", "pi"), ("n_body", "pi"), ("n_face", "pi"), ("n_abc", "pd"), ("n_geom", "pd"),
    ("pose0", "pd"), ("vel0", "pd"),
    ("Mblk", "pd"), ("pvec", "pd"), ("cop", "pd"), ("x", "pd"), ("lam", "pd"), ("slack", "pd"), ("nu", "pd"),
    ("cop_body", "pi"), ("lcp_iters", "pi"), ("lcp_status", "pi"),
    ("ovl", "pi"), ("pair_list", "pi"), ("n_pairs", "pi"), ("invalid", "pi"), ("overflow", "pi"),
    ("pc_count", "pi"), ("pc_stats", "pi"), ("pc_face", "pi"), ("pc_abc", "pd"), ("pc_geom", "pd"),
    ("cand_face", "pi"), ("cand_state", "pi"), ("cand_buf", "pd"),
    ("max_sub", "i"),
    ("tp_pose", "pd"), ("tp_vel", "pd"), ("tp_dt", "pd"), ("tp_x", "pd"), ("tp_lam", "pd"), ("tp_slack", "pd"),
    ("tp_nu", "pd"), ("tp_abc", "pd"), ("tp_geom", "pd"),
    ("tp_nc", "pi"), ("tp_body", "pi"), ("tp_face", "pi"), ("tp_flags", "pi"), ("tp_t", "pd"),
    ("ev_lcp_start", "ev"), ("ev_lcp_stop", "ev"), ("ev_np_start", "ev"), ("ev_np_stop", "ev"),
    # neural SDF bodies: DssIgrNet (six pointers, width, latent size), capacities, the round-based narrow phase's item state and
    # query lists
    *[("igr_" + k, "pd" if k in IGR_NET_POINTERS else "i") for k in IGR_NET_FIELDS],
    ("igr_items_cap", "i"), ("igr_qcap", "i"), ("igr_rounds", "i"),
    ("igr_list", "pi"), ("igr_hdr", "pi"), ("igr_cface", "pi"), ("igr_cstate", "pi"), ("igr_cbuf", "pd"),
    ("igr_qpts", "pd"), ("igr_qlat", "pi"), ("igr_qtag", "pi"), ("igr_qsdf", "pd"), ("igr_qgrad", "pd"), ("igr_qn", "pi"),
    ("igr_hint", "ev"), ("igr_ev", "ev"),
    ("igr_latent", "pd"),
]


def _world_fields():
    """ctypes fields of DssWorld: FIELDS in order, with the members of `DssIgrNet igr` (listed there as igr_<member>, as the
    header's text reads) as ONE nested struct `igr`: W.igr.latent is the network's latent size, W.igr_latent the latent table."""
    i0 = FIELDS.index(("igr_" + IGR_NET_FIELDS[0], "pd"))
    flat = [(n, {"i": _I, "d": _D}.get(k, _P)) for n, k in FIELDS]
    return flat[:i0] + [("igr", DssIgrNet)] + flat[i0 + len(IGR_NET_FIELDS):]


class DssWorld(ctypes.Structure):
    _fields_ = _world_fields()


NP_DTYPE = {"pd": np.float64, "pi": np.int32, "pb": np.uint8}


def igr_shapes(items_cap, qcap, max_cand, B=None, nb=None, maxc=None):
    """Arrays of the round-based narrow phase for neural SDF bodies (narrowphase_igr.hip); with B, nb and maxc also the
    latent table and what the reverse sweep adds for such bodies (step_bwd.hip): igr_bw_grad holds d phi / d xyz [cap][3]
    followed by d phi / d latent in rows of three (the two-number code) or of IGR_LATENT_MAX (the four-number code), so it
    is sized for the wider of the two."""
    extra = {}
    if B is not None:
        cap = B * 2 * maxc
        extra = {"igr_latent": (B, nb, IGR_LATENT_MAX), "g_latent": (B, nb, IGR_LATENT_MAX), "igr_bw_n": (1,), "igr_bw_idx": (B, 2, maxc),
                 "igr_bw_pts": (cap, 3), "igr_bw_lat": (cap,), "igr_bw_sdf": (2, cap), "igr_bw_grad": (cap * (3 + IGR_LATENT_MAX),)}
    return {
        **extra,
        "igr_list": (items_cap,), "igr_hdr": (items_cap, IGR_HDR), "igr_cface": (items_cap, 3, max_cand),
        "igr_cstate": (items_cap, max_cand), "igr_cbuf": (items_cap, CAND_FIELDS, max_cand),
        "igr_qpts": (4, qcap, 3), "igr_qlat": (4, qcap), "igr_qtag": (4, qcap), "igr_qsdf": (4, qcap), "igr_qgrad": (2, qcap, 3),
        "igr_qn": (2 * (IGR_ROUNDS + 2),),
    }


def array_shapes(B, nb, neq, maxc, fd, max_cand, max_pc, max_sub, nmesh, NV, NF, np_slots, NFC=1, NVC=1):
    """Shapes of every array the kernels touch (state, scratch, tape); np_slots = dss_np_slots(B, nb)."""
    npair = nb * (nb - 1)
    NR = fd + 2
    NFc = 3 * (1 + fd // 2) + 8
    nz = 6 * nb
    s = {
        "pose": (B, nb, 7), "vel": (B, nb, 6), "mass": (B, nb), "inertia": (B, nb, 9), "restitution": (B, nb),
        "fric": (B, nb), "fext": (B, nb, 6), "shape_type": (B, nb), "shape_prm": (B, nb, 3), "shape_aux": (B, nb), "mesh_id": (B, nb),
        "no_contact": (nb, nb), "mesh_voff": (nmesh,), "mesh_nv": (nmesh,), "mesh_foff": (nmesh,), "mesh_nf": (nmesh,),
        "verts": (NV, 3), "faces": (NF, 3), "fcent": (NF, 3), "frad": (NF,), "vgrad": (NV, 3),
        "fch_box": (NFC, 6), "vch_box": (NVC, 6), "mesh_fch_off": (nmesh,), "mesh_vch_off": (nmesh,),
        "Je": (B, max(neq, 1), nz), "b_eq": (B, max(neq, 1)),
        "t": (B,), "t_end": (B,), "dt_try": (B,), "last_dt": (B,), "dt_use": (B,),
        "active": (B,), "had_contacts": (B,), "toc": (B,), "nsub": (B,), "n_active": (1,),
        "nc": (B,), "c_body": (B, 2, maxc), "c_face": (B, maxc), "c_abc": (B, 3, maxc), "c_geom": (B, 10, maxc),
        "n_nc": (B,), "n_body": (B, 2, maxc), "n_face": (B, maxc), "n_abc": (B, 3, maxc), "n_geom": (B, 10, maxc),
        "pose0": (B, nb, 7), "vel0": (B, nb, 6),
        "Mblk": (B, nb, 6, 6), "pvec": (B, nz), "cop": (B, NFc, maxc), "x": (B, nz), "lam": (B, NR, maxc),
        "slack": (B, NR, maxc), "nu": (B, max(neq, 1)), "cop_body": (B, 2, maxc), "lcp_iters": (B,), "lcp_status": (B,),
        "ovl": (B, nb, nb), "pair_list": (3 * B * npair,), "n_pairs": (8,), "invalid": (B,), "overflow": (B,),
        "pc_count": (B, npair), "pc_stats": (B, npair, 2), "pc_face": (B, npair, max_pc), "pc_abc": (B, npair, 3, max_pc),
        "pc_geom": (B, npair, 10, max_pc),
        "cand_face": (np_slots, 2, max_cand), "cand_state": (np_slots, max_cand), "cand_buf": (np_slots, CAND_FIELDS, max_cand),
    }
    if max_sub > 0:
        s.update({
            "tp_pose": (max_sub, B, nb, 7), "tp_vel": (max_sub, B, nb, 6), "tp_dt": (max_sub, B), "tp_x": (max_sub, B, nz),
            "tp_lam": (max_sub, B, NR, maxc), "tp_slack": (max_sub, B, NR, maxc), "tp_nu": (max_sub, B, max(neq, 1)),
            "tp_abc": (max_sub, B, 3, maxc), "tp_geom": (max_sub, B, 10, maxc),
            "tp_nc": (max_sub, B), "tp_body": (max_sub, B, 2, maxc), "tp_face": (max_sub, B, maxc), "tp_flags": (max_sub, B), "tp_t": (max_sub, B),
        })
    return s


ADJ_FIELDS = [
    ("a_pose", "pd"), ("a_vel", "pd"), ("a_geom", "pd"), ("a_last_dt", "pd"), ("a_dt", "pd"),
    ("g_mass", "pd"), ("g_inertia", "pd"), ("g_rest", "pd"), ("g_fric", "pd"), ("g_fext", "pd"), ("g_prm", "pd"), ("g_verts", "pd"),
    ("cur_slot", "pi"), ("lo_slot", "pi"), ("bw_active", "pi"),
    ("a_x", "pd"), ("dMblk", "pd"), ("dpvec", "pd"), ("dcop", "pd"), ("cscr", "pd"), ("bw_nc", "pi"),
    ("igr_bw_n", "pi"), ("igr_bw_idx", "pi"), ("igr_bw_pts", "pd"), ("igr_bw_lat", "pi"), ("igr_bw_sdf", "pd"), ("igr_bw_grad", "pd"),
    ("g_latent", "pd"),
]


class DssAdjoint(ctypes.Structure):
    _fields_ = [(n, _P) for n, k in ADJ_FIELDS]


def adjoint_shapes(B, nb, maxc, fd, NV=1, igr=False, latent_table=False):
    """Arrays of DssAdjoint; igr: the scratch of the neural bodies' records, latent_table: g_latent (DssWorld.igr_latent is set)."""
    NFc = 3 * (1 + fd // 2) + 8
    names = [n for n, _k in ADJ_FIELDS if n.startswith("igr_bw_")] * bool(igr) + ["g_latent"] * bool(latent_table)
    every = igr_shapes(1, 1, 1, B, nb, maxc)
    extra = {n: every[n] for n in names}
    return {
        **extra,
        "a_pose": (B, nb, 7), "a_vel": (B, nb, 6), "a_geom": (B, 10, maxc), "a_last_dt": (B,), "a_dt": (B,),
        "g_mass": (B, nb), "g_inertia": (B, nb, 9), "g_rest": (B, nb), "g_fric": (B, nb), "g_fext": (B, nb, 6),
        "g_prm": (B, nb, 3), "g_verts": (NV, 3), "cur_slot": (B,), "lo_slot": (B,), "bw_active": (B,),
        "a_x": (B, 6 * nb), "dMblk": (B, nb, 36), "dpvec": (B, 6 * nb), "dcop": (B, NFc, maxc),
        "cscr": (B, CSCR_ROWS, maxc), "bw_nc": (B,),
    }
