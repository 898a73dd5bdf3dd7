"""CPU: the C-ABI library builds, loads and exports every symbol include/*.h declares; the ctypes mirrors of the structs
list the header's fields in the header's order; the prototype table and the constants of world_abi follow the header."""
import ctypes
import glob
import os
import re

from helpers import ROOT


def header_text():
    text = "".join(open(h).read() for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))))
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def declared_symbols():
    return sorted(set(re.findall(r"\b(dss_[a-z0-9_]+)\s*\(", header_text())))


def struct_fields(name):
    """Field names of `typedef struct <name> {...}` in declaration order; `T *a, *b;` gives a, b and a nested DssIgrNet
    member m gives m_<field> for each of DssIgrNet's fields."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header_text(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        if decl.split()[0] == "DssIgrNet":
            names += ["%s_%s" % (decl.split()[1], f) for f in struct_fields("DssIgrNet")]
            continue
        names += [re.findall(r"\w+", piece)[-1] for piece in decl.split(",")]
    return names


def header_prototypes():
    """{name: (return kind, argument kinds)} of every dss_* prototype of the header, in world_abi.PROTOTYPES' spelling:
    an argument with `*` is a pointer 'p', otherwise its type is int 'i', double 'd' or size_t 'z'."""
    text = re.sub(r"typedef struct (\w+) \{.*?\} \1;", "", header_text(), flags=re.S)
    kind = {"int": "i", "double": "d", "size_t": "z", "void": "v"}
    protos = {}
    for ret, name, args in re.findall(r"\b(int|size_t|void)\s+(dss_\w+)\s*\(([^)]*)\)\s*;", text):
        assert name not in protos, "%s declared twice" % name
        args = [] if args.strip() in ("", "void") else [a.strip() for a in args.split(",")]
        protos[name] = (kind[ret], "".join("p" if "*" in a else kind[a.replace("const ", "").split()[0]] for a in args))
    return protos


def header_defines():
    """{name: value} of the header's #defines whose value is an integer expression."""
    out = {}
    for name, val in re.findall(r"^#define (DSS_\w+)[ \t]+(\(?-?\d[\d <()-]*?)[ \t]*$", header_text(), flags=re.M):
        out[name] = eval(val, {"__builtins__": {}})
    return out


def test_library_exports_every_declared_symbol():
    from diffsdfsim_amd import _lib
    _lib.build()
    L = _lib.lib()
    syms = declared_symbols()
    assert len(syms) >= 4
    for s in syms:
        assert hasattr(L, s), "missing export %s" % s
    assert L.dss_abi_version() == _lib.ABI_VERSION
    for s in ("dss_diag_set_lcp_stamps", "dss_diag_set_np_stamps", "dss_diag_latency"):
        assert not hasattr(L, s), "diagnostic export %s in the product library" % s
    # _lib.lib() has bound every declared function: none is left to ctypes' guess (a bare int passed as a 32-bit C int)
    from diffsdfsim_amd import world_abi
    ctype = {"i": ctypes.c_int, "z": ctypes.c_size_t}
    for s in syms:
        ret, args = world_abi.PROTOTYPES[s]
        fn = getattr(L, s)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), "%s not bound" % s
        assert fn.restype is ctype[ret], s


def test_prototype_table_follows_the_header():
    from diffsdfsim_amd import world_abi
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) == 53
    assert sorted(world_abi.PROTOTYPES) == sorted(protos)
    for name, sig in protos.items():
        assert world_abi.PROTOTYPES[name] == sig, name
    assert not set(world_abi.OPTIONAL_PROTOTYPES) & set(protos)


def test_constants_follow_the_header():
    from diffsdfsim_amd import _lib, world_abi
    d = header_defines()
    assert _lib.ABI_VERSION == world_abi.ABI_VERSION == d["DSS_ABI_VERSION"]
    for name in ("CAND_FIELDS", "N_ACTIVE_OVERFLOW", "IGR_HDR", "IGR_ROUNDS", "CSCR_ROWS"):
        assert getattr(world_abi, name) == d["DSS_" + name], name
    shapes = sorted(n for n in d if n.startswith("DSS_SHAPE_"))
    assert len(shapes) == 8 and sorted(d[n] for n in shapes) == list(range(8))
    for name in shapes:
        assert getattr(world_abi, name[4:]) == d[name], name
    assert sorted(n for n in vars(world_abi) if n.startswith("SHAPE_")) == [n[4:] for n in shapes]
    # the headers beside diffsdfsim_hip.h
    from diffsdfsim_amd import chamfer, grids, pointcloud
    for name in ("CIRCLE", "RECT", "BOWL", "GRID", "MAXCAND", "OVER_CAP", "OVER_CAND", "MALFORMED"):
        assert getattr(world_abi, "SDF2D_" + name) == d["DSS_SDF2D_" + name], name
    assert pointcloud.OUT_IGR == d["DSS_PC_IGR_OUT"]
    assert grids.BLOCK == d["DSS_GRID_BLOCK"]
    assert (chamfer.TILE, chamfer.QUERIES) == (d["DSS_CHAMFER_TILE"], d["DSS_CHAMFER_QUERIES"])


def test_struct_mirrors_follow_the_header():
    # dss_world_sizeof() checks the size only: two fields of one size that swap places or are renamed pass it
    from diffsdfsim_amd import world_abi
    assert struct_fields("DssWorld") == [n for n, _ in world_abi.FIELDS]
    assert struct_fields("DssAdjoint") == [n for n, _ in world_abi.ADJ_FIELDS]
    assert struct_fields("DssIgrNet") == [n for n, _ in world_abi.DssIgrNet._fields_] == list(world_abi.IGR_NET_FIELDS)
    assert struct_fields("DssSdf2dGrids") == [n for n, _ in world_abi.DssSdf2dGrids._fields_] == ["ngrids"] + list(world_abi.SDF2D_GRID_FIELDS)


class _Lacking:
    """Stands in for a loaded library: every function of world_abi.PROTOTYPES but one, as plain attributes."""

    def __init__(self, lacking):
        from diffsdfsim_amd import world_abi
        for name in world_abi.PROTOTYPES:
            if name != lacking:
                setattr(self, name, lambda *a: 0)


def test_bind_raises_on_a_missing_declared_function():
    import pytest
    from diffsdfsim_amd import world_abi
    assert world_abi.bind(_Lacking(None)).dss_shade_render.argtypes is not None      # (complete, and without the optional ones: binds)
    with pytest.raises(AttributeError, match=r"\bdss_shade_render\b"):
        world_abi.bind(_Lacking("dss_shade_render"))


def test_loader_names_the_missing_function():
    import pytest
    from diffsdfsim_amd import _lib
    assert isinstance(_lib.bind_or_raise(_Lacking(None)), _Lacking)
    with pytest.raises(_lib.HipLibraryError, match=r"does not export .*\bdss_chamfer_nn\b.*rebuild it"):
        _lib.bind_or_raise(_Lacking("dss_chamfer_nn"))


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch
    from diffsdfsim_amd import _lib
    from diffsdfsim_amd.lcp import LCPFunction
    Q = torch.eye(3, dtype=torch.double)[None]
    with pytest.raises(_lib.HipLibraryError):
        LCPFunction()(Q, torch.zeros(1, 3).double(), torch.ones(1, 2, 3).double(), torch.ones(1, 2).double(),
                      torch.tensor([]), torch.tensor([]), torch.zeros(1, 2, 2).double())
