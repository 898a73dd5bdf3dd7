"""CPU: the C-ABI library builds, loads and exports every symbol include/*.h declares; the ctypes mirrors of the structs
list the header's fields in the header's order."""
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


def test_struct_mirrors_follow_the_header():
    # dss_world_sizeof() checks the size only: two fields of one size that swap places or are renamed pass it
    from diffsdfsim_amd import world_abi
    assert struct_fields("DssWorld") == [n for n, _ in world_abi.FIELDS]
    assert struct_fields("DssAdjoint") == [n for n, _ in world_abi.ADJ_FIELDS]


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch
    from diffsdfsim_amd import _lib
    from diffsdfsim_amd.lcp import LCPFunction
    Q = torch.eye(3, dtype=torch.double)[None]
    with pytest.raises(_lib.HipLibraryError):
        LCPFunction()(Q, torch.zeros(1, 3).double(), torch.ones(1, 2, 3).double(), torch.ones(1, 2).double(),
                      torch.tensor([]), torch.tensor([]), torch.zeros(1, 2, 2).double())
