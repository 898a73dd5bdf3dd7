"""CPU: the ABI of contact stepping with a 4-number latent code (DSS_ABI_VERSION 4) -- the latent table DssWorld.igr_latent and
its adjoint DssAdjoint.g_latent in the header and in the ctypes mirror, the size of the reverse sweep's latent-derivative
scratch, and what BatchEngine demands of a spec with neural bodies (checked before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT


def header():
    return open(os.path.join(ROOT, "include", "diffsdfsim_hip.h")).read()


def test_header_declares_the_latent_table():
    h = header()
    assert re.search(r"#define DSS_ABI_VERSION 4\b", h)
    assert re.search(r"#define DSS_IGR_LATENT_MAX 4\b", h)
    world = re.search(r"typedef struct DssWorld \{(.*?)\} DssWorld;", h, flags=re.S).group(1)
    adjoint = re.search(r"typedef struct DssAdjoint \{(.*?)\} DssAdjoint;", h, flags=re.S).group(1)
    assert re.search(r"const double \*igr_latent;", world)
    assert re.search(r"double \*g_latent;", adjoint)


def test_mirror_has_both_fields():
    from diffsdfsim_amd import world_abi as abi
    assert abi.ABI_VERSION == 4 and abi.IGR_LATENT_MAX == 4
    assert ("igr_latent", "pd") in abi.FIELDS and ("g_latent", "pd") in abi.ADJ_FIELDS
    # the table is a pointer of its own, next to the network's latent SIZE inside the nested DssIgrNet
    W = abi.DssWorld()
    W.igr.latent, W.igr_latent = 4, 4096
    assert (W.igr.latent, W.igr_latent) == (4, 4096)
    assert abi.DssWorld.igr_latent.size == ctypes.sizeof(ctypes.c_void_p) and abi.DssWorld.igr.size == ctypes.sizeof(abi.DssIgrNet)
    assert abi.DssWorld.igr_latent.offset + 8 == ctypes.sizeof(abi.DssWorld)
    # DssAdjoint follows DssWorld in the kernel arguments without padding
    assert ctypes.sizeof(abi.DssWorld) % 8 == 0
    assert abi.DssAdjoint.g_latent.offset + 8 == ctypes.sizeof(abi.DssAdjoint)


def test_latent_derivative_scratch_holds_four_columns():
    from diffsdfsim_amd import world_abi as abi
    B, nb, maxc = 3, 2, 16
    cap = B * 2 * maxc
    s = abi.igr_shapes(4, 100, 64, B, nb, maxc)
    assert int(np.prod(s["igr_bw_grad"])) == cap * 3 + cap * 4      # d phi / d xyz [cap][3], then d phi / d latent [cap][4]
    assert s["igr_latent"] == s["g_latent"] == (B, nb, 4)
    a = abi.adjoint_shapes(B, nb, maxc, 8, igr=True, latent_table=True)
    assert a["igr_bw_grad"] == s["igr_bw_grad"] and a["g_latent"] == (B, nb, 4)
    assert "g_latent" not in abi.adjoint_shapes(B, nb, maxc, 8, igr=True) and "igr_bw_grad" not in abi.adjoint_shapes(B, nb, maxc, 8)
    assert "igr_latent" not in abi.igr_shapes(4, 100, 64)


def fake_packed(width, latent):
    return dict(W0=np.zeros((width, latent + 3)))      # (check_igr_spec reads the network's shape off W0)


def test_spec_validation():
    from diffsdfsim_amd.engine import check_igr_spec
    B, nb = 2, 3
    base = dict(pose=np.zeros((B, nb, 7)))
    lat = np.zeros((B, nb, 4)); lat[:, 2] = (0.1, 0.2, 0.3, 0.4)
    with pytest.raises(ValueError, match="igr_net"):
        check_igr_spec(dict(base))
    # the (256, 4) network needs the table ...
    with pytest.raises(ValueError, match="igr_latent"):
        check_igr_spec(dict(base, igr_net=fake_packed(256, 4)))
    got = check_igr_spec(dict(base, igr_net=fake_packed(256, 4), igr_latent=lat.tolist()))
    assert got.dtype == np.float64 and np.array_equal(got, lat)
    with pytest.raises(ValueError, match="shape"):
        check_igr_spec(dict(base, igr_net=fake_packed(256, 4), igr_latent=lat[:, :, :3]))
    # ... the (128, 2) network reads shape_prm and refuses one
    assert check_igr_spec(dict(base, igr_net=fake_packed(128, 2))) is None
    with pytest.raises(ValueError, match="igr_latent"):
        check_igr_spec(dict(base, igr_net=fake_packed(128, 2), igr_latent=lat))
    with pytest.raises(NotImplementedError):
        check_igr_spec(dict(base, igr_net=fake_packed(64, 2)))


def test_set_latents_puts_the_code_where_the_network_reads_it():
    from diffsdfsim_amd import scenes
    spec = scenes._base(2, 2)
    scenes.set_latents(spec, 1, np.array([[1.0, 2.0], [3.0, 4.0]]), fake_packed(128, 2))
    assert "igr_latent" not in spec and np.array_equal(spec["shape_prm"][:, 1], [[1, 2, 0], [3, 4, 0]])
    spec = scenes._base(2, 2)
    scenes.set_latents(spec, 1, np.arange(8.0).reshape(2, 4), fake_packed(256, 4))
    assert np.array_equal(spec["igr_latent"][:, 1], np.arange(8.0).reshape(2, 4)) and not spec["igr_latent"][:, 0].any()
    assert not spec["shape_prm"][:, 1].any()
    with pytest.raises(ValueError):
        scenes.set_latents(spec, 1, np.zeros((2, 2)), fake_packed(256, 4))
