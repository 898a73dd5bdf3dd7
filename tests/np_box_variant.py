"""Shared by test_np_box_variant_gpu.py and test_np_box_variant_emu.py: step the same scenes through two compilations of the
narrow phase and hold every output of the rollout and of the reverse sweep to equality, bit for bit."""
import numpy as np

import rollout_helpers as R

# what a rollout leaves behind: the current contacts, the state, and the tape the reverse sweep reads
WORLD_ARRAYS = ("nc", "c_body", "c_face", "c_abc", "c_geom", "pose", "vel", "t", "nsub", "last_dt", "toc", "overflow",
                "tp_pose", "tp_vel", "tp_dt", "tp_t", "tp_nc", "tp_body", "tp_face", "tp_abc", "tp_geom", "tp_x", "tp_lam", "tp_slack", "tp_nu", "tp_flags")
FLOOR = (6.0, 1.0, 6.0)
ENGINE = dict(maxc=128, max_cand=1024, max_pc=32, max_sub=96)


def stack_spec(push):
    from diffsdfsim_amd import scenes
    return scenes.box_stack(4, nbox=3, seed=77, floor_dims=FLOOR, push=push)


def mixed_spec():
    """Two scenes of two bodies: floor + box, floor + sphere (scenes.sphere_drop), their mesh tables joined."""
    from diffsdfsim_amd import scenes
    a = scenes.box_stack(1, nbox=1, seed=5, floor_dims=FLOOR, push=0.2)
    b = scenes.sphere_drop(1, seed=5, floor_dims=FLOOR)
    spec = {k: np.concatenate([a[k], b[k]]) for k in a if k not in ("meshes", "mesh_vgrad", "mesh_id")}
    spec["meshes"] = a["meshes"] + b["meshes"]
    spec["mesh_vgrad"] = a["mesh_vgrad"] + b["mesh_vgrad"]
    spec["mesh_id"] = np.concatenate([a["mesh_id"], b["mesh_id"] + len(a["meshes"])])
    return spec


def rollout(spec, lean, nsteps, backend=None, **kw):
    """`nsteps` outer steps and the reverse sweep of sum |pos_T|^2.  lean: the engine's classification forced to the lean
    variant (spec['full_kernels'] = False); otherwise the engine classifies the batch itself.
    Returns (engine, {name: array} of every world array above and every array of the adjoint)."""
    from diffsdfsim_amd.engine import BatchEngine
    spec = dict(spec)
    if lean:
        spec["full_kernels"] = False
    E = BatchEngine(spec, backend=backend, **{**ENGINE, **kw})
    R.rollout_and_sweep(E, nsteps)
    out = {k: E.get(k).copy() for k in WORLD_ARRAYS}
    out.update({"adj_" + k: E.be.to_numpy(v).copy() for k, v in E.adj.items()})
    return E, out


def assert_identical(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert (a[k] == b[k]).all(), (k, int((a[k] != b[k]).sum()))
