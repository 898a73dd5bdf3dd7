"""CPU (emulator): what test_np_box_variant_gpu.py asks of the device, on the emulated kernels -- the box-only compilation of
the narrow phase gives the lean one's results bit for bit, and the engine picks it for batches made only of boxes."""
import numpy as np

import np_box_variant as V
from emu import emu


def test_box_only_narrow_phase_equals_the_lean_one_bit_for_bit():
    spec = V.stack_spec(0.4)
    El, lean = V.rollout(spec, True, 2, backend=emu.EmuBackend())
    Eb, box = V.rollout(spec, False, 2, backend=emu.EmuBackend())
    assert (int(El.W.shape_rare), int(El.W.shape_box)) == (0, 0)
    assert (int(Eb.W.shape_rare), int(Eb.W.shape_box)) == (0, 1)
    assert int(lean["nc"].min()) > 0 and abs(lean["adj_g_prm"]).max() > 0
    V.assert_identical(lean, box)


def test_classification_of_the_batch():
    """box-only / lean / full, and the override: spec['full_kernels'] = False keeps a box batch on the lean variant."""
    from diffsdfsim_amd import scenes, world_abi as abi
    from diffsdfsim_amd.engine import BatchEngine
    kinds = lambda spec: (lambda W: (int(W.shape_rare), int(W.shape_box)))(BatchEngine(spec, backend=emu.EmuBackend(), maxc=32, max_pc=16).W)
    box = scenes.box_stack(2, nbox=1, seed=1, floor_dims=V.FLOOR)
    assert kinds(box) == (0, 1)
    assert kinds(dict(box, full_kernels=False)) == (0, 0)
    assert kinds(dict(box, full_kernels=True)) == (1, 0)
    assert kinds(V.mixed_spec()) == (0, 0)
    rounded = dict(box, shape_type=np.where(np.arange(2)[None] == 1, abi.SHAPE_BOX_ROUNDED, 0).astype(np.int32) * np.ones((2, 1), np.int32),
                   shape_aux=np.full((2, 2), 0.05))
    assert kinds(rounded) == (1, 0)
