"""GPU: the box-only compilation of the narrow phase (narrowphase_box.hip, picked when every body of the batch is a box) against
the lean one on the same scenes: contact counts, bodies, faces, barycentrics, geometry, poses, velocities, sub-step counts, the
whole tape and every array of the reverse sweep are equal with ==, not merely close.  The box-only source is the lean source
with the sphere and cylinder branches removed by the preprocessor, so the statements that run are the same."""
import pytest

import np_box_variant as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("push", [0.0, 3.0])
def test_box_only_narrow_phase_equals_the_lean_one_bit_for_bit(push):
    """scenes.box_stack(B=4, nbox=3), six steps and the reverse sweep; push > 0 slides the boxes off each other's faces, which
    brings edge contacts, ties and rejected attempts (more attempts than outer steps: a penetration halves the step)."""
    spec = V.stack_spec(push)
    El, lean = V.rollout(spec, True, 6)
    Eb, box = V.rollout(spec, False, 6)
    assert (int(El.W.shape_rare), int(El.W.shape_box)) == (0, 0)
    assert (int(Eb.W.shape_rare), int(Eb.W.shape_box)) == (0, 1)
    assert int(lean["nc"].min()) > 0 and int(lean["overflow"].max()) == 0
    if push:
        assert El.attempts > 6 and El.attempts == Eb.attempts
    assert abs(lean["adj_g_prm"]).max() > 0
    V.assert_identical(lean, box)


def test_a_batch_with_a_sphere_keeps_the_lean_narrow_phase():
    """A box scene next to a sphere drop: the engine classifies the batch as lean, and the results are those of the lean
    variant forced."""
    spec = V.mixed_spec()
    Ea, auto = V.rollout(spec, False, 6)
    El, lean = V.rollout(spec, True, 6)
    assert (int(Ea.W.shape_rare), int(Ea.W.shape_box)) == (0, 0) == (int(El.W.shape_rare), int(El.W.shape_box))
    assert int(lean["tp_nc"].max()) > 0
    V.assert_identical(auto, lean)
