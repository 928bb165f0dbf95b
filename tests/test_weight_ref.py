"""contrib_ref, attrib_ref and values_ref are three sinks of one float64 walk (tests/weight_ref.py): on stack frames built
through the oracle's K1 and depth sort (blend_ref.oracle_frame), without a device, they agree where their definitions say so."""
import numpy as np
import pytest

import attrib_ref
import blend_ref
import contrib_ref
import values_ref
from attrib_frames import _stack

VIEW = (32, 32)


@pytest.mark.parametrize("opacity", [0.002, 0.9], ids=["faint", "opaque"])
@pytest.mark.parametrize("k", [5, 257])
def test_the_three_references_walk_the_same_weights(oracle, k, opacity):
    w, h = VIEW
    frame = blend_ref.oracle_frame(oracle, _stack(k, opacity), VIEW)
    plain = contrib_ref.contrib_f64(frame, w, h, k)
    assert (plain["kept"] > 0).all() and plain["sum"].sum() > 0
    # v = w * 1.0 and the same order of summation: exactly the plain result
    unit = attrib_ref.attrib_f64(frame, w, h, k, np.ones((h, w), np.float32))
    for key in ("sum", "max", "kept", "P", "U", "T"):
        assert np.array_equal(unit[key], plain[key]), key
    # a one-hot column j draws Gaussian j's weights to the plane: the same terms, summed per pixel first
    for j in sorted({0, k // 2, k - 1}):
        hot = np.zeros(k, np.float32)
        hot[j] = 1
        ref = values_ref.values_f64(frame, w, h, hot)
        assert np.array_equal(ref["T"], plain["T"])
        assert abs(ref["out"][..., 0].sum() - plain["sum"][j]) <= 1e-12 * plain["sum"][j], j
