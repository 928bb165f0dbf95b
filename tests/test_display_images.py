"""tests/display_images.py without a device: the EXACT class is exact (a fused and an unfused evaluation of c + background * k
agree on every value, from float64 arithmetic alone), its named edges are present, and the undecided share of the GENERAL class
stays under its cap."""
import numpy as np
import pytest

import display_images as di

F = np.float32
CASES = [(w, h, fmt) for (w, h) in di.SIZES for fmt in di.SOURCES]
IDS = [f"{w}x{h}-{fmt}" for w, h, fmt in CASES]
GENERAL_SEEDS = (0, 1)


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_exact_class_is_exact(w, h, fmt):
    """k and background * k are exact in f32, and the sum rounded once from float64 (what a fused multiply-add gives) equals
    the separately rounded f32 sum -- on every value, the non-finite ones included"""
    src = di.decode(di.exact_image(w, h, fmt))
    assert src.shape == (h, w, 4)
    for bg in di.EXACT_BACKGROUNDS:
        b32 = np.array(bg, F)
        with np.errstate(invalid="ignore", over="ignore"):
            k32 = F(1.0) - src[..., 3:4]
            k64 = 1.0 - src[..., 3:4].astype(np.float64)
            t32 = b32 * k32
            t64 = b32.astype(np.float64) * k32.astype(np.float64)
            unfused = src + t32
            fused = (src.astype(np.float64) + t64).astype(F)
        if fmt != "rgba8unorm":                                                  # (a decoded code's 1 - a is rounded: the same both ways)
            assert _same(k32.astype(np.float64), k64).all()
        assert _same(t32.astype(np.float64), t64).all()
        assert _same(unfused, fused).all()
        if fmt != "rgba8unorm":                                                  # the sum itself is exact
            with np.errstate(invalid="ignore"):
                assert _same(unfused.astype(np.float64), src.astype(np.float64) + t64).all()


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_exact_class_holds_its_edges(w, h, fmt):
    img = di.exact_image(w, h, fmt)
    n = w * h
    if fmt == "rgba8unorm":
        if n >= 256:
            for ch in range(4):
                assert len(np.unique(img[..., ch])) == 256
        return
    c, a = img[..., :3].astype(F), img[..., 3].astype(F)
    assert np.isnan(c).any() and np.isinf(c).any()
    if n >= 16:
        assert (c == -np.inf).any() and (c < 0).any() and np.isnan(a).any()
        for v in (-0.5, 0.0, 1.0, 1.5):
            assert (a == v).any(), v
        out = di.composite_f32(img, di.EXACT_BACKGROUNDS[0], "rgba8unorm")
        assert (out == 128).any() and (out == 0).any() and (out == 255).any()    # 0.5 * 255 = 127.5 -> 128, the even neighbour
        assert (c[..., 0].reshape(-1)[0] == 0.5) and out.reshape(-1, 4)[0, 0] == 128


def test_half_landings_show_the_rounding_rule():
    lands = di.half_landings()
    odd = [m for m, _ in lands if m % 2]
    even = [m for m, _ in lands if m % 2 == 0]
    assert len(odd) >= 8 and len(even) >= 8
    img = di.exact_image(129, 9, "rgba32float")
    flat = img.reshape(-1, 4)
    out = di.composite_f32(img, di.EXACT_BACKGROUNDS[3], "rgba8unorm").reshape(-1, 4)
    for i, (m, v) in enumerate(lands):
        assert flat[16 + i, 0] == F(v) and flat[16 + i, 3] == 1.0
        assert float(F(v) * F(255.0)) == m + 0.5
        assert out[16 + i, 0] == (m if m % 2 == 0 else m + 1)                   # half to even; half up would give m + 1 always
    back = di.readback(img).reshape(-1, 4)
    assert all(back[16 + i, 0] == m for i, (m, _) in enumerate(lands))          # truncation


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_undecided_share_of_the_general_class(w, h, fmt):
    """a condition on the committed images, from the float64 reference alone"""
    und = total = 0
    for seed in GENERAL_SEEDS:
        img = di.general_image(w, h, fmt, seed)
        if fmt != "rgba8unorm":
            f = img.astype(F)
            assert f.min() >= -0.25 and f.max() <= 1.25
        for surface in di.SURFACES:
            _, decided = di.composite_f64(img, di.general_background(seed), surface)
            und += int((~decided).sum())
            total += decided.size
    if w * h >= 100:
        assert und / total < di.MAX_UNDECIDED, (und, total)
    else:                                                                       # a 1 x 1 image: no value of the few may be undecided
        assert und == 0


def test_margin_is_the_derived_one():
    assert di.E_BOUND == 2.0 ** -25 + (2.0 ** -24 + 2.0 ** -25) + 2.0 ** -24 + 2.0 ** -23
    assert di.MARGIN == 255 * di.E_BOUND + 2.0 ** -17 and di.MARGIN < 1e-4


def test_readback_reference_defines_nan():
    img = np.array([[[np.nan, -np.inf, np.inf, -0.0], [0.999999, 1.5, -0.5, 0.5]]], F)
    assert di.readback(img).tolist() == [[[0, 0, 255, 0], [254, 255, 0, 127]]]
    assert di.readback(img.astype(np.float16)).tolist() == [[[0, 0, 255, 0], [255, 255, 0, 127]]]
    assert di.composite_f32(img, (0, 0, 0, 0), "bgra8unorm").tolist() == [[[255, 0, 0, 0], [0, 255, 255, 128]]]
