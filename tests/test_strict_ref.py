"""tests/strict_ref.py without a device: the restatement of k_blend_strict IS the oracle's arithmetic, its interval is closed
almost everywhere on the named frames, and it tells wrong blends from the right one.

Every frame is built through the oracle's K1 and depth sort (blend_ref.oracle_frame).

  restatement  libm_walk (the walk with the C library's expf, which the oracle calls) equals oracle.render(mode 1 / 2, and 0) bit
               for bit, and the oracle's image passes `check` against the interval of the walk with the float64 exp.
  open cap     the share of pixels whose interval is still open at the end is at most strict_ref.MAX_OPEN = 1 % on every named
               frame in rgba16float and rgba8unorm.  A condition on the frames, from the reference alone: everywhere else the
               device is held to the bit.
  f32 width    on an rgba32float target nothing swallows the exp uncertainty; the largest hi - lo stays below 2e-5, the gate
               test_strict_kernel_against_the_oracle has.
  composite    target= and occluder= of the walk against walks that need neither.
  defects      every wrong walk of strict_ref.DEFECTS puts at least one value outside its interval on the frames named for it:

               defect            frames                                             formats
               f16_rtz           every named frame                                  rgba16float
               u8_trunc          every named frame                                  rgba8unorm
               near_to_far       every named frame but stacks-k1                    both
               round_once        every named frame but stacks-k1                    both
               alpha_unrounded   every named frame but stacks-k1 and saturated      both  (saturated: alpha is 1 all over)
               no_clamp          saturated                                          both
               tail_twice        stacks-k1, -k63, -k65, -k129, -k193                both  (k = 64, 128: the walk is unchanged)

               (one record alone has no order, and one rounding at the end is its only rounding.)

  one unit     f16_rtz and u8_trunc on stacks-k1 leave every value within one unit of the centre image -- one record is one
               rounding of one value, and two roundings of a value are neighbours -- while `check` sees them on about half the
               values: the one-unit gate of test_strict_kernel_against_the_oracle lets that frame through.  On the longer
               stacks no such bound can be derived and none holds: rounding toward zero takes a whole unit off wherever a faint
               record pulls the destination down by less than one, so the error grows with the list (measured, f16 / unorm8:
               f16_rtz up to 51 units at k = 193, u8_trunc up to 32), and an unrounded alpha adds up the faint records that the
               per-record rounding swallows (up to 8 / 2 units).  The figures of every stack are printed; alpha_unrounded on
               one record is no defect at all (the store is its one rounding), so for it only "caught" is claimed.
"""
import functools

import numpy as np
import pytest

import blend_ref as B
import oracle_lib
import strict_ref as S

NARROW = ("rgba16float", "rgba8unorm")
ALL = tuple(S.FRAMES)
NOT_K1 = tuple(n for n in ALL if n != "stacks-k1")
TAIL = tuple(f"stacks-k{k}" for k in S.STACK_K if k % 64)
NO_TAIL = tuple(f"stacks-k{k}" for k in S.STACK_K if k % 64 == 0)
DEFECT_FRAMES = {"f16_rtz": (ALL, ("rgba16float",)), "u8_trunc": (ALL, ("rgba8unorm",)), "near_to_far": (NOT_K1, NARROW),
                 "round_once": (NOT_K1, NARROW), "alpha_unrounded": (tuple(n for n in NOT_K1 if n != "saturated"), NARROW),
                 "no_clamp": (("saturated",), NARROW), "tail_twice": (TAIL, NARROW)}
DEFECT_CASES = [(d, n, f) for d, (names, fmts) in DEFECT_FRAMES.items() for n in names for f in fmts]


@functools.lru_cache(maxsize=None)
def _frame(name):
    rows, viewport = S.frame(name)
    frame = B.oracle_frame(oracle_lib, rows, viewport)
    assert len(frame["sorted"]) >= min(len(rows), 1)
    return frame, viewport


def _ref(name, fmt):
    frame, (w, h) = _frame(name)
    return S.reference(frame, w, h, fmt, S.exact_background(fmt))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_defect_table_names_every_defect():
    assert sorted(DEFECT_FRAMES) == sorted(S.DEFECTS)


def test_the_stacks_are_whole_lists():
    """Every record of a stack is visible, so the frame's length is the k that tail_twice and the chunk boundaries are about."""
    for k in S.STACK_K:
        frame, _ = _frame(f"stacks-k{k}")
        assert len(frame["sorted"]) == k


def test_the_edge_viewports_have_partial_quadrants_and_odd_tile_counts():
    """33 x 17 cuts through quadrants; 72 x 40 leaves whole quadrants of its last tiles outside, and its tile count at every
    shape is no multiple of the eight tiles one round of the kernel's tile mapping covers (15 of 16 px: more than one round)."""
    for name, tiles16 in (("edges-33x17", 6), ("edges-72x40", 15)):
        w, h = S.frame(name)[1]
        assert (w % 16 or h % 16) and -(-w // 16) * -(-h // 16) == tiles16
    w, h = S.frame("edges-33x17")[1]
    assert w % 8 and h % 8
    w, h = S.frame("edges-72x40")[1]
    assert -(-w // 16) * -(-h // 16) > 8 and (-(-w // 16) * -(-h // 16)) % 8 and (-(-w // 32) * -(-h // 16)) % 8 and (-(-w // 32) * -(-h // 32)) % 8


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("name", ALL)
def test_restatement_against_the_oracle(name, fmt):
    frame, (w, h) = _frame(name)
    bg = S.exact_background(fmt)
    want = oracle_lib.render(frame["splats"], frame["sorted"], w, h, bg, S.ORACLE_MODE[fmt])
    got = S.libm_walk(frame, w, h, fmt, bg)
    assert np.array_equal(_bits(got), _bits(want)), "the walk with libm's expf is not the oracle's image"
    res = S.check(want, _ref(name, fmt), fmt)
    print(f"{name} {fmt}: oracle against the interval: {res}")
    assert res["outside"] == 0, res["first"]


@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("name", ALL)
def test_open_pixels_stay_under_the_cap(name, fmt):
    ref = _ref(name, fmt)
    share, ever = float(ref["open"].mean()), float(ref["ever_open"].mean())
    print(f"{name} {fmt}: open at the end {share:.4%} of the pixels, open at some record {ever:.4%}")
    assert share <= S.MAX_OPEN
    assert (ref["lo"] <= ref["centre"]).all() and (ref["centre"] <= ref["hi"]).all()


@pytest.mark.parametrize("name", ALL)
def test_f32_interval_stays_inside_the_existing_gate(name):
    ref = _ref(name, "rgba32float")
    width = float((ref["hi"].astype(np.float64) - ref["lo"].astype(np.float64)).max())
    print(f"{name} rgba32float: largest hi - lo {width:.3e}")
    assert width < 2e-5
    assert (ref["lo"] <= ref["centre"]).all() and (ref["centre"] <= ref["hi"]).all()


def test_unorm8_rounds_half_to_even():
    v = (np.array([0.5, 1.5, 2.5, 126.5, 127.5]) / 255.0).astype(S.F)
    exact = (v * S.F(255.0)).astype(np.float64) % 1.0 == 0.5
    assert exact.any()
    got = S.words("rgba8unorm", S.quantize(v, "rgba8unorm"))
    assert np.array_equal(got[exact], np.array([0, 2, 2, 126, 128], dtype=np.uint8)[exact])
    assert np.array_equal(S.quantize(np.array([np.nan, -1.0, 2.0], dtype=S.F), "rgba8unorm"), np.array([0.0, 0.0, 1.0], dtype=S.F))


@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("name", ["general", "stacks-k129"])
def test_composite_walks(name, fmt):
    """target= of the stored background is the walk over that background; an occluder behind everything changes nothing; a
    constant occluder between two list positions is the walk of the records in front of it."""
    frame, (w, h) = _frame(name)
    bg = S.exact_background(fmt)
    ref = _ref(name, fmt)
    stored = np.broadcast_to(S.words(fmt, np.asarray(bg, dtype=S.F)), (h, w, 4)).copy()
    stored = stored if fmt == "rgba8unorm" else stored.view(np.float16)
    z = frame["z"]
    behind = np.full((h, w), np.inf, dtype=np.float32)
    loaded = S.strict_walk(frame, w, h, fmt, target=stored, occluder=behind, z=z)
    for key in ("lo", "hi", "centre"):
        assert np.array_equal(_bits(loaded[key]), _bits(ref[key])), key
    order = frame["sorted"].astype(np.int64)  # far to near
    cut = len(order) // 3
    d = np.float32((np.float64(z[order[cut - 1]]) + np.float64(z[order[cut]])) / 2)
    assert z[order[cut]] < d < z[order[cut - 1]]
    front = {"splats": frame["splats"], "sorted": frame["sorted"][cut:]}
    want = S.strict_walk(front, w, h, fmt, bg)
    got = S.strict_walk(frame, w, h, fmt, bg, occluder=np.full((h, w), d, dtype=np.float32), z=z)
    for key in ("lo", "hi", "centre"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    assert not np.array_equal(_bits(got["centre"]), _bits(ref["centre"]))


@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("occluder", S.OCCLUDERS)
@pytest.mark.parametrize("name", ["general", "stacks-k129"])
def test_open_pixels_of_the_composite_cases(name, occluder, fmt):
    """The cap, on what tests/test_gpu_blend_strict.py composites: a random target loaded, behind each occluder."""
    frame, (w, h) = _frame(name)
    ref = S.strict_walk(frame, w, h, fmt, target=S.random_target(fmt, w, h), occluder=S.occluder_plane(occluder, frame, frame["z"], w, h),
                        z=frame["z"])
    print(f"{name} {occluder} {fmt}: open at the end {float(ref['open'].mean()):.4%} of the pixels")
    assert ref["open"].mean() <= S.MAX_OPEN


@pytest.mark.parametrize("defect,name,fmt", DEFECT_CASES)
def test_defects_leave_the_interval(defect, name, fmt):
    frame, (w, h) = _frame(name)
    bad = S.strict_walk(frame, w, h, fmt, S.exact_background(fmt), defect=defect)
    assert bad["lo"] is None
    res = S.check(bad["centre"], _ref(name, fmt), fmt)
    print(f"{defect} {name} {fmt}: {res['outside']} values outside, at most {res['max_units']} units from the centre")
    assert res["outside"] >= 1


@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("name", NO_TAIL)
def test_a_whole_last_chunk_has_no_tail(name, fmt):
    frame, (w, h) = _frame(name)
    bad = S.strict_walk(frame, w, h, fmt, S.exact_background(fmt), defect="tail_twice")
    assert np.array_equal(_bits(bad["centre"]), _bits(_ref(name, fmt)["centre"]))


@pytest.mark.parametrize("defect,fmt", [("f16_rtz", "rgba16float"), ("u8_trunc", "rgba8unorm"), ("alpha_unrounded", "rgba16float"),
                                        ("alpha_unrounded", "rgba8unorm")])
def test_what_a_one_unit_gate_lets_through(defect, fmt):
    """See "one unit" above: asserted on the one-record stack, where it can be derived; printed for the others."""
    for name in S.STACKS:
        frame, (w, h) = _frame(name)
        bad = S.strict_walk(frame, w, h, fmt, S.exact_background(fmt), defect=defect)
        res = S.check(bad["centre"], _ref(name, fmt), fmt)
        print(f"{defect} {name} {fmt}: at most {res['max_units']} units from the centre, {res['outside']} of {4 * res['pixels']} values outside")
        if name == "stacks-k1":
            assert res["max_units"] <= 1
            if defect != "alpha_unrounded":
                assert res["outside"] >= 0.25 * 4 * res["pixels"]
