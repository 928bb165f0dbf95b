"""The frames of tests/test_gpu_blend_boundary.py, without a device: every frame is built through the oracle's K1 and depth sort
(blend_ref.oracle_frame) and walked in float64 (blend_ref.reference), and the test shows FROM THE REFERENCE ALONE that the frame
can tell a correct k_blend from one that loses a marker record or lets two neighbouring markers change places:

  * list position i is stack index i, every record of the cloud is in the frame, no pixel has a fragment within f32 rounding of
    the cut-off (`undecided` is empty), and in the faint frames T ends above 2^-10 at every pixel;
  * for every marker m and every 8 x 8 quadrant its stack covers, drop=m moves the float64 colour or T somewhere in that quadrant
    by at least SENSITIVITY = 10 x the device test's gate, and so does swap=(m, m + 1) for every pair of neighbouring markers;
  * in the frames of the depth forms the median crossing of the stack's centre pixels lies on the marker at list position STAGE,
    and dropping that marker changes the median plane;
  * in the saturating frames the first list position that meets T < T_MIN lies below STAGE in one whole quadrant of tile (0, 0) and at
    or above it in another.

"Covers" is NARROWER here than "the cut-off ellipse reaches the quadrant" (blend_ref.COVERED): some pixel of the quadrant gives the stack's records at least 0.6 of their opacity.  Exchanging two
records moves a pixel by g^2 b_m b_{m+1} T |colour_m - colour_{m+1}| (g = that share): in a quadrant the cut-off ellipse merely
grazes (g = 0.05 .. 0.45 in these frames) no pair of opacities whose 19 markers leave T above 2^-10 makes that visible.  Such
quadrants still walk the records, and the device test compares them with the same gate; they just cannot be shown to bite."""
import numpy as np
import pytest

import blend_ref as B

SENSITIVITY = 10 * B.GATE
SPECS = B.all_specs()


def _frame(oracle, spec):
    w, h = spec.viewport
    frame = B.oracle_frame(oracle, spec.rows, spec.viewport)
    return frame, B.reference(frame, frame["z"], w, h)


def _moved(ref, base, box):
    """Per quadrant of the box, the most any pixel's colour or T moved; ref = (C, T) over the box."""
    return B.quadrants(np.maximum(np.abs(ref[0] - base["C"][box]).max(axis=2), np.abs(ref[1] - base["T"][box])))


def _same(fast, slow):
    return np.abs(fast[0] - slow["C"]).max() <= 1e-12 and np.abs(fast[1] - slow["T"]).max() <= 1e-12


@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_frame_orders_and_exposes_its_markers(oracle, spec):
    w, h = spec.viewport
    frame, base = _frame(oracle, spec)
    near_to_far = frame["src_index"][frame["sorted"].astype(np.int64)[::-1]]
    assert len(near_to_far) == len(spec.rows), "K1 culled a record of the stack"
    assert not base["undecided"].any()
    if spec.faint:
        assert base["T"].min() > 2.0 ** -10, base["T"].min()
    worst = np.inf
    b = B.record_weights(frame, w, h)
    assert _same(B.walk(frame, b), base)
    for st in spec.stacks:
        if st["k"] == 0:
            continue
        rows_of_stack = near_to_far[(near_to_far >= st["first"]) & (near_to_far < st["first"] + st["k"])]
        assert np.array_equal(rows_of_stack, st["first"] + np.arange(st["k"])), "list position is not stack index"
        if len(spec.stacks) == 1:
            assert np.array_equal(near_to_far, np.arange(st["k"]))
        slot = int(np.nonzero(frame["src_index"] == st["first"])[0][0])
        g = B.falloff(frame, w, h, slot)
        cy, cx = np.unravel_index(np.argmax(g), g.shape)
        assert abs(cx + 0.5 - st["centre"][0]) <= 0.5 and abs(cy + 0.5 - st["centre"][1]) <= 0.5 or not spec.faint
        box = B.footprint_box(g)  # (outside it the stack's records weigh nothing: nothing moves there)
        covered = B.quadrants(g[box]) >= B.COVERED
        assert covered.any() or not spec.faint
        where = [B.list_position(frame, st["first"] + m) for m in st["positions"]]
        for m, p in zip(st["positions"], where):
            moved = _moved(B.walk(frame, b, drop=p, box=box), base, box)[covered].min()
            worst = min(worst, moved)
            assert moved >= SENSITIVITY, f"drop={m}: the best covered quadrant pixel moves by {moved:.2e} only"
        for (m, p), (m1, p1) in zip(zip(st["positions"], where), zip(st["positions"][1:], where[1:])):
            if m1 != m + 1:
                continue
            moved = _moved(B.walk(frame, b, swap=(p, p1), box=box), base, box)[covered].min()
            worst = min(worst, moved)
            assert moved >= SENSITIVITY, f"swap=({m}, {m1}): the best covered quadrant pixel moves by {moved:.2e} only"
        if st is not spec.stacks[0]:
            continue
        if where:  # composite_f64's own drop= and swap=, once per frame: the last marker of its first stack, and the last two
            assert _same(B.walk(frame, b, drop=where[-1]), B.reference(frame, None, w, h, drop=where[-1]))
        if len(where) > 1:
            assert _same(B.walk(frame, b, swap=(where[-2], where[-1])), B.reference(frame, None, w, h, swap=(where[-2], where[-1])))
    print(f"{spec.name}: least movement of a covered quadrant under any drop / swap {worst:.2e} (needs {SENSITIVITY:.0e}); "
          f"T ends at {base['T'].min():.3e} .. {base['T'].max():.3e}")
    for shape in B.SHAPES:  # (asserts the clearances that make the device test's exact list lengths safe)
        spec.list_lengths(shape), spec.list_lengths(shape, coarse=True)
    B._REF_CACHE.clear()


@pytest.mark.parametrize("shape,k", B.MEDIAN_CASES, ids=[f"{s}-{k}" for s, k in B.MEDIAN_CASES])
def test_median_crossing_sits_on_the_first_record_of_the_second_batch(oracle, shape, k):
    spec = B.median(shape, k)
    frame, base = _frame(oracle, spec)
    stage = spec.stage
    z_of = frame["z"][frame["sorted"].astype(np.int64)[::-1]]  # near -> far
    centre = (slice(15, 17), slice(15, 17))
    assert np.all(base["median"][centre] == z_of[stage]), "the centre pixels' crossing is not on the marker at STAGE"
    crossed = base["T"] <= 0.5
    assert crossed[centre].all()
    assert np.all(base["median"][crossed] >= z_of[stage]), "a crossing in the first batch"
    assert base["tcross"][centre].min() > 100 * B.NEAR_HALF
    dropped = B.reference(frame, frame["z"], 32, 32, drop=stage)
    assert np.all(dropped["median"][centre] != base["median"][centre])
    B._REF_CACHE.clear()


@pytest.mark.parametrize("shape", list(B.SHAPES))
def test_saturation_straddles_the_batch_boundary(oracle, shape):
    spec = B.saturating(shape)
    frame, base = _frame(oracle, spec)
    near, far = (base["first_below"][8 * q[1]:8 * q[1] + 8, 8 * q[0]:8 * q[0] + 8] for q in spec.quadrants)
    print(f"{spec.name}: first list position below T_MIN {near.min()} .. {near.max()} in quadrant {spec.quadrants[0]}, "
          f"{far.min()} .. {far.max()} in quadrant {spec.quadrants[1]}")
    assert near.max() < spec.stage <= far.min()
    assert far.max() < len(spec.rows)
    B._REF_CACHE.clear()
