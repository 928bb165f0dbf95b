"""The pattern clouds of tests/k1_patterns.py, checked on the CPU: what tests/test_gpu_k1_compaction.py asserts on the device
means something only if (1) the masks hold the shapes they are named for, (2) the oracle's visible set of every cloud the GPU
file prepares IS the mask, with every Gaussian at least 10 % away from every cull threshold, and (3) the frame checker reports
what a wrong compactor would produce."""
import numpy as np
import pytest

import k1_patterns as kp
from k1_patterns import B, N_BIG, N_EDGES, T, W


# ---- 1. the masks ----------------------------------------------------------------------------------------------------------
def _block_counts(m):
    pad = np.zeros(-(-len(m) // B) * B, dtype=bool)
    pad[:len(m)] = m
    return pad.reshape(-1, B).sum(axis=1)


def test_sizes():
    assert N_BIG == 68_625 and -(-N_BIG // B) == 68 > W       # more workgroups than one look-back poll covers
    assert N_BIG - (N_BIG - 1) // B * B == 17                  # the last block holds 17 Gaussians
    assert kp.mask("last_block_only", N_BIG).sum() == 17 and kp.mask("last_block_only", N_BIG)[-17:].all()
    assert set(kp.REDUCED) <= set(kp.PATTERNS) and set(kp.EDGE_PATTERNS) <= set(kp.PATTERNS)
    assert len(set(kp.PATTERNS)) == len(kp.PATTERNS)
    for n in (N_BIG,) + N_EDGES:
        for name in kp.PATTERNS:
            m = kp.mask(name, n)
            assert m.dtype == bool and m.shape == (n,)


def test_masks_hold_what_they_are_named_for():
    n = N_BIG
    whole = n // B
    m = kp.mask("one_wave_per_block", n)
    waves = m[:whole * B].reshape(whole, B // W, W).sum(axis=2)
    assert np.all((waves == W).sum(axis=1) == 1) and np.all((waves == 0).sum(axis=1) == B // W - 1)
    assert len(set(np.argmax(waves, axis=1).tolist())) == 16   # the full wave visits every (item, wave) of the block

    counts = _block_counts(kp.mask("ramp", n))
    assert {0, 64, 128, 1024} <= set(counts.tolist())
    assert {64 * k for k in range(17)} <= set(counts.tolist())  # every multiple of 64 up to the full block
    assert {63, 127} <= set(counts.tolist())                    # and one short of a multiple
    assert any(c % W not in (0, W - 1) for c in counts.tolist())

    counts = _block_counts(kp.mask("tail_after_66_empty", n))
    lead = int(np.argmax(counts > 0))
    assert lead >= 65 and counts[:lead].sum() == 0 and counts[lead:].min() > 0

    for k in range(4):
        rows = kp.mask(f"item_{k}", n)[:whole * B].reshape(whole, B // T, T).sum(axis=2)
        assert np.all(rows[:, k] == T) and rows.sum() == whole * T
    assert np.all(_block_counts(kp.mask("one_per_block", n))[:whole] == 1)
    assert np.all(_block_counts(kp.mask("alt_blocks", n))[0::2] == 0)
    assert _block_counts(kp.mask("block0_only", n)).tolist() == [B] + [0] * 67
    w = kp.mask("alt_waves", n)[:whole * B].reshape(-1, W).sum(axis=1)
    assert set(w.tolist()) == {0, W}
    assert kp.mask("lane63", n).reshape(-1)[63::W].all() and kp.mask("lane63", n).sum() == n // W
    assert kp.mask("first_only", n).nonzero()[0].tolist() == [0] and kp.mask("last_only", n).nonzero()[0].tolist() == [n - 1]
    for name, period in (("period_192", 192), ("period_997", 997)):
        assert all(period % x and x % period for x in (T, B))     # no item row or block is a whole number of periods
        assert 0 < kp.mask(name, n).sum() < n
    assert abs(kp.mask("random_50", n).mean() - 0.5) < 0.02 and 0 < kp.mask("random_1", n).mean() < 0.02 < 0.98 < kp.mask("random_99", n).mean() < 1
    for name in kp.PATTERNS:
        assert len(kp.variants(name)) == (2 if name == "random_50" else 1)
    assert [kp.variants(p)[0] for p in kp.PATTERNS[:4]] == ["clip", "frustum", "clip", "frustum"]


# ---- 2. the oracle's visible set equals the mask ---------------------------------------------------------------------------
def _visible_set_is_the_mask(ws, oracle, cl, args=None):
    r = kp.threshold_ratios(cl, oracle, args)
    m = cl.mask
    worst_in = r[m].max() if m.any() else 0.0
    assert worst_in <= kp.INSIDE + 1e-6, f"a survivor stands at {worst_in:.4f} of a cull threshold"
    if (~m).any():
        worst_out = r[~m].max(axis=1).min()
        assert worst_out >= 1.1 - 1e-6, f"a culled Gaussian is only {worst_out:.4f} x a cull threshold"
    fr = cl.oracle_frame(oracle, args)
    assert np.array_equal(fr["src_index"], np.nonzero(m)[0])
    assert fr["num_visible"] == int(m.sum())
    return fr


@pytest.mark.parametrize("viewport", kp.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("layout", kp.LAYOUTS)
@pytest.mark.parametrize("name,variant", kp.cases(kp.PATTERNS))
def test_visible_set_equals_mask_big(ws, oracle, name, variant, layout, viewport):
    _visible_set_is_the_mask(ws, oracle, kp.cloud(ws, name, N_BIG, layout, variant, viewport))


@pytest.mark.parametrize("viewport", kp.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("layout", kp.LAYOUTS)
@pytest.mark.parametrize("n", N_EDGES)
def test_visible_set_equals_mask_edges(ws, oracle, n, layout, viewport):
    for name, variant in kp.cases(kp.EDGE_PATTERNS):
        _visible_set_is_the_mask(ws, oracle, kp.cloud(ws, name, n, layout, variant, viewport))


@pytest.mark.parametrize("name", ["ramp", "one_per_block"])
def test_visible_set_equals_mask_orbit_views(ws, oracle, name):
    """The frames-in-flight test draws a "clip" cloud from nine orbit cameras: the box decides, whatever the camera."""
    cl = kp.cloud(ws, name, N_BIG, "uncompressed", "clip", (640, 480))
    views = kp.orbit_views(ws, cl, 9)
    assert len(views) == 9
    for v in views:
        _visible_set_is_the_mask(ws, oracle, cl, v)


def test_clip_culled_stay_inside_the_frustum(ws, oracle):
    """"clip" clouds at 640 x 480: the clipping box is the ONLY test a culled Gaussian fails."""
    cl = kp.cloud(ws, "random_50", N_BIG, "uncompressed", "clip", (640, 480))
    r = kp.threshold_ratios(cl, oracle)[~cl.mask]
    assert np.all((r[:, :6] >= 1.1 - 1e-6).sum(axis=1) == 1) and r[:, 6:].max() < 1.0
    cl = kp.cloud(ws, "random_50", N_BIG, "uncompressed", "frustum", (640, 480))
    r = kp.threshold_ratios(cl, oracle)[~cl.mask]
    assert r[:, :6].max() < 1.0 and np.all(r[:, 6:].max(axis=1) >= 1.1 - 1e-6)   # "frustum": the box culls nothing
    causes = np.argmax(r[:, 6:] >= 1.1 - 1e-6, axis=1)
    assert set(causes.tolist()) == {0, 1} and np.isinf(r[:, 8]).sum() >= len(r) // 5 - 1   # x, y (behind: all three)


def test_clouds_share_their_uniforms(ws, oracle):
    """Every pattern and size of one (variant, viewport, layout) is seen through the same uniforms."""
    for variant in ("clip", "frustum"):
        ref = None
        for name, n in (("random_50", N_BIG), ("all", 1), ("lane63", 4097)):
            cl = kp.cloud(ws, name, n, "uncompressed", variant, (640, 480))
            cu, rs = cl.uniforms(oracle)
            both = bytes(cu) + bytes(rs)
            assert ref is None or both == ref
            ref = both


# ---- 3. the checker is sensitive -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_frame(ws, oracle):
    cl = kp.cloud(ws, "random_50", 4097, "uncompressed", "clip", (640, 480))
    fr = cl.oracle_frame(oracle)
    assert fr["num_visible"] > 1500
    from test_gpu_aux import _numpy_z   # the z plane's reference and bound, as the GPU test uses them
    cu, _ = cl.uniforms(oracle)
    fr["z"], fr["z_tol"] = _numpy_z(list(cu.view), cl.xyz[fr["src_index"]])
    assert len(np.unique(fr["z"])) > 1000
    for a in fr.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return fr


def _copy(fr):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}


def _swap_slots(fr, a, b):
    """What a compactor that stores survivors a and b at each other's slots leaves: every per-slot array swapped."""
    for k in ("splats", "keys", "src_index", "z"):
        fr[k][[a, b]] = fr[k][[b, a]]


def _corrupt(fr, how):
    fr = _copy(fr)
    v = fr["num_visible"]
    if how == "swap_adjacent":
        _swap_slots(fr, 700, 701)
    elif how == "swap_waves":              # the survivors of two waves of 64 lanes change places
        for k in ("splats", "keys", "src_index", "z"):
            a, b = fr[k][640:704].copy(), fr[k][704:768].copy()
            fr[k][640:704], fr[k][704:768] = b, a
    elif how == "drop_last":
        for k in ("splats", "keys", "src_index", "z"):
            fr[k] = fr[k][:v - 1]
        fr["sorted"] = fr["sorted"][fr["sorted"] != v - 1]
        fr["num_visible"] = v - 1
    elif how == "duplicate_slot":          # slot 901 holds what slot 900 holds
        for k in ("splats", "keys", "src_index", "z"):
            fr[k][901] = fr[k][900]
    elif how == "src_index_shift":
        fr["src_index"] = fr["src_index"] + 1
    elif how == "z_shift":                 # slot s's z stored at s + 1
        fr["z"] = np.roll(fr["z"], 1)
    elif how == "bit_flip":                # the low bit of one half (a colour: not NaN, not at a binade edge that matters)
        h = fr["splats"].view(np.uint16).reshape(-1, 10)
        h[1234, 7] ^= 1
    else:
        raise KeyError(how)
    return fr


CORRUPTIONS = ["swap_adjacent", "swap_waves", "drop_last", "duplicate_slot", "src_index_shift", "z_shift", "bit_flip"]


def test_checker_accepts_the_frame_itself(oracle_frame):
    for mode in ("bitwise", "oracle"):
        tally = {}
        assert kp.compare_frame(_copy(oracle_frame), oracle_frame, mode, tally=tally) == []
        if mode == "oracle":
            assert tally["halves"] == 10 * oracle_frame["num_visible"] and tally["keys"] == oracle_frame["num_visible"]
            assert tally["halves_inexact"] == tally["keys_inexact"] == tally["key_max"] == 0


@pytest.mark.parametrize("how", CORRUPTIONS)
def test_checker_reports_every_corruption(oracle_frame, how):
    bad = _corrupt(oracle_frame, how)
    assert kp.compare_frame(bad, oracle_frame, "bitwise"), how
    tally = {}
    diffs = kp.compare_frame(bad, oracle_frame, "oracle", tally=tally)
    if how == "bit_flip":     # one ulp of one half: inside the oracle bound, and counted for the pooled cap
        assert diffs == [] and tally["halves_inexact"] == 1
    else:
        assert diffs, how
    if how == "z_shift":      # nothing but the z plane is wrong
        assert all(d.startswith("z ") for d in diffs), diffs
