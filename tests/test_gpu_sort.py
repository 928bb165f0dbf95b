"""GPU parity of the radix sort against the contract of GPURSSorter (gpu_rs.rs:865-884): ascending,
stable, (u32, u32) pairs, count optionally read from device memory.  Bit-exact."""
import os

import numpy as np
import pytest

from depth_fold_cases import CASES, FF, FF_TILE_CASES, fold_reference, hostile_keys
from variants import env_param, exp_param  # noqa: F401

pytestmark = pytest.mark.gpu


def _context(ws, env):
    """a context created under the WS_* switches `env` (the process environment is restored at once)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ws.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=["generic", "depth", "depth_noskip", "depth9", "depth9k8",
                                        exp_param("depth:onesweep", id="depth_fat_onesweep"), exp_param("depth:coop", id="depth_fat_coop")],
                ids=lambda p: {"generic": "reduce_scan", "depth": "depth_scan_companion", "depth_noskip": "depth_noskip",
                               "depth9": "depth_9bit_digits", "depth9k8": "depth_9bit_digits_2048_tiles"}.get(p))
def sort_ctx(ws, request):
    """Four paths to the same contract: the generic sorter (per-tile histograms -> column scan -> scatter), and the
    renderer's depth sorts behind ws_sorter_sort_depth -- the generic sorter carrying a companion value in the frame's form
    (the key-range fold: passes 1..3 over key - base, the fourth skipped on a narrow range) at 8 and 9 bits, and with the fold
    off (WS_DEPTH_SKIP_TOP=0: four plain passes); and the fat-tile one-sweep (round 4) as per-pass launches and as ONE launch
    with device-wide barriers (WS_DEPTH_SORT selects; inputs beyond the fat form's 2 M pairs take the generic sorter)."""
    depth = request.param != "generic"
    env = {"WS_DEPTH_DIGIT_BITS": "8", "WS_DEPTH_TILE_KPT": "0", "WS_DEPTH_SKIP_TOP": "1"}
    if depth and ":" in request.param:
        env["WS_DEPTH_SORT"] = request.param.split(":")[1]
    if request.param == "depth_noskip":
        env["WS_DEPTH_SKIP_TOP"] = "0"
    if request.param.startswith("depth9"):   # round 6: 9-bit digits (k_dsort9_*), at both tile sizes
        env["WS_DEPTH_DIGIT_BITS"] = "9"
        env["WS_DEPTH_TILE_KPT"] = "8" if request.param.endswith("k8") else "4"
    c = _context(ws, env)
    c.depth_mode = depth
    # the radix of the fold the sort reports (ws_sorter_depth_range); None: no fold to check -- four plain passes (depth_noskip:
    # the read-back must refuse) or the fat-tile one-sweep (it hands only the inputs beyond its capacity to the folded sort)
    c.fold_digits = {"depth": 256, "depth9": 512, "depth9k8": 512}.get(request.param)
    c.fold_absent = request.param == "depth_noskip"
    yield c
    c.close()


def test_sort_known_answer(sort_ctx):
    """The reference's own start-up self test: 8192 reversed f32 keys (gpu_rs.rs:295-331)."""
    assert sort_ctx.sort_selftest()


def _check(ws, ctx, oracle, keys, count=None):
    n = len(keys)
    m = n if count is None else min(count, n)
    sorter = ws.GPURSSorter(ctx, max(n, 1))
    try:
        if getattr(ctx, "depth_mode", False):  # a companion value rides along: must arrive with its pair
            aux_in = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5BD1E995)
            k, p, ax = sorter.sort_host(keys, np.arange(n, dtype=np.uint32), count=count, depth=True, aux=aux_in)
            assert np.array_equal(ax[:m], aux_in[p[:m]]), "companion values separated from their pairs"
            assert np.array_equal(ax[m:], aux_in[m:])
            if getattr(ctx, "fold_digits", None):  # what the device decided from keys[:count]: base, skip, span class
                assert sorter.depth_range() == fold_reference(keys[:m], ctx.fold_digits), "key-range fold differs from the reference"
            elif getattr(ctx, "fold_absent", False):
                with pytest.raises(ws.WebSplatError):
                    sorter.depth_range()
        else:
            k, p = sorter.sort_host(keys, np.arange(n, dtype=np.uint32), count=count)
    finally:
        sorter.close()
    ok, op = oracle.sort_pairs(keys[:m], np.arange(m, dtype=np.uint32))
    assert np.array_equal(k[:m], ok), "keys differ from the stable reference sort"
    assert np.array_equal(p[:m], op), "payload differs (stability or permutation broken)"
    if m < n:  # elements past the device-side count are never touched
        assert np.array_equal(k[m:], keys[m:])
        assert np.array_equal(p[m:], np.arange(m, n, dtype=np.uint32))


SIZES = [1, 2, 63, 64, 65, 255, 256, 1023, 1024, 1025, 3840, 4095, 4096, 4097, 8192, 12289, 100_000, 131_072, 131_073, 524_288,
         524_289, 1_000_003, 1_048_576, 1_048_577, 2_097_152, 2_097_153]


@pytest.mark.parametrize("n", SIZES)
def test_sort_random_u32(ws, sort_ctx, oracle, n):
    rng = np.random.default_rng(n)
    _check(ws, sort_ctx, oracle, rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("kind", ["all_equal", "two_values", "few_distinct", "sorted", "reversed", "all_ones",
                                  "depth_like", "low_byte_only", "high_byte_only"])
def test_sort_distributions(ws, sort_ctx, oracle, kind):
    n = 200_003
    rng = np.random.default_rng(7)
    if kind == "all_equal":
        keys = np.full(n, 0x3F800000, dtype=np.uint32)
    elif kind == "two_values":
        keys = rng.integers(0, 2, size=n).astype(np.uint32) * 0x01000000
    elif kind == "few_distinct":
        keys = rng.integers(0, 17, size=n).astype(np.uint32) * 0x00010203
    elif kind == "sorted":
        keys = np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    elif kind == "reversed":
        keys = np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))[::-1].copy()
    elif kind == "all_ones":
        keys = np.full(n, 0xFFFFFFFF, dtype=np.uint32)  # same bit pattern as the padding keys
    elif kind == "depth_like":
        keys = (rng.uniform(0.0, 37.5, size=n).astype(np.float32)).view(np.uint32)  # bits of zfar - z
    elif kind == "low_byte_only":
        keys = rng.integers(0, 256, size=n).astype(np.uint32)
    else:
        keys = rng.integers(0, 256, size=n).astype(np.uint32) << 24
    _check(ws, sort_ctx, oracle, keys)


@pytest.mark.parametrize("n,count", [(10_000, 0), (10_000, 1), (10_000, 4096), (10_000, 4097), (10_000, 9_999),
                                     (10_000, 10_000), (10_000, 50_000)])
def test_sort_device_side_count(ws, sort_ctx, oracle, n, count):
    """record_sort_indirect: the number of keys lives in device memory (gpu_rs.rs:875-884)."""
    rng = np.random.default_rng(count)
    _check(ws, sort_ctx, oracle, rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), count=count)


def test_sort_large_sortedness(ws, sort_ctx):
    """Full-size property check (C3: 5 M keys): sortedness, permutation, stability -- no oracle involved."""
    n = 5_000_000
    rng = np.random.default_rng(99)
    keys = rng.uniform(0.0, 20.0, size=n).astype(np.float32).view(np.uint32)
    keys[::7] = keys[0]  # plenty of duplicates to exercise stability
    sorter = ws.GPURSSorter(sort_ctx, n)
    try:
        k, p = sorter.sort_host(keys, np.arange(n, dtype=np.uint32), depth=getattr(sort_ctx, "depth_mode", False))
    finally:
        sorter.close()
    assert np.all(k[1:] >= k[:-1])
    assert np.array_equal(keys[p], k)
    seen = np.zeros(n, dtype=bool)
    seen[p] = True
    assert seen.all()
    ties = k[1:] == k[:-1]
    assert np.all(p[1:][ties] > p[:-1][ties])


@pytest.mark.parametrize("digit_bits", ["8", "9"])
@pytest.mark.parametrize("nbits", [0, 1, 5, 12, 13, 20, 26, 27, 28, 30, 31, 32])
def test_depth_sort_key_ranges(ws, oracle, nbits, digit_bits, monkeypatch):
    """Keys confined to a range of nbits bits that starts anywhere (a frame's depth keys are: bits of zfar - z), from a
    single value to the full 32 bits: passes whose digit is the same for every key are the degenerate case of every
    histogram and scan in the sorter.  The sort folds the key range as a frame's does; the decision it reports shows the rows
    up to 24 (8-bit) / 27 (9-bit) bits above the base sorted by three passes, the others by four."""
    n = 300_001
    rng = np.random.default_rng(1000 + nbits)
    span = (1 << nbits) - 1 if nbits else 0
    base = 0 if nbits >= 32 else int(rng.integers(0, (1 << 32) - span))
    keys = (base + rng.integers(0, span + 1, size=n, dtype=np.uint64)).astype(np.uint32)
    if nbits:
        keys[0], keys[1] = np.uint32(base), np.uint32(base + span)   # the range is exactly nbits wide
    monkeypatch.setenv("WS_DEPTH_DIGIT_BITS", digit_bits)
    ctx = ws.Context(0)
    sorter = ws.GPURSSorter(ctx, n)
    try:
        k, p = sorter.sort_host(keys, np.arange(n, dtype=np.uint32), depth=True)
        fold = sorter.depth_range()
    finally:
        sorter.close()
        ctx.close()
    ok, op = oracle.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    assert np.array_equal(k, ok) and np.array_equal(p, op)
    assert fold == fold_reference(keys, 1 << int(digit_bits))


@pytest.fixture(scope="module", params=["8", "9k4", "9k8"], ids=["8bit", "9bit_1024_tiles", "9bit_2048_tiles"])
def fold_ctx(ws, request):
    """The renderer's folded depth sort behind ws_sorter_sort_depth: 8-bit digits, and 9-bit digits over 1024-key tiles (up to
    SORT_SMALL_MAX keys, 2048 beyond) and 2048-key tiles."""
    nine = request.param != "8"
    c = _context(ws, {"WS_DEPTH_DIGIT_BITS": "9" if nine else "8", "WS_DEPTH_TILE_KPT": request.param[-1] if nine else "0",
                      "WS_DEPTH_SKIP_TOP": "1"})
    c.digits = 512 if nine else 256
    yield c
    c.close()


SMALL_MAX = 2_097_152  # ws_internal.h SORT_SMALL_MAX: where the 8-bit form's tile (and the 9-bit form's at 4 keys per thread) grows
FOLD_BIG = ("ff_tile_middle", "ff_tile_last", "span_below", "span_at")
FOLD_PARAMS = ([(c, n, cm) for c in CASES for n in (8192, 12_289) for cm in ("all", "count_stale0", "count_staleff")] +
               [(c, n, cm) for c in FOLD_BIG for n in (SMALL_MAX, SMALL_MAX + 1) for cm in ("all", "count_staleff")])


@pytest.mark.parametrize("case,n,count_mode", FOLD_PARAMS)
def test_depth_sort_range_fold(ws, oracle, fold_ctx, case, n, count_mode):
    """The depth sort's key-range fold on hostile keys (tests/depth_fold_cases.py): a whole 2048-aligned tile of 0xFFFFFFFF
    among keys that span < 2^20 (first, middle, partial last tile), scattered 0xFFFFFFFF, a maximum of 0xFFFFFFFE, only
    0xFFFFFFFF, minima at the digit edges, max - base at radix^3 - 1 and at radix^3, NaN bit patterns -- at tile multiples and
    at SORT_SMALL_MAX / + 1, with the count in device memory below n and stale keys of 0 / 0xFFFFFFFF past it, which must not
    move the decision (the renderer's key buffer holds stale keys past num_visible).  (a) keys and payload are the stable
    reference sort's, the companion stays with its pair, nothing past the count is touched; (b) the decision read back from
    the device is the Python-integer reference's on keys[:count]; (c) so the fourth pass is skipped exactly where the reference
    says, and there the result came through three passes and the copy back."""
    count = n if count_mode == "all" else n - 1500
    keys = hostile_keys(case, count, fold_ctx.digits, seed=n)
    if count < n:
        keys = np.concatenate([keys, np.full(n - count, 0 if count_mode == "count_stale0" else FF, dtype=np.uint32)])
    aux_in = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5BD1E995)
    sorter = ws.GPURSSorter(fold_ctx, n)
    try:
        k, p, ax = sorter.sort_host(keys, np.arange(n, dtype=np.uint32), count=None if count_mode == "all" else count, depth=True,
                                    aux=aux_in)
        fold = sorter.depth_range()
    finally:
        sorter.close()
    ok, op = oracle.sort_pairs(keys[:count], np.arange(count, dtype=np.uint32))
    assert np.array_equal(k[:count], ok), "keys differ from the stable reference sort"
    assert np.array_equal(p[:count], op), "payload differs (stability or permutation broken)"
    assert np.array_equal(ax[:count], aux_in[p[:count]]), "companion values separated from their pairs"
    assert np.array_equal(k[count:], keys[count:]) and np.array_equal(p[count:], np.arange(count, n, dtype=np.uint32))
    assert np.array_equal(ax[count:], aux_in[count:])
    want = fold_reference(keys[:count], fold_ctx.digits)
    assert fold == want, f"device fold {fold} != reference {want}"
    # (c) both outcomes of the skip are reached: the cases that hold a 0xFFFFFFFF or span radix^3 run four passes, the others three
    if case in FF_TILE_CASES or case in ("ff_scattered", "all_ff", "span_at", "nan_mix"):
        assert fold[1] == 0
    else:
        assert fold[1] == 1
