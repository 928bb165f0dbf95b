"""The depth sort's key-range fold (ws_internal.h depth_range_decide, depth_tile_reports): a plain Python-integer reference of
the decision, and the hostile key sets both the host twin (test_host.py) and the device sort (test_gpu_sort.py) are held to."""
import numpy as np

FF = 0xFFFFFFFF
NAN_BITS = (0x7FC00000, 0xFFC00000, FF)


def fold_reference(keys, digits):
    """(base, skip, span_class) from min and max of the keys, in Python integers: base = 0 when a key is 0xFFFFFFFF, else min
    with the first digit's bits cleared; skip iff max - base < digits^3 (three passes cover it); span class on the 8-bit base
    (1: < 2^24, 2: not).  (0, 0, 0) when no key lies below 0xFFFFFFFF -- max(~key) == 0: nothing known."""
    keys = np.asarray(keys, dtype=np.uint32)
    if keys.size == 0 or int(keys.min()) == FF:
        return 0, 0, 0
    lo, hi = int(keys.min()), int(keys.max())
    base = 0 if hi == FF else lo & ~(digits - 1)
    base8 = 0 if hi == FF else lo & ~255
    return base, int(hi - base < digits ** 3), 1 if hi - base8 < (1 << 24) else 2


def _band(rng, n, lo, width):
    """n keys in [lo, lo + width), both ends present (n >= 2)"""
    k = (lo + rng.integers(0, width, size=n, dtype=np.uint64)).astype(np.uint32)
    if n >= 2:
        k[0], k[-1] = np.uint32(lo), np.uint32(lo + width - 1)
    return k


# Named key sets.  FF_TILE_CASES put a whole sort tile of 0xFFFFFFFF among keys that span < 2^20: the reports the old rule
# (`if (knmin)`) dropped.  A run of 2048 keys at a multiple of 2048 is a whole tile at 1024 and at 2048 keys per tile.
FF_TILE_CASES = ("ff_tile_first", "ff_tile_middle", "ff_tile_last")
CASES = FF_TILE_CASES + ("ff_scattered", "max_fffffffe", "all_ff", "min_low_00", "min_low_ff", "min_low_1ff", "span_below",
                         "span_at", "nan_mix")


def hostile_keys(name, count, digits, seed=0, run=2048):
    """`count` keys of the named set; the ff_tile cases put their run of `run` keys at a multiple of `run` (count > 2 * run for
    them to mean what they say)."""
    rng = np.random.default_rng(seed)
    lo = 0x40A01234
    if name in FF_TILE_CASES:
        k = _band(rng, count, lo, 1 << 20)
        k[0] = k[-1] = np.uint32(lo + 7)  # (the band's ends elsewhere: the all-0xFFFFFFFF tile may sit at either end)
        k[count // 3] = np.uint32(lo)
        k[count // 3 + 1] = np.uint32(lo + (1 << 20) - 1)
        full = count // run
        t = {"ff_tile_first": 0, "ff_tile_middle": full // 2, "ff_tile_last": full}[name]
        if name == "ff_tile_last" and t * run == count:
            t -= 1
        if name == "ff_tile_middle" and (count // 3) // run == t:
            t += 1
        k[t * run:(t + 1) * run] = np.uint32(FF)
        return k
    if name == "ff_scattered":
        k = _band(rng, count, lo, 1 << 20)
        k[rng.choice(count, size=min(count, 5), replace=False)] = np.uint32(FF)
        return k
    if name == "max_fffffffe":
        return _band(rng, count, 0xFFFFFFFE - (1 << 20) + 1, 1 << 20)
    if name == "all_ff":
        return np.full(count, FF, dtype=np.uint32)
    if name == "min_low_00":
        return _band(rng, count, 0x3F123400, 1 << 16)
    if name == "min_low_ff":
        return _band(rng, count, 0x3F1234FF, 1 << 16)
    if name == "min_low_1ff":
        return _band(rng, count, 0x3F1235FF, 1 << 16)
    if name in ("span_below", "span_at"):
        base = 0x20000000 + 0x12345 * digits
        k = _band(rng, count, base + 3, 1 << 12)
        k[count // 2] = np.uint32(base + digits ** 3 - (1 if name == "span_below" else 0))
        return k
    if name == "nan_mix":
        k = rng.uniform(1.0, 30.0, size=count).astype(np.float32).view(np.uint32)
        k[rng.choice(count, size=min(count, 3), replace=False)] = np.array(NAN_BITS[:min(count, 3)], dtype=np.uint32)
        return k
    raise KeyError(name)


def random_keys(rng, count):
    """one key set of the property sweep: depth-like f32 bits, NaN patterns, negative-float bits, runs of 0xFFFFFFFF"""
    kind = int(rng.integers(0, 5))
    if kind == 0:  # bits of zfar - z: positive floats in a band of random width
        lo = float(rng.uniform(0.01, 100.0))
        k = rng.uniform(lo, lo * float(rng.uniform(1.0, 8.0)), size=count).astype(np.float32).view(np.uint32)
    elif kind == 1:  # negative-float bits (>= 0x80000000)
        k = (-rng.uniform(0.5, 50.0, size=count)).astype(np.float32).view(np.uint32)
    elif kind == 2:  # a narrow integer band anywhere in [0, 2^32)
        w = 1 << int(rng.integers(0, 29))
        lo = int(rng.integers(0, (1 << 32) - w))
        k = (lo + rng.integers(0, w, size=count, dtype=np.uint64)).astype(np.uint32)
    elif kind == 3:  # full-range keys
        k = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    else:  # positive and negative floats mixed
        k = rng.uniform(-20.0, 20.0, size=count).astype(np.float32).view(np.uint32)
    if count and rng.random() < 0.5:  # NaN patterns sprinkled
        m = int(rng.integers(1, 4))
        k[rng.integers(0, count, size=m)] = rng.choice(np.array(NAN_BITS, dtype=np.uint32), size=m)
    if count and rng.random() < 0.5:  # a run of 0xFFFFFFFF of random length and offset
        a = int(rng.integers(0, count))
        k[a:a + int(rng.integers(1, 5000))] = np.uint32(FF)
    return k
