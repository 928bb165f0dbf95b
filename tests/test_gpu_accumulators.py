"""The lifecycle the three per-Gaussian accumulators share (include/websplat.h: ws_contrib, ws_grad, ws_shgrad): create, download,
add, reset, the refusals and close -- through Contrib, Grad and ShGrad, and for the refusals through the library itself.  No frame
is rendered and no cloud is created: what a frame adds is the subject of test_gpu_contrib / test_gpu_gradient / test_gpu_sh_gradient.

Every expectation is integer or bit equality computed in numpy.  The sizes: one Gaussian; one block of the merge kernels (256
threads in k_grad_merge and in k_contrib_merge) and one more; and, where a Gaussian has C words, the N at which N x C reaches 256
words and the next one (k_grad_merge walks words, not Gaussians)."""
import ctypes as C

import numpy as np
import pytest

from websplat import _lib as L

pytestmark = pytest.mark.gpu

BLOCK = 256
_u64p, _i64p, _f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_float)

# Word k of an array is SUMS_x[k % 8] + (k // 8 << 34) (the second term keeps the words of a long array distinct and touches no
# low word).  Word 0 is the only one an accumulator of one Gaussian and one word has: low word 0xFFFFFFFF under a value above 2^32,
# and B's 1 carries across bit 32.  The others: negatives, a carry into a negative's high word, a sum that changes sign, zeros.
SUMS_A = [(5 << 32) | 0xFFFFFFFF, -1, 0xFFFFFFFF, -(1 << 32) - 1, 1 << 40, -(3 << 33), 0, (7 << 32) | 0x80000000]
SUMS_B = [1, -0xFFFFFFFF, 1, 2, -(1 << 41), (3 << 33) + 1, 0, 0x80000000]
# ... and Contrib's largest weights: both sides win, 0.0 stays 0.0, a denormal beats 0.0 and loses to a larger denormal
DENORMAL = np.array([1], dtype=np.uint32).view(np.float32)[0]
MAX_A = np.array([0.0, DENORMAL, 1.0, 0.5, 0.0, 0.25], dtype=np.float32)
MAX_B = np.array([1.0, 0.0, DENORMAL, 0.75, 0.0, DENORMAL * 2], dtype=np.float32)


def _words(pattern, shape, dtype):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    w = np.array(pattern, dtype=np.int64)[k % len(pattern)] + ((k // len(pattern)) << 34)
    return w.reshape(shape).astype(dtype)   # (int64 -> uint64 keeps the bits)


def _maxima(pattern, n):
    return pattern[np.arange(n) % len(pattern)].copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


class _Contrib:
    prefix, args, words = "ws_contrib", (), 1
    parts = ("sum", "max")

    @staticmethod
    def make(ws, ctx, n):
        return ws.Contrib(ctx, n)

    @staticmethod
    def values(n, which):
        return {"sum": _words(SUMS_A if which == "A" else SUMS_B, (n,), np.uint64), "max": _maxima(MAX_A if which == "A" else MAX_B, n)}

    @staticmethod
    def download(acc):
        s, q, m = acc.download()
        assert s.dtype == np.float64 and np.array_equal(s, q.astype(np.float64) / L.WS_CONTRIB_SUM_SCALE)
        return {"sum": q, "max": m}

    @staticmethod
    def add(acc, parts):
        acc.add(parts.get("sum"), parts.get("max"))

    @staticmethod
    def merged(a, b):
        return {"sum": a["sum"] + b["sum"], "max": np.maximum(a["max"], b["max"])}

    @staticmethod
    def lib_download(h, capacity, n):
        q, m = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.float32)
        return L.lib.ws_contrib_download(h, capacity, q.ctypes.data_as(_u64p), m.ctypes.data_as(_f32p))

    @staticmethod
    def lib_download_nothing(h):
        return L.lib.ws_contrib_download(h, 0, None, None)

    @staticmethod
    def lib_add(h, count, n, nothing=False):
        q, m = np.ones(n, dtype=np.uint64), np.ones(n, dtype=np.float32)
        if nothing:
            return L.lib.ws_contrib_add(h, None, None, count)
        return L.lib.ws_contrib_add(h, q.ctypes.data_as(_u64p), m.ctypes.data_as(_f32p), count)


class _Grad:
    prefix, args, words = "ws_grad", (), L.WS_GRAD_CHANNELS
    parts = ("q",)

    @staticmethod
    def make(ws, ctx, n):
        return ws.Grad(ctx, n)

    @staticmethod
    def values(n, which):
        return {"q": _words(SUMS_A if which == "A" else SUMS_B, (n, L.WS_GRAD_CHANNELS), np.int64)}

    @staticmethod
    def download(acc):
        return {"q": acc.download()}

    @staticmethod
    def add(acc, parts):
        acc.add(parts["q"])

    @staticmethod
    def merged(a, b):
        return {"q": a["q"] + b["q"]}

    @staticmethod
    def lib_download(h, capacity, n):
        q = np.empty((n, L.WS_GRAD_CHANNELS), dtype=np.int64)
        return L.lib.ws_grad_download(h, capacity, q.ctypes.data_as(_i64p))

    @staticmethod
    def lib_download_nothing(h):
        return L.lib.ws_grad_download(h, 0, None)

    @staticmethod
    def lib_add(h, count, n, nothing=False):
        q = np.ones((n, L.WS_GRAD_CHANNELS), dtype=np.int64)
        return L.lib.ws_grad_add(h, None if nothing else q.ctypes.data_as(_i64p), count)


def _shgrad(sh_deg):
    ncoef = (sh_deg + 1) ** 2

    class _ShGrad:
        prefix, args, words = "ws_shgrad", (sh_deg,), 3 * ncoef + 1
        parts = ("sh", "opacity")

        @staticmethod
        def make(ws, ctx, n):
            return ws.ShGrad(ctx, n, sh_deg)

        @staticmethod
        def values(n, which):
            # one pattern over a Gaussian's 3 ncoef + 1 words, so that the two arrays differ wherever a transpose could confuse them
            w = _words(SUMS_A if which == "A" else SUMS_B, (n, 3 * ncoef + 1), np.int64)
            return {"sh": np.ascontiguousarray(w[:, :-1]).reshape(n, ncoef, 3), "opacity": np.ascontiguousarray(w[:, -1])}

        @staticmethod
        def download(acc):
            assert acc.sh_deg == sh_deg
            return acc.download()

        @staticmethod
        def add(acc, parts):
            acc.add(**parts)

        @staticmethod
        def merged(a, b):
            return {"sh": a["sh"] + b["sh"], "opacity": a["opacity"] + b["opacity"]}

        @staticmethod
        def lib_download(h, capacity, n):
            sh, o = np.empty((n, ncoef, 3), dtype=np.int64), np.empty(n, dtype=np.int64)
            return L.lib.ws_shgrad_download(h, capacity, sh.ctypes.data_as(_i64p), o.ctypes.data_as(_i64p))

        @staticmethod
        def lib_download_nothing(h):
            return L.lib.ws_shgrad_download(h, 0, None, None)

        @staticmethod
        def lib_add(h, count, n, nothing=False):
            sh, o = np.ones((n, ncoef, 3), dtype=np.int64), np.ones(n, dtype=np.int64)
            if nothing:
                return L.lib.ws_shgrad_add(h, None, None, count)
            return L.lib.ws_shgrad_add(h, sh.ctypes.data_as(_i64p), o.ctypes.data_as(_i64p), count)

    return _ShGrad


KINDS = {"contrib": _Contrib, "grad": _Grad, "shgrad0": _shgrad(0), "shgrad2": _shgrad(2)}


def _sizes(words):
    ns = {1, BLOCK, BLOCK + 1}
    if words > 1:   # the largest N whose words fit one block of k_grad_merge (28 words at degree 2: 252 of 256), and the next
        ns |= {BLOCK // words, BLOCK // words + 1}
    return sorted(ns)


CASES = [pytest.param(name, n, id=f"{name}-{n}") for name, kind in KINDS.items() for n in _sizes(kind.words)]


def _same(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        bad = np.argwhere(_bits(got[name]) != _bits(want[name]))
        assert bad.size == 0, f"{name}: {bad.shape[0]} values differ, first at {bad[0]}: {got[name][tuple(bad[0])]!r} != {want[name][tuple(bad[0])]!r}"


def _zeros(kind, n):
    return {name: np.zeros_like(a) for name, a in kind.values(n, "A").items()}


def _refused(rc, text):
    assert rc == L.WS_ERR_INVALID, rc
    assert L.lib.ws_last_error().decode() == text


@pytest.mark.parametrize("name,n", CASES)
def test_lifecycle(ws, ctx, name, n):
    kind = KINDS[name]
    a, b = kind.values(n, "A"), kind.values(n, "B")
    acc = kind.make(ws, ctx, n)
    try:
        # ---- fresh
        assert acc.num_points() == n and acc.frames == 0
        _same(kind.download(acc), _zeros(kind, n))
        # ---- add, add again
        kind.add(acc, a)
        _same(kind.download(acc), a)
        kind.add(acc, b)
        ab = kind.merged(a, b)
        _same(kind.download(acc), ab)
        assert acc.frames == 0 and acc.num_points() == n   # (a merge is no frame)
        # ---- a partial add leaves the other array; an add with nothing is none
        if len(kind.parts) == 2:
            first, second = kind.parts
            want = dict(ab)
            kind.add(acc, {first: b[first]})
            want[first] = kind.merged(ab, b)[first]
            _same(kind.download(acc), want)
            kind.add(acc, {second: a[second]})
            want[second] = kind.merged(ab, a)[second]
            _same(kind.download(acc), want)
            kind.add(acc, {})
            _same(kind.download(acc), want)
        else:
            want = ab
        assert kind.lib_add(acc.handle, n, n, nothing=True) == L.WS_OK
        _same(kind.download(acc), want)
        # ---- refusals leave the sums alone; the texts are the entry point's own
        _refused(kind.lib_download(acc.handle, n - 1, n), f"{kind.prefix}_download: capacity smaller than the number of points")
        _refused(kind.lib_add(acc.handle, n - 1, n), f"{kind.prefix}_add: fewer values than the accumulator has points")
        _refused(kind.lib_add(acc.handle, n - 1, n, nothing=True), f"{kind.prefix}_add: fewer values than the accumulator has points")
        assert kind.lib_download_nothing(acc.handle) == L.WS_OK   # (no array: no capacity to judge, the wait alone)
        _same(kind.download(acc), want)
        # ---- reset, and on
        acc.reset()
        assert acc.frames == 0 and acc.num_points() == n
        _same(kind.download(acc), _zeros(kind, n))
        kind.add(acc, a)
        _same(kind.download(acc), a)
    finally:
        acc.close()
    acc.close()
    assert not acc.handle


@pytest.mark.parametrize("name", list(KINDS))
def test_null_handles_and_creation(ws, ctx, name):
    kind, lib, p = KINDS[name], L.lib, KINDS[name].prefix
    _refused(getattr(lib, p + "_reset")(None, None), f"{p}_reset: null accumulator")
    _refused(kind.lib_download(None, 4, 4), f"{p}_download: null accumulator")
    _refused(kind.lib_download_nothing(None), f"{p}_download: null accumulator")
    _refused(kind.lib_add(None, 4, 4), f"{p}_add: null accumulator")
    _refused(kind.lib_add(None, 4, 4, nothing=True), f"{p}_add: null accumulator")
    assert getattr(lib, p + "_num_points")(None) == 0 and getattr(lib, p + "_frames")(None) == 0
    getattr(lib, p + "_destroy")(None)
    create, h = getattr(lib, p + "_create"), C.c_void_p()
    _refused(create(None, 4, *kind.args, C.byref(h)), f"{p}_create: null argument")
    _refused(create(ctx.handle, 4, *kind.args, None), f"{p}_create: null argument")
    _refused(create(ctx.handle, 0, *kind.args, C.byref(h)), f"{p}_create: no points")
    assert not h.value
    if kind.args:
        assert create(ctx.handle, 4, 4, C.byref(h)) == L.WS_ERR_UNSUPPORTED and not h.value
        assert lib.ws_last_error().decode() == "ws_shgrad_create: sh_deg > 3"
        _refused(create(ctx.handle, 0, 4, C.byref(h)), "ws_shgrad_create: no points")   # (the count is judged before the degree)
