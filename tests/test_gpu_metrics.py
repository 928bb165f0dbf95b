"""GPU tests of the image metrics (include/websplat.h "Image metrics"): k_image_metrics against the numpy
reference of tests/metrics_ref.py on every tile edge, every format pair, padded pitches, the zero-padded border, identical
inputs, reproducibility and the accumulator's behaviour.

Tolerances.  sse_u8 is exact.  mse: 1e-5 relative -- one rounding in d * d and a fixed-order sum of a few thousand non-negative
terms per workgroup bound the relative error by about 50 * 2^-24 = 3e-6; threefold margin.  SSIM mean and map: 8 x the
float32-against-float64 gap of metrics_ref on the same case (floors 1e-7 / 1e-6), never a figure taken from the kernel.
Each case's gap and the device's deviation go to metrics_parity.json in the directory WEBSPLAT_REPORT_DIR names (default:
test_reports/ under the repository root); profiles/metrics/metrics_parity.json is a committed copy of an MI355X run."""
import json
import os

import numpy as np
import pytest

import metrics_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = []

# every width of {1, 5, 11, 31, 32, 33, 63, 64, 65, 75} and every height of {1, 5, 16, 17, 33, 53} at least once: all tile edges
# of the 32 x 16 tile (and of any power-of-two tile up to 64), and images smaller than the 11-tap window
SHAPES = [(1, 1), (5, 5), (11, 16), (31, 17), (32, 33), (33, 17), (63, 53), (64, 16), (65, 33), (75, 53), (33, 1), (1, 53)]
assert {w for w, _ in SHAPES} == {1, 5, 11, 31, 32, 33, 63, 64, 65, 75} and {h for _, h in SHAPES} == {1, 5, 16, 17, 33, 53}
FORMAT_PAIRS = ["f32/f32", "f16/f16", "u8/u8", "f16bg/u8"]
DTYPES = {"f32": np.float32, "f16": np.float16, "u8": np.uint8}
NAMES = {np.dtype(np.float32): "rgba32float", np.dtype(np.float16): "rgba16float", np.dtype(np.uint8): "rgba8unorm"}


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    if PARITY:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "metrics_parity.json"), "w") as f:
            json.dump({"tolerance": "ssim: 8 x (ssim_f32 - ssim_f64 of tests/metrics_ref.py), floors 1e-7 mean / 1e-6 map; mse 1e-5 relative",
                       "cases": PARITY}, f, indent=1)


def _as(img, dtype):
    """float64 H x W x 4 in any range -> the dtype's image (uint8: rounded and clipped; floats keep values outside [0, 1])"""
    if dtype == np.uint8:
        return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
    return img.astype(dtype)


def _pair(w, h, seed, fa, fb, noise=0.05, flat=None):
    """uniform noise (or a flat value) against itself + N(0, noise), alpha included"""
    rng = np.random.default_rng(seed)
    a = rng.random((h, w, 4)) if flat is None else np.full((h, w, 4), flat)
    b = a + rng.normal(0.0, noise, a.shape)
    return _as(a, fa), _as(b, fb)


class _Dev:
    """images uploaded with a row padding of 0xFF bytes (NaN in f16 and f32), freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def view(self, ws, img, pad=0, background=None):
        h, w = img.shape[:2]
        row = w * 4 * img.itemsize
        host = np.full((h, row + pad), 0xFF, dtype=np.uint8)
        host[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
        p = self.ctx.malloc(host.nbytes)
        self.ptrs.append(p)
        self.ctx.upload(p, host)
        return ws.ImageView(p, NAMES[img.dtype], row + pad, background)

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


def _run(ws, ctx, a, b, bg_a=None, bg_b=None, pads=(16, 48), quantize=False):
    dev, m = _Dev(ctx), ws.Metrics(ctx, 1)
    try:
        h, w = a.shape[:2]
        m.add(dev.view(ws, a, pads[0], bg_a), dev.view(ws, b, pads[1], bg_b), w, h, quantize_u8=quantize, ssim_map=True)
        rec = m.download()[0]
        return rec, m.maps()[0]
    finally:
        m.close()
        dev.close()


def _check(name, rec, dmap, ref, quantize):
    tol_mean, tol_map = mr.tolerances(ref)
    dev_mean = abs(rec["ssim"] - ref["ssim"])
    dev_map = float(np.abs(dmap.astype(np.float64) - ref["map"]).max())
    rel_mse = abs(rec["mse"] - ref["mse"]) / ref["mse"] if ref["mse"] else abs(rec["mse"])
    PARITY.append({"case": name, "quantize_u8": bool(quantize), "width": ref["width"], "height": ref["height"],
                   "ref_gap_mean": ref["gap_mean"], "ref_gap_map": ref["gap_map"], "tol_mean": tol_mean, "tol_map": tol_map,
                   "device_dev_mean": dev_mean, "device_dev_map": dev_map, "mse_rel_dev": rel_mse, "ssim": rec["ssim"], "psnr": rec["psnr"]})
    print(f"{name} q={int(quantize)}: gap mean {ref['gap_mean']:.3e} map {ref['gap_map']:.3e} | device mean {dev_mean:.3e} "
          f"map {dev_map:.3e} | mse rel {rel_mse:.3e}")
    assert (rec["width"], rec["height"]) == (ref["width"], ref["height"])
    assert rec["flags"] == (1 if quantize else 0)
    if quantize:
        assert rec["sse_u8"] == ref["sse_u8"]
        assert rel_mse <= 1e-12
        if ref["mse"]:
            assert abs(rec["psnr"] - ref["psnr"]) <= 1e-12 * abs(ref["psnr"])
    else:
        assert rec["sse_u8"] == 0
        assert rel_mse <= 1e-5
    if ref["mse"] == 0:
        assert rec["mse"] == 0.0 and rec["psnr"] == float("inf")
    else:
        assert abs(rec["psnr"] - ref["psnr"]) <= 1e-4   # (follows from the mse bound: 10 / ln 10 * 1e-5)
    assert dev_mean <= tol_mean, (dev_mean, tol_mean)
    assert dmap.shape == ref["map"].shape and dev_map <= tol_map, (dev_map, tol_map)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_f32(ws, ctx, shape):
    w, h = shape
    a, b = _pair(w, h, 100 + w * 97 + h, np.float32, np.float32)
    for quantize in (False, True):
        rec, dmap = _run(ws, ctx, a, b, quantize=quantize)
        _check(f"noise f32/f32 {w}x{h}", rec, dmap, mr.reference(a, b, quantize=quantize), quantize)


@pytest.mark.parametrize("shape", [(33, 17), (75, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", FORMAT_PAIRS)
def test_format_pairs(ws, ctx, pair, shape):
    w, h = shape
    fa, fb = pair.split("/")
    bg = (0.25, 0.5, 0.75) if fa.endswith("bg") else None
    a, b = _pair(w, h, 7 + w, DTYPES[fa.replace("bg", "")], DTYPES[fb])
    if bg is not None:
        b[..., 3] = 255                                     # the opaque ground truth
        a[..., :3] *= a[..., 3:4]                           # a premultiplied render
    for quantize in (False, True):
        rec, dmap = _run(ws, ctx, a, b, bg_a=bg, pads=(32, 16), quantize=quantize)
        _check(f"noise {pair} {w}x{h}", rec, dmap, mr.reference(a, b, bg_a=bg, quantize=quantize), quantize)


def test_flat_low_noise(ws, ctx):
    """The cancellation worst case: a flat 0.9 image against itself + N(0, 0.002); gated at its own 8 x gap like the others."""
    a, b = _pair(75, 53, 5, np.float32, np.float32, noise=0.002, flat=0.9)
    ref = mr.reference(a, b)
    assert ref["gap_map"] > 1e-5        # (the case is what it is meant to be: float32 loses digits here)
    rec, dmap = _run(ws, ctx, a, b)
    _check("flat 0.9 + N(0, 0.002) f32/f32 75x53", rec, dmap, ref, False)


def test_nonfinite_and_out_of_range_values(ws, ctx):
    """NaN -> 0, +-inf and values outside [0, 1] are clamped, in colour and (over a background) through alpha."""
    a, b = _pair(33, 17, 9, np.float32, np.float16)
    a[2, 3, 0], a[4, 5, 1], a[6, 7, 2], a[8, 9, 3] = np.nan, np.inf, -np.inf, np.nan
    b[1, 1, 0], b[3, 30, 3] = np.nan, np.inf
    bg = (1.0, 0.5, 0.0)
    for quantize in (False, True):
        rec, dmap = _run(ws, ctx, a, b, bg_a=bg, bg_b=bg, quantize=quantize)
        _check("non-finite f32bg/f16bg 33x17", rec, dmap, mr.reference(a, b, bg_a=bg, bg_b=bg, quantize=quantize), quantize)


def test_border_zero_padding(ws, ctx):
    """40 x 40, constant 0.25 inside a one-pixel frame of 1.0, against the same without the frame: the map, pixel by pixel."""
    b = np.full((40, 40, 4), 0.25, dtype=np.float32)
    b[..., 3] = 1.0
    a = b.copy()
    a[0, :, :3] = a[-1, :, :3] = a[:, 0, :3] = a[:, -1, :3] = 1.0
    ref = mr.reference(a, b)
    rec, dmap = _run(ws, ctx, a, b)
    _check("border frame f32/f32 40x40", rec, dmap, ref, False)
    # the corner, an edge and the interior see the frame differently; a replicated or mirrored border would not
    assert ref["map"][0, 0] < ref["map"][0, 20] < ref["map"][20, 20] and abs(ref["map"][20, 20] - 1.0) < 1e-9
    tol = mr.tolerances(ref)[1]
    assert np.all(np.abs(dmap.astype(np.float64) - ref["map"]) <= tol)


@pytest.mark.parametrize("fmt", ["f32", "f16", "u8"])
def test_identical_inputs(ws, ctx, fmt):
    a, _ = _pair(65, 33, 3, DTYPES[fmt], DTYPES[fmt])
    for quantize in (False, True):
        rec, dmap = _run(ws, ctx, a, a.copy(), pads=(16, 32), quantize=quantize)
        assert rec["mse"] == 0.0 and rec["psnr"] == float("inf") and rec["sse_u8"] == 0
        assert abs(rec["ssim"] - 1.0) <= 1e-6 and np.all(np.abs(dmap - 1.0) <= 1e-6)


def _bits(rec):
    return tuple(np.float64(rec[k]).view(np.uint64) for k in ("mse", "psnr", "ssim")) + (rec["sse_u8"],)


def test_reproducible_and_order_independent(ws, ctx):
    """The same pair twice gives bit-equal doubles; another add order (and with it another slab history) changes no record."""
    pa = _pair(75, 53, 21, np.float16, np.float16)
    pb = _pair(33, 17, 22, np.float32, np.uint8)
    dev = _Dev(ctx)
    m1, m2 = ws.Metrics(ctx, 4), ws.Metrics(ctx, 4)
    try:
        va = (dev.view(ws, pa[0], 16), dev.view(ws, pa[1], 16), 75, 53)
        vb = (dev.view(ws, pb[0], 16), dev.view(ws, pb[1], 48), 33, 17)
        for v in (vb, va, vb, va):
            m1.add(*v)
        for v in (va, vb):
            m2.add(*v, quantize_u8=True)
            m2.add(*v)
        r1, r2 = m1.download(), m2.download()
        assert _bits(r1[0]) == _bits(r1[2]) == _bits(r2[3]) and _bits(r1[1]) == _bits(r1[3]) == _bits(r2[1])
        assert r1[0]["mse"] > 0 and r1[1]["mse"] > 0 and r2[0]["sse_u8"] > 0
    finally:
        m1.close()
        m2.close()
        dev.close()


def test_padded_and_tight_pitch_agree_bitwise(ws, ctx):
    a, b = _pair(63, 53, 31, np.float16, np.uint8)
    bg = (0.1, 0.2, 0.3)
    tight, mt = _run(ws, ctx, a, b, bg_a=bg, pads=(0, 0))
    padded, mp = _run(ws, ctx, a, b, bg_a=bg, pads=(48, 16))
    assert _bits(tight) == _bits(padded) and np.array_equal(mt.view(np.uint32), mp.view(np.uint32))


def test_accumulator_behaviour(ws, ctx):
    from websplat import _lib as L
    sizes = [(5, 5), (33, 17), (64, 16)]
    pairs = [_pair(w, h, 40 + i, np.float32, np.float32) for i, (w, h) in enumerate(sizes)]
    dev, m = _Dev(ctx), ws.Metrics(ctx, 3)
    try:
        views = [(dev.view(ws, a, 16), dev.view(ws, b, 16), a.shape[1], a.shape[0]) for a, b in pairs]
        assert m.count == 0 and m.download() == []
        for i, v in enumerate(views):
            m.add(*v, quantize_u8=(i == 1))
        assert m.count == 3
        recs = m.download()
        assert [(r["width"], r["height"], r["flags"]) for r in recs] == [(5, 5, 0), (33, 17, 1), (64, 16, 0)]
        for r, (a, b), q in zip(recs, pairs, (False, True, False)):
            ref = mr.reference(a, b, quantize=q)
            assert abs(r["mse"] - ref["mse"]) <= 1e-5 * ref["mse"] and abs(r["ssim"] - ref["ssim"]) <= mr.tolerances(ref)[0]
        # full: refused, and the earlier records stay
        with pytest.raises(ws.WebSplatError) as e:
            m.add(*views[0])
        assert e.value.code == L.WS_ERR_OVERFLOW and m.count == 3
        assert [_bits(r) for r in m.download()] == [_bits(r) for r in recs]
        # refused arguments add nothing
        va, vb, w, h = views[1]
        m.reset()
        assert m.count == 0 and m.download() == []
        for bad in (dict(a=ws.ImageView(va.ptr, va.format, w * 16 - 16), b=vb), dict(a=va, b=ws.ImageView(vb.ptr, "rgba32float", 8)),
                    dict(a=ws.ImageView(va.ptr + 4, va.format, va.pitch), b=vb), dict(a=ws.ImageView(0, va.format, va.pitch), b=vb)):
            with pytest.raises(ws.WebSplatError) as e:
                m.add(bad["a"], bad["b"], w, h)
            assert e.value.code == L.WS_ERR_INVALID
        with pytest.raises(ws.WebSplatError) as e:
            m.add(va, vb, 0, h)
        assert e.value.code == L.WS_ERR_INVALID
        ca, cb = va.to_c(), vb.to_c()
        import ctypes as C
        assert ws.lib.ws_metrics_add(m.handle, C.byref(ca), C.byref(cb), w, h, 2, None, 0, None) == L.WS_ERR_INVALID  # unknown flag bit
        buf = (L.ws_image_metrics * 1)()
        m.add(va, vb, w, h)
        m.add(va, vb, w, h)
        assert ws.lib.ws_metrics_download(m.handle, 1, buf, None) == L.WS_ERR_INVALID                                 # capacity < count
        again = m.download()
        assert len(again) == 2 and _bits(again[0]) == _bits(again[1])
    finally:
        m.close()
        dev.close()


def test_image_metrics_convenience(ws, ctx):
    a, b = _pair(31, 17, 51, np.float16, np.uint8)
    rec, dmap = ws.image_metrics(ctx, a, b, background_a=(0.0, 0.0, 0.0), quantize_u8=True, ssim_map=True)
    _check("image_metrics f16bg/u8 31x17", rec, dmap, mr.reference(a, b, bg_a=(0, 0, 0), quantize=True), True)
    assert ws.image_metrics(ctx, a, a)["psnr"] == float("inf")
