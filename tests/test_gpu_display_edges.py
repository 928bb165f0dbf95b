"""ws_display_composite (k_display, raster.hip) and ws_download_texture_rgba8 (drivers.cpp) on the hostile images of
tests/display_images.py: NaN, +-inf, negative colours, alpha outside [0, 1], every code of an rgba8unorm source, the 64 x 4
workgroup edges, padded source and destination pitches.

  exact class     byte for byte against the f32 restatement (a fused and an unfused c + background * k agree there)
  general class   against float64: exact where the value is decided, within 1 elsewhere (display_images.py derives the margin;
                  tests/test_display_images.py holds the undecided share under 1 %)
  read-back       clamp with NaN -> 0, * 255, truncation: byte for byte, rgba8unorm copied
  padding         source rows end in 0xFF bytes (NaN in f16 and f32) that must not be read into a pixel; destination rows end in
                  0xA5 bytes that must come back untouched

Raw device pointers through ctx.malloc / ctx.upload, as tests/test_gpu_metrics.py's _Dev.  Every case is one launch on at most
129 x 9 pixels."""
import ctypes as C

import numpy as np
import pytest

import display_images as di
from websplat import _lib as L

pytestmark = pytest.mark.gpu

CASES = [(w, h, fmt) for (w, h) in di.SIZES for fmt in di.SOURCES]
IDS = [f"{w}x{h}-{fmt}" for w, h, fmt in CASES]
FORMAT = {"rgba8unorm": L.WS_FORMAT_RGBA8_UNORM, "rgba16float": L.WS_FORMAT_RGBA16_FLOAT, "rgba32float": L.WS_FORMAT_RGBA32_FLOAT}
SURFACE = {"rgba8unorm": L.WS_SURFACE_RGBA8_UNORM, "bgra8unorm": L.WS_SURFACE_BGRA8_UNORM}


class _Dev:
    """one source image uploaded with padded rows, one padded destination; freed together"""

    def __init__(self, ws, ctx, img):
        self.ws, self.ctx, self.img = ws, ctx, img
        self.h, self.w = img.shape[:2]
        host = di.padded(img)
        self.src_pitch = host.shape[1]
        self.dst_pitch = self.w * 4 + di.DST_PAD
        self.fmt = FORMAT[{np.dtype(v): k for k, v in di.DTYPES.items()}[img.dtype]]
        self.src = ctx.malloc(host.nbytes)
        self.dst = None
        try:
            self.dst = ctx.malloc(self.h * self.dst_pitch)
            ctx.upload(self.src, host)
        except Exception:
            self.close()
            raise

    def display(self, background, surface):
        """H x W x 4 uint8 of the surface; asserts that the row padding of the destination came back untouched"""
        ws, ctx = self.ws, self.ctx
        ctx.upload(self.dst, np.full((self.h, self.dst_pitch), di.DST_FILL, np.uint8))
        bg = (C.c_float * 4)(*[float(x) for x in background])
        ws.check(ws.lib.ws_display_composite(ctx.handle, C.c_void_p(self.src), self.fmt, self.src_pitch, self.w, self.h, bg,
                                             SURFACE[surface], C.c_void_p(self.dst), self.dst_pitch, None))
        ctx.sync()
        got = ctx.download(self.dst, (self.h, self.dst_pitch), np.uint8)
        assert (got[:, self.w * 4:] == di.DST_FILL).all()
        return got[:, :self.w * 4].reshape(self.h, self.w, 4)

    def readback(self):
        out = np.full((self.h, self.w, 4), 0x5A, np.uint8)
        self.ws.check(self.ws.lib.ws_download_texture_rgba8(self.ctx.handle, C.c_void_p(self.src), self.fmt, self.w, self.h,
                                                            self.src_pitch, out.ctypes.data_as(C.c_void_p), None))
        return out

    def close(self):
        for p in (self.src, self.dst):
            if p:
                self.ctx.free(p)
        self.src = self.dst = None


def _where(bad, got, want, img):
    y, x, ch = np.argwhere(bad)[0].tolist()
    return f"{int(bad.sum())} values differ; first at x={x} y={y} channel={ch}: got {got[y, x, ch]}, want {want[y, x, ch]}, texel {img[y, x].tolist()}"


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_display_exact_class(ws, ctx, w, h, fmt):
    img = di.exact_image(w, h, fmt)
    dev = _Dev(ws, ctx, img)
    try:
        for surface in di.SURFACES:
            for bg in di.EXACT_BACKGROUNDS:
                got = dev.display(bg, surface)
                want = di.composite_f32(img, bg, surface)
                assert np.array_equal(got, want), (surface, bg, _where(got != want, got, want, img))
    finally:
        dev.close()


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_display_general_class(ws, ctx, w, h, fmt):
    for seed in (0, 1):
        img = di.general_image(w, h, fmt, seed)
        bg = di.general_background(seed)
        dev = _Dev(ws, ctx, img)
        try:
            for surface in di.SURFACES:
                got = dev.display(bg, surface)
                want, decided = di.composite_f64(img, bg, surface)
                d = np.abs(got.astype(np.int32) - want.astype(np.int32))
                print(f"{w}x{h} {fmt} {surface} seed {seed}: undecided {int((~decided).sum())} of {decided.size}, "
                      f"differing {int((d != 0).sum())}, of them decided {int(((d != 0) & decided).sum())}")
                bad = (d != 0) & decided
                assert not bad.any(), (surface, _where(bad, got, want, img))
                assert d.max() <= 1, (surface, _where(d > 1, got, want, img))
        finally:
            dev.close()


@pytest.mark.parametrize("w,h,fmt", CASES, ids=IDS)
def test_readback_of_hostile_images(ws, ctx, w, h, fmt):
    for img in (di.exact_image(w, h, fmt), di.general_image(w, h, fmt, 0)):
        dev = _Dev(ws, ctx, img)
        try:
            got = dev.readback()
            want = di.readback(img)
            assert np.array_equal(got, want), _where(got != want, got, want, img)
        finally:
            dev.close()
