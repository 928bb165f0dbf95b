"""numpy reference of the image metrics (include/websplat.h "Image metrics").  No scipy.

  pixel_value   the bit-defined pixel value in float32 (decode, over a background, clamp, optional 8-bit quantisation)
  mse / psnr    d = x - y in float32, everything from d on in float64
  ssim_f64      the definition evaluated in float64 on the float32 pixel values, as a direct 11 x 11 window (not separably)
  ssim_f32      the same restated plainly in float32, the way a torch conv2d evaluation computes it

The gap between ssim_f32 and ssim_f64 on a case is the yardstick of the device's SSIM tolerance on that case (reference() reports it, tolerances() applies it).
"""
import numpy as np

F = np.float32
C1, C2 = 0.01 ** 2, 0.03 ** 2
# g[0..5] as websplat.h lists them; g[10 - k] = g[k]
WINDOW_HEX = ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c4p-3", "0x1.10656p-2")


def window():
    """The 11 taps: exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double, rounded to float32."""
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g32 = (g / g.sum()).astype(F)
    assert [float(v) for v in g32[:6]] == [float.fromhex(h) for h in WINDOW_HEX] and np.array_equal(g32, g32[::-1])
    return g32


def decode(img):
    """H x W x 4 uint8 / float16 / float32 -> float32, as ws_display_composite decodes."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(F) / F(255.0)
    assert img.dtype in (np.float16, np.float32)
    return img.astype(F)


def pixel_value(img, background=None, quantize=False):
    """(v, q): the H x W x 3 float32 pixel values and, with quantize, the uint8 codes they came from (else None)."""
    t = decode(img)
    v = t[..., :3]
    with np.errstate(invalid="ignore"):            # (non-finite texels are ordinary inputs)
        if background is not None:
            k = F(1.0) - t[..., 3:4]               # three separately rounded float32 operations
            tt = np.asarray(background, dtype=F)[:3] * k
            v = v + tt
        v = np.where(np.isnan(v), F(0.0), np.minimum(np.maximum(v, F(0.0)), F(1.0))).astype(F)
    q = None
    if quantize:
        q = (v * F(255.0)).astype(np.uint8)        # truncation
        v = q.astype(F) / F(255.0)
    return v, q


def mse(x, y):
    d = (x - y).astype(F)                          # float32
    e = d.astype(np.float64) ** 2
    return float(e.sum() / e.size)


def psnr(m):
    return float("inf") if m == 0 else float(-10.0 * np.log10(m))


def sse_u8(qx, qy):
    d = qx.astype(np.int64) - qy.astype(np.int64)
    return int((d * d).sum())


def _moments(x, y, dtype):
    """mu_x, mu_y, E[x^2], E[y^2], E[xy] of H x W x 3 images under the zero-padded 11 x 11 window, evaluated in `dtype`."""
    g = window().astype(dtype)
    w2 = np.outer(g, g).astype(dtype)              # (float64: exact products of the float32 taps)
    x, y = x.astype(dtype), y.astype(dtype)
    h, w = x.shape[:2]
    planes = [x, y, x * x, y * y, x * y]
    padded = [np.pad(p, ((5, 5), (5, 5), (0, 0))) for p in planes]
    out = [np.zeros_like(p) for p in planes]
    for i in range(11):
        for j in range(11):
            for o, p in zip(out, padded):
                o += w2[i, j] * p[i:i + h, j:j + w]
    return out


def _ssim(x, y, dtype):
    mx, my, xx, yy, xy = _moments(x, y, dtype)
    c1, c2, two = dtype(C1), dtype(C2), dtype(2.0)
    mx2, my2, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = xx - mx2, yy - my2, xy - mxy
    full = ((two * mxy + c1) * (two * sxy + c2)) / ((mx2 + my2 + c1) * (sx + sy + c2))
    pix = ((full[..., 0] + full[..., 1]) + full[..., 2]) / dtype(3.0)
    return full.mean(dtype=dtype), pix


def ssim_f64(x, y):
    """(mean over 3 W H, H x W map of the per-pixel mean of the three channel maps), float64."""
    m, pix = _ssim(x, y, np.float64)
    return float(m), pix


def ssim_f32(x, y):
    m, pix = _ssim(x, y, np.float32)
    return float(m), pix.astype(np.float64)


def reference(img_a, img_b, bg_a=None, bg_b=None, quantize=False):
    """Everything a record holds, plus the float32-against-float64 gaps of this case."""
    x, qx = pixel_value(img_a, bg_a, quantize)
    y, qy = pixel_value(img_b, bg_b, quantize)
    s64, map64 = ssim_f64(x, y)
    s32, map32 = ssim_f32(x, y)
    out = {"ssim": s64, "map": map64, "gap_mean": abs(s32 - s64), "gap_map": float(np.abs(map32 - map64).max()),
           "width": x.shape[1], "height": x.shape[0]}
    if quantize:
        out["sse_u8"] = sse_u8(qx, qy)
        out["mse"] = out["sse_u8"] / (255.0 ** 2 * x.size)
    else:
        out["sse_u8"] = 0
        out["mse"] = mse(x, y)
    out["psnr"] = psnr(out["mse"])
    return out


# SSIM tolerances: 8 x this file's own float32-against-float64 gap on the case, floors 1e-7 (mean) and 1e-6 (map)
def tolerances(ref):
    return max(8.0 * ref["gap_mean"], 1e-7), max(8.0 * ref["gap_map"], 1e-6)
