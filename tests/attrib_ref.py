"""Float64 reference of the weighted contribution sums (include/websplat.h "Attributing a pixel plane to Gaussians"; contrib.h):
contrib_ref.contrib_f64 with the weight of every kept pair multiplied by E(p), E the float32 clamp result taken to float64.  The
transmittance, the kept pairs and the draw order do not see E.

Per source Gaussian j:
  sum[j], max[j]  sum and maximum of v = w E over its kept pairs
  kept[j], P[j], U[j]   as contrib_ref, counted over pixels with E > 0 only (a pair at a pixel with E == 0 is exactly 0 on the
                  device whatever its w: it needs no allowance)
  front[j]        (with `watch`) the largest transmittance in front of j's pairs over the watched pixels: where the device's
                  waves that own those pixels may have stopped

Tolerances: contrib_ref.bounds applied to this result.  Every term of that bound is a perturbation of w; v = w E with E <= 1
scales it down, and the one extra float32 rounding of the product (2^-24 relative) is inside the 1e-5 relative term.
"""
import numpy as np

import contrib_ref
import scenes

F = np.float32


def clamp_plane(plane, scale=1.0, bias=0.0):
    """E as the device forms it: fma(scale, plane, bias) in float32, clamped to [0, 1], NaN -> 0.  The fused multiply-add is
    taken in float64 and rounded once (the product of two float32 is exact there; with scale in {0, 1} or bias == 0, the cases
    the tests use, so is the sum)."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = (np.float64(F(scale)) * np.asarray(plane, dtype=F).astype(np.float64) + np.float64(F(bias))).astype(F)
        return np.where(np.isnan(e), F(0.0), np.minimum(np.maximum(e, F(0.0)), F(1.0))).astype(F)


def attrib_f64(frame, width, height, num_points, E, watch=None):
    """E: H x W float32, already clamped (clamp_plane).  watch: H x W bool or None."""
    E = np.asarray(E, dtype=F)
    assert E.shape == (height, width) and E.min() >= 0 and E.max() <= 1
    E64 = E.astype(np.float64)
    order = frame["sorted"].astype(np.int64)[::-1]  # near -> far
    src = frame["src_index"].astype(np.int64)
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
    T = np.ones((height, width))
    und_count = np.zeros((height, width), dtype=np.int64)
    out = {k: np.zeros(num_points, dtype=np.float64 if k in ("sum", "max") else np.int64) for k in ("sum", "max", "kept", "P", "U")}
    out["front"] = np.zeros(num_points)
    mine = []
    e = 2.0 ** -24
    rad = np.sqrt(scenes.CUT_A) * 1.001
    for s in order:
        m00, m01, m10, m11 = h[s, 0] * W, h[s, 2] * W, -h[s, 1] * H, -h[s, 3] * H
        det = m00 * m11 - m01 * m10
        if not np.isfinite(det) or det == 0:
            continue
        i00, i01, i10, i11 = m11 / det, -m01 / det, -m10 / det, m00 / det
        cx, cy = (h[s, 4] * 0.5 + 0.5) * W, (0.5 - h[s, 5] * 0.5) * H
        ex, ey = rad * np.hypot(m00, m01) + 2, rad * np.hypot(m10, m11) + 2
        x0, x1 = max(int(np.floor(cx - ex)), 0), min(int(np.ceil(cx + ex)), width - 1)
        y0, y1 = max(int(np.floor(cy - ey)), 0), min(int(np.ceil(cy + ey)), height - 1)
        if x0 > x1 or y0 > y1:
            continue
        xs = np.arange(x0, x1 + 1) + 0.5 - cx
        ys = np.arange(y0, y1 + 1)[:, None] + 0.5 - cy
        t00, t01, t10, t11 = i00 * xs, i01 * ys, i10 * xs, i11 * ys
        p0, p1 = t00 + t01, t10 + t11
        a = p0 * p0 + p1 * p1
        e0 = 6 * e * (np.abs(t00) + np.abs(t01)) + 4 * e * 64.0 * (abs(i00) + abs(i01))
        e1 = 6 * e * (np.abs(t10) + np.abs(t11)) + 4 * e * 64.0 * (abs(i10) + abs(i11))
        tol = 4.0 * (2 * np.abs(p0) * e0 + 2 * np.abs(p1) * e1 + 2 * e * a) + 1e-7
        keep = a <= scenes.CUT_A
        und = np.abs(a - scenes.CUT_A) <= tol
        if not (keep.any() or und.any()):
            continue
        j = src[s]
        blk = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        Tb, Eb = T[blk], E64[blk]
        pos = Eb > 0
        w = np.where(keep, np.minimum(0.99, np.exp(-a) * h[s, 9]) * Tb, 0.0)
        v = w * Eb
        out["sum"][j] += v.sum()
        out["max"][j] = max(out["max"][j], v.max())
        out["kept"][j] += int((keep & pos).sum())
        out["P"][j] += int((keep & pos & (Tb < contrib_ref.T_P)).sum())
        if watch is not None and watch[blk].any():
            out["front"][j] = max(out["front"][j], Tb[watch[blk]].max())
        und_count[blk] += und & pos
        mine.append((j, blk, (keep | und) & pos))
        T[blk] = Tb - w
    if und_count.any():
        for j, blk, m in mine:
            b = und_count[blk]
            if b.any():
                out["U"][j] += int(b[m].sum())
    out["T"] = T
    return out


bounds = contrib_ref.bounds
