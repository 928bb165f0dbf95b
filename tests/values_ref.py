"""Float64 reference of ws_renderer_render_values (include/websplat.h "Rendering per-Gaussian values"; values.h): the walk of
contrib_ref.contrib_f64 -- the same decode, cut-off and undecided band, front to back, no early termination -- kept per PIXEL
instead of per Gaussian.

Per pixel p:
  out[p, c]   sum over kept pairs of w * values[src, c]
  wmax[p]     the largest w of any kept pair, and
  win[p]      the source index of the first pair that has it (-1: no pair with w > 0)
  n[p]        kept pairs
  und[p]      undecided (cut-off-band) pairs
  T[p]        the final transmittance
  wwatch[p]   (with `watch`, H x W source indices) the w of watch[p]'s own kept pair at p, 0 if it has none: what a claimed
              winner weighs in the reference

tolerance(): per pixel, for values bounded by fmax,
  fmax * (1e-5 * (1 - T) + 2^-13 * [T < 2^-13] + 2 * CUT_STEP * und)
-- contrib_ref.bounds' rounding term on the drawn mass; the mass a quadrant may leave behind once every pixel of it is below
T_MIN = 2^-14 (the device's f32 T carries rounding: contrib_ref.T_P); and per flipped cut-off decision its own term (at most
CUT_STEP * fmax) plus what it moves behind it (at most the same)."""
import numpy as np

import contrib_ref
import scenes


def values_f64(frame, width, height, values, watch=None):
    values = np.asarray(values, dtype=np.float32).astype(np.float64)
    if values.ndim == 1:
        values = values[:, None]
    C = values.shape[1]
    order = frame["sorted"].astype(np.int64)[::-1]  # near -> far
    src = frame["src_index"].astype(np.int64)
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
    T = np.ones((height, width))
    out = np.zeros((height, width, C))
    wmax = np.zeros((height, width))
    win = np.full((height, width), -1, dtype=np.int64)
    n = np.zeros((height, width), dtype=np.int64)
    und_count = np.zeros((height, width), dtype=np.int64)
    wwatch = np.zeros((height, width)) if watch is not None else None
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
        Tb = T[blk]
        w = np.where(keep, np.minimum(0.99, np.exp(-a) * h[s, 9]) * Tb, 0.0)
        with np.errstate(invalid="ignore"):  # (a non-finite value times the 0 of a pair that is not kept: discarded)
            out[blk] += np.where(keep[..., None], w[..., None] * values[j], 0.0)
        better = w > wmax[blk]
        wmax[blk] = np.where(better, w, wmax[blk])
        win[blk] = np.where(better, j, win[blk])
        n[blk] += keep
        und_count[blk] += und
        if watch is not None:
            wwatch[blk] += np.where(keep & (watch[blk] == j), w, 0.0)
        T[blk] = Tb - w
    res = {"out": out, "wmax": wmax, "win": win, "n": n, "und": und_count, "T": T}
    if watch is not None:
        res["wwatch"] = wwatch
    return res


def tolerance(ref, fmax):
    """Per pixel (H x W): see the module text."""
    return fmax * (1e-5 * (1.0 - ref["T"]) + contrib_ref.T_P * (ref["T"] < contrib_ref.T_P) + 2.0 * contrib_ref.CUT_STEP * ref["und"])
