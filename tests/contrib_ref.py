"""Float64 per-Gaussian contribution sums of a device frame (its Splat records, draw order and source indices): the reference
of tests/test_gpu_contrib.py.  Decode and cut-off exactly as composite_ref.composite_f64 (gaussian.wgsl:40-66,
scenes.BoundaryProof's rounding bound); front to back, no early termination.

Per source Gaussian j:
  sum[j], max[j]  sum and maximum of w = b T over its kept pairs
  kept[j]         number of kept pairs (pixels)
  P[j]            kept pixels whose transmittance in front of the pair is below 2^-13 (twice the blend's T_MIN: the device may
                  have stopped the pixel's quadrant there, and its f32 T carries rounding)
  U[j]            sum over its pixels of the number of undecided (cut-off-band) pairs at that pixel, its own included.  "Its
                  pixels" are the kept ones AND those where its own pair is undecided: a correct f32 evaluator may keep a pair
                  that float64 discards, and that pixel has to carry the allowance too.
"""
import numpy as np

import scenes

T_P = 2.0 ** -13
CUT_STEP = 0.0092  # weight of a pair on the cut-off, e^(-2 CUTOFF) * 0.99 / (1 - that): what one flipped decision can move


def contrib_f64(frame, width, height, num_points):
    order = frame["sorted"].astype(np.int64)[::-1]  # near -> far
    src = frame["src_index"].astype(np.int64)
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
    T = np.ones((height, width))
    und_count = np.zeros((height, width), dtype=np.int64)
    out = {k: np.zeros(num_points, dtype=np.float64 if k in ("sum", "max") else np.int64) for k in ("sum", "max", "kept", "P", "U")}
    mine = []  # (j, y0, y1, x0, x1, keep | undecided) of every pair set that needs U
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
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        w = np.where(keep, np.minimum(0.99, np.exp(-a) * h[s, 9]) * Tb, 0.0)
        out["sum"][j] += w.sum()
        out["max"][j] = max(out["max"][j], w.max())
        out["kept"][j] += int(keep.sum())
        out["P"][j] += int((keep & (Tb < T_P)).sum())
        und_count[y0:y1 + 1, x0:x1 + 1] += und
        mine.append((j, y0, y1, x0, x1, keep | und))
        T[y0:y1 + 1, x0:x1 + 1] = Tb - w
    if und_count.any():
        for j, y0, y1, x0, x1, m in mine:
            blk = und_count[y0:y1 + 1, x0:x1 + 1]
            if blk.any():
                out["U"][j] += int(blk[m].sum())
    out["T"] = T
    return out


def bounds(ref):
    """(sum tolerance, max tolerance) per Gaussian."""
    tol_sum = 1e-5 * ref["sum"] + 2.0 ** -14 * ref["P"] + CUT_STEP * ref["U"] + 2.0 ** -32 * ref["kept"]
    tol_max = 1e-5 * ref["max"] + np.where(ref["U"] > 0, CUT_STEP, 0.0) + np.where(ref["P"] > 0, 2.0 ** -14, 0.0)
    return tol_sum, tol_max
