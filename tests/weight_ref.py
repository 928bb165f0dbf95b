"""The float64 walk of a device frame (its Splat records, draw order and source indices) that contrib_ref, attrib_ref and
values_ref share: the frame's records near -> far, each with its pairs over its footprint box.  Decode and cut-off exactly as
composite_ref.composite_f64 (gaussian.wgsl:40-66, scenes.BoundaryProof's rounding bound); front to back, no early termination.
The transmittance is the caller's: w = weights(...) of a record on T[blk], then T[blk] -= w."""
import numpy as np

import scenes


def records(frame, width, height):
    """Per record with any kept or undecided pair, near -> far: (j, blk, a, keep, und, alpha).
      j      its source Gaussian (frame["src_index"])
      blk    (row slice, column slice) of its footprint box in the viewport; a, keep and und have the box's shape
      a      the exponent of its falloff per pixel
      keep   pairs inside the cut-off
      und    pairs so close to the cut-off that a correct f32 evaluator may decide either way
      alpha  its opacity factor"""
    order = frame["sorted"].astype(np.int64)[::-1]  # near -> far
    src = frame["src_index"].astype(np.int64)
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
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
        if keep.any() or und.any():
            yield src[s], (slice(y0, y1 + 1), slice(x0, x1 + 1)), a, keep, und, h[s, 9]


def weights(a, keep, alpha, Tb):
    """w = b T of a record's kept pairs over its box, 0 elsewhere; Tb: the transmittance in front of it."""
    return np.where(keep, np.minimum(0.99, np.exp(-a) * alpha) * Tb, 0.0)
