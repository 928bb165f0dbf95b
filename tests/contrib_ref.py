"""Float64 per-Gaussian contribution sums of a device frame (its Splat records, draw order and source indices): the reference
of tests/test_gpu_contrib.py.  The pairs are weight_ref.records': front to back, no early termination.

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

import weight_ref

T_P = 2.0 ** -13
CUT_STEP = 0.0092  # weight of a pair on the cut-off, e^(-2 CUTOFF) * 0.99 / (1 - that): what one flipped decision can move


def contrib_f64(frame, width, height, num_points):
    T = np.ones((height, width))
    und_count = np.zeros((height, width), dtype=np.int64)
    out = {k: np.zeros(num_points, dtype=np.float64 if k in ("sum", "max") else np.int64) for k in ("sum", "max", "kept", "P", "U")}
    mine = []  # (j, blk, keep | undecided) of every pair set that needs U
    for j, blk, a, keep, und, alpha in weight_ref.records(frame, width, height):
        Tb = T[blk]
        w = weight_ref.weights(a, keep, alpha, Tb)
        out["sum"][j] += w.sum()
        out["max"][j] = max(out["max"][j], w.max())
        out["kept"][j] += int(keep.sum())
        out["P"][j] += int((keep & (Tb < T_P)).sum())
        und_count[blk] += und
        mine.append((j, blk, keep | und))
        T[blk] = Tb - w
    if und_count.any():
        for j, blk, m in mine:
            b = und_count[blk]
            if b.any():
                out["U"][j] += int(b[m].sum())
    out["T"] = T
    return out


def bounds(ref):
    """(sum tolerance, max tolerance) per Gaussian."""
    tol_sum = 1e-5 * ref["sum"] + 2.0 ** -14 * ref["P"] + CUT_STEP * ref["U"] + 2.0 ** -32 * ref["kept"]
    tol_max = 1e-5 * ref["max"] + np.where(ref["U"] > 0, CUT_STEP, 0.0) + np.where(ref["P"] > 0, 2.0 ** -14, 0.0)
    return tol_sum, tol_max
