"""Float64 reference of ws_renderer_render_values (include/websplat.h "Rendering per-Gaussian values"; values.h): the walk of
contrib_ref.contrib_f64 (weight_ref.records: front to back, no early termination) kept per PIXEL instead of per Gaussian.

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
import weight_ref


def values_f64(frame, width, height, values, watch=None):
    values = np.asarray(values, dtype=np.float32).astype(np.float64)
    if values.ndim == 1:
        values = values[:, None]
    C = values.shape[1]
    T = np.ones((height, width))
    out = np.zeros((height, width, C))
    wmax = np.zeros((height, width))
    win = np.full((height, width), -1, dtype=np.int64)
    n = np.zeros((height, width), dtype=np.int64)
    und_count = np.zeros((height, width), dtype=np.int64)
    wwatch = np.zeros((height, width)) if watch is not None else None
    for j, blk, a, keep, und, alpha in weight_ref.records(frame, width, height):
        Tb = T[blk]
        w = weight_ref.weights(a, keep, alpha, Tb)
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
