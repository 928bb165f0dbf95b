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
import weight_ref

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
    T = np.ones((height, width))
    und_count = np.zeros((height, width), dtype=np.int64)
    out = {k: np.zeros(num_points, dtype=np.float64 if k in ("sum", "max") else np.int64) for k in ("sum", "max", "kept", "P", "U")}
    out["front"] = np.zeros(num_points)
    mine = []
    for j, blk, a, keep, und, alpha in weight_ref.records(frame, width, height):
        Tb, Eb = T[blk], E64[blk]
        pos = Eb > 0
        w = weight_ref.weights(a, keep, alpha, Tb)
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
