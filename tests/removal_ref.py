"""Float64 reference of ws_renderer_accumulate_removal (include/websplat.h "Removal effect"; removal.h): what deleting each
Gaussian alone would do to a device frame (its Splat records, draw order and source indices).  The pairs are weight_ref.records':
front to back, NO early termination, in two passes as the definition has them.

Pass 1, per pixel:  F = sum over kept pairs of w c + T_end * background, T_end, L = kept pairs, und = undecided (cut-off-band)
pairs, cmax = the largest of 1, |background| and |c| of any kept pair at the pixel.
Pass 2, per pair:   Tb, w, T = Tb - w, P += w c; the pair counts iff kept, w > 0 and Tb >= 2^-14; r = w / T, d = r (F - P) - w c,
m = mean_ch d^2 ("sq") or mean_ch |d| ("abs"), v = min(scale m, 1 - 2^-24) * E(p).

removal_f64 returns, per source Gaussian j: sum[j], max[j] of v; pairs[j] counted pairs with E > 0; U[j] those of them at a pixel
with an undecided pair (no bound holds there: a flipped cut-off decision moves every weight behind it -- the tests mask such
pixels and assert U == 0); tol_sum[j], tol_max[j] (bounds()); and per pixel F, T, L, und, cmax; dmax = the largest |d|.

bounds(): DERIVED, per counted pair, for a device that follows the definition in f32.  d = r s - w c with s = F - P:
  delta = r cmax ((L + 2) 2^-23 + 2e-5) + r cmax ((L + 2) 2^-24 + 1e-5) + (2e-5 + 4 2^-24) w cmax  [+ r 2^-13 cmax]
    r cmax (L + 2) 2^-23   F and P are chains of at most L fused multiply-adds plus F's background term, every rounding at most
                         2^-24 of a partial sum of magnitude <= cmax (the weights sum to at most 1).  P is bit for bit pass 1's
                         prefix, so only the roundings behind the pair survive in s: at most (L + 2) 2^-24 cmax, taken twice for
                         good measure; s enters d times r
    r cmax 2e-5          contrib_ref.bounds' 1e-5 relative allowance on every w (the f32 exponent and exp2) and on the T it is
                         formed from, reaching s through what lies behind the pair; times r
    r cmax ((L + 2) 2^-24 + 1e-5)   r = w / T carries T's own error -- L rounded subtractions from at most 1 and the allowance
                         on the mass drawn so far -- as a RELATIVE error dT / T; what lies behind the pair is at most cmax T, so
                         r s moves by at most r cmax dT
    (2e-5 + 4 2^-24) w cmax   the allowance on the pair's own w, once in r and once in t = w c (|r s| and |t| are at most
                         w cmax), and the four roundings of r, s, t and the final fused multiply-add, each of a value that small
    r 2^-13 cmax         SATURATING FRAMES ONLY, pixels whose float64 T_end < 2^-13 (contrib_ref.T_P): the device's quadrant may
                         have stopped, and its F lacks the tail, at most the transmittance left there times cmax
  Against the form the feature was specified with, (1 + r) cmax ((L + 2) 2^-23 + 2e-5) + 1e-5 w cmax: the "1" has no source in
  this arithmetic -- nothing of magnitude cmax enters d except through r -- and on a faint stack of a thousand layers it alone
  is six times the value under test, so it is dropped (tighter wherever r < 2); T's own error and the second use of w were
  missing and are added (wider by up to half at r >= 2, the opaque stacks).
  sq:  |mean (d + x)^2 - mean d^2| <= (2 sqrt(3 m) + delta) delta for |x| <= delta per channel (|d_ch| <= sqrt(3 m))
  abs: |mean |d + x| - mean |d||   <= delta
  + 8 2^-24 v            the separately rounded steps behind d: e, two additions, / 3, scale * m, v * E (at most 6 roundings)
  + 2^-32                the truncation of v 2^32
  a pair whose Tb lies in [2^-15, 2^-13] may count on one side and not on the other (the device's f32 T carries rounding): it
  gets an allowance of its whole v on top.
tol_sum[j] is the sum of this over j's pairs (times scale and E); tol_max[j] its largest single value: maxima differ by at most
the largest pairwise difference.

base_bounds(): per pixel, for the base plane.  F: cmax ((L + 2) 2^-24 + 1e-5) -- the chain above once, and the weights'
allowance; T_end: (L + 2) 2^-24 + 1e-5 (L rounded subtractions from at most 1, the allowance on the drawn mass); both + 2^-13
cmax where the float64 T_end < 2^-13 (the stop)."""
import numpy as np

import contrib_ref
import weight_ref

T_MIN = 2.0 ** -14
V_CAP = 1.0 - 2.0 ** -24
MUTATIONS = ("no_background", "prefix_without_i", "r_over_Tb")


def _colours(frame):
    """c[j] of every source Gaussian: halves 6..8 of its Splat record."""
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    src = frame["src_index"].astype(np.int64)
    col = np.zeros((int(src.max()) + 1 if src.size else 1, 3))
    col[src] = h[: src.size, 6:9]
    return col


def base_f64(frame, width, height, background, skip=None, records=None):
    """Pass 1 (and the brute force of the tests: skip = a source index left out of the frame)."""
    bg = np.asarray(background, dtype=np.float32).astype(np.float64)
    col = _colours(frame)
    T = np.ones((height, width))
    acc = np.zeros((height, width, 3))
    L = np.zeros((height, width), dtype=np.int64)
    und_count = np.zeros((height, width), dtype=np.int64)
    cmax = np.full((height, width), max(1.0, float(np.abs(bg).max())))
    for j, blk, a, keep, und, alpha in (records if records is not None else weight_ref.records(frame, width, height)):
        if skip is not None and j == skip:
            continue
        Tb = T[blk]
        w = weight_ref.weights(a, keep, alpha, Tb)
        acc[blk] += w[..., None] * col[j]
        L[blk] += keep
        und_count[blk] += und
        cmax[blk] = np.where(keep, np.maximum(cmax[blk], np.abs(col[j]).max()), cmax[blk])
        T[blk] = Tb - w
    return {"F": acc + T[..., None] * bg, "acc": acc, "T": T, "L": L, "und": und_count, "cmax": cmax}


def removal_f64(frame, width, height, num_points, background=(0.0, 0.0, 0.0), kind="sq", scale=1.0, E=None, saturating=False,
                mutate=None):
    """See the module text.  E: None or the H x W plane of weights in [0, 1] (already clamped).  mutate: one of MUTATIONS, the
    wrong formulas bounds() has to tell from the right one."""
    assert kind in ("sq", "abs") and (mutate is None or mutate in MUTATIONS)
    recs = list(weight_ref.records(frame, width, height))
    bg = np.asarray(background, dtype=np.float32).astype(np.float64)
    base = base_f64(frame, width, height, bg, records=recs)
    col = _colours(frame)
    F = base["acc"] if mutate == "no_background" else base["F"]
    Ew = np.ones((height, width)) if E is None else np.asarray(E, dtype=np.float32).astype(np.float64)
    tail = np.where(base["T"] < contrib_ref.T_P, contrib_ref.T_P, 0.0) if saturating else np.zeros((height, width))
    acc_err = (base["L"] + 2) * 2.0 ** -23 + 2e-5
    t_err = (base["L"] + 2) * 2.0 ** -24 + 1e-5
    T = np.ones((height, width))
    P = np.zeros((height, width, 3))
    out = {k: np.zeros(num_points) for k in ("sum", "max", "tol_sum", "tol_max")}
    out.update({k: np.zeros(num_points, dtype=np.int64) for k in ("pairs", "U", "band")})
    dmax = 0.0
    for j, blk, a, keep, und, alpha in recs:
        Tb = T[blk]
        w = weight_ref.weights(a, keep, alpha, Tb)
        Ta = Tb - w
        c = col[j]
        Pb = P[blk]
        Pa = Pb + w[..., None] * c
        counted = keep & (w > 0) & (Tb >= T_MIN)
        if counted.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(counted, w / (Tb if mutate == "r_over_Tb" else Ta), 0.0)
            s = F[blk] - (Pb if mutate == "prefix_without_i" else Pa)
            d = r[..., None] * s - w[..., None] * c
            m = (d * d).mean(axis=-1) if kind == "sq" else np.abs(d).mean(axis=-1)
            e = Ew[blk]
            v = np.where(counted, np.minimum(scale * m, V_CAP) * e, 0.0)
            cm = base["cmax"][blk]
            delta = r * cm * (acc_err[blk] + t_err[blk] + tail[blk]) + (2e-5 + 4 * 2.0 ** -24) * w * cm
            dm = (2.0 * np.sqrt(3.0 * m) + delta) * delta if kind == "sq" else delta
            tol = scale * dm * e + 8.0 * 2.0 ** -24 * v + 2.0 ** -32
            in_band = counted & (Tb >= 2.0 ** -15) & (Tb <= 2.0 ** -13)
            tol = np.where(counted & (e > 0), tol + np.where(in_band, v, 0.0), 0.0)
            live = counted & (e > 0)
            out["sum"][j] += v.sum()
            out["max"][j] = max(out["max"][j], v.max())
            out["tol_sum"][j] += tol.sum()
            out["tol_max"][j] = max(out["tol_max"][j], tol.max())
            out["pairs"][j] += int(live.sum())
            out["U"][j] += int((live & (base["und"][blk] > 0)).sum())
            out["band"][j] += int((in_band & (e > 0)).sum())
            dmax = max(dmax, float(np.abs(d[counted]).max()))
        # a pair below the counting threshold that the device's T may still count: Tb in [2^-15, 2^-14)
        low = keep & (w > 0) & (Tb < T_MIN) & (Tb >= 2.0 ** -15) & (Ew[blk] > 0)
        if low.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(low, w / Ta, 0.0)
            d = r[..., None] * (F[blk] - Pa) - w[..., None] * c
            m = (d * d).mean(axis=-1) if kind == "sq" else np.abs(d).mean(axis=-1)
            cm = base["cmax"][blk]
            delta = r * cm * (acc_err[blk] + t_err[blk] + tail[blk]) + (2e-5 + 4 * 2.0 ** -24) * w * cm
            dm = (2.0 * np.sqrt(3.0 * m) + delta) * delta if kind == "sq" else delta
            allow = np.where(low, (np.minimum(scale * m, V_CAP) + scale * dm) * Ew[blk] + 2.0 ** -32, 0.0)
            out["tol_sum"][j] += allow.sum()
            out["tol_max"][j] = max(out["tol_max"][j], allow.max())
            out["band"][j] += int(low.sum())
        P[blk] = Pa
        T[blk] = Ta
    out.update({k: base[k] for k in ("F", "T", "L", "und", "cmax")})
    out["dmax"] = dmax
    return out


def bounds(ref):
    """(sum tolerance, max tolerance) per Gaussian: the module text."""
    return ref["tol_sum"], ref["tol_max"]


def base_bounds(ref, saturating=False):
    """(tolerance of F, tolerance of T_end), H x W each."""
    chain = (ref["L"] + 2) * 2.0 ** -24 + 1e-5
    tail = np.where(ref["T"] < contrib_ref.T_P, contrib_ref.T_P, 0.0) if saturating else 0.0
    return ref["cmax"] * (chain + tail), chain + tail


def undecided_mask(ref):
    """H x W bool: the pixels a test has to give a weight of 0 -- an undecided pair, or a float64 T_end below 2^-13."""
    return (ref["und"] > 0) | (ref["T"] < contrib_ref.T_P)
