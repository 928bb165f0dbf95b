"""Float64 reference of ws_renderer_accumulate_gradient (include/websplat.h "Gradients of an image loss"; gradient.h): the colour
and ln-opacity gradients of an image loss per Gaussian of a device frame (its Splat records, draw order and source indices).  The
pairs are weight_ref.records': front to back, NO early termination; pass 1 is removal_ref.base_f64.

Per pair, with G = plane_G(g, scale) the clamped plane (formed in f32, as the device forms it) and F, T_end of pass 1:
  Tb, w = b Tb, T = Tb - w, P += w c                                     removal_ref's pass 2
  colour:   v_ch = w G_ch                                                iff kept, w > 0 and c_ch > 0
  opacity:  r = w / T, d = r (F - P) - w c, u = r T_end
            v_o = -clamp(opacity_scale (G_r d_r + G_g d_g + G_b d_b + G_T u), +-(1 - 2^-24))
                                                                         iff kept, w > 0, Tb >= 2^-14 and b < 0.99 (not clamped)

gradient_f64 returns, per source Gaussian j: sum[j][4] (colour r, g, b; opacity), tol[j][4] (bounds()); pairs[j] pairs with w > 0
and G != 0; U[j] those of them at a pixel with an undecided (cut-off-band) pair (no bound holds there: the tests mask such pixels
and assert U == 0); band[j] pairs the device may count on one side and not on the other (below); clamped[j] kept pairs with w > 0
on the 0.99 clamp; and per pixel F, T, L, und, cmax of pass 1; amax = the largest |opacity_scale a|.

bounds(): DERIVED, per counted pair, for a device that follows the definition in f32.
  colour   |G_ch| w (1e-5 + 2^-24) + 2^-32
    1e-5 |G| w           contrib_ref.bounds' relative allowance on every w (the f32 exponent and exp2, and the T it is formed from)
    2^-24 |G| w          the one rounded multiply v = w G
    2^-32                the truncation of v 2^32
    a pair whose Tb < 2^-13 (contrib_ref.T_P) may not be walked at all -- its quadrant may have stopped, the device's f32 T
    carries rounding: it gets its whole |v| on top.  The faint stacks have none.
  opacity  opacity_scale (delta (|G_r| + |G_g| + |G_b|) + |G_T| u (2 t_err + 2e-5 + 2^-23) [+ |G_T| r 2^-13] + 4 2^-24 A)
           + 2^-24 |v| + 2^-32
    delta                removal_ref's error of d per channel, term by term as derived there (the chains of F and P, the allowance
                         on w and on T, the four roundings of r, s, t and the fused multiply-add; the r 2^-13 cmax tail on
                         saturating frames): each d_ch enters the dot product times G_ch
    |G_T| u (...)        u = r T_end = w T_end / T: the allowance on w (1e-5) and the rounding of r (2^-24); T and T_end each
                         carry (L + 2) 2^-24 + 1e-5 = t_err as a relative error (chains of factors 1 - b); the rounded multiply
                         (2^-24); 1e-5 + 1e-5 + 2 t_err + 2 2^-24
    |G_T| r 2^-13        SATURATING FRAMES ONLY, pixels whose float64 T_end < 2^-13: the device's T_end may be that of a stopped
                         quadrant, anywhere in [0, 2^-13)
    4 2^-24 A            the four roundings of the dot product (one multiply, three fused multiply-adds), each of a partial sum of
                         magnitude at most A = sum_ch |G_ch d_ch| + |G_T u|
    2^-24 |v|            the rounded multiply by opacity_scale
    2^-32                the truncation
    a pair whose Tb lies in [2^-15, 2^-13] may count on one side and not on the other (removal's band); so may a pair whose
    b = alpha exp(-a) lies within 2e-5 (relative) of 0.99 -- the clamp decision is taken on f32 values that carry the 1e-5
    allowance: either gets an allowance of its whole |v| on top, and is reported in band[j].
tol[j][k] is the sum of this over j's pairs."""
import numpy as np

import contrib_ref
import removal_ref
import weight_ref

T_MIN = 2.0 ** -14
V_CAP = 1.0 - 2.0 ** -24
B_CLAMP = 0.99
MUTATIONS = ("sign_flipped", "r_over_Tb", "clamped_pairs_counted")
SCALE = 2.0 ** 32


def plane_G(g, scale=1.0):
    """G = min(max(scale * g, -1), 1) with NaN -> 0, one rounded f32 multiply: H x W x 4 float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.float32(scale) * np.asarray(g, dtype=np.float32)
    return np.where(np.isnan(e), np.float32(0), np.clip(e, np.float32(-1), np.float32(1))).astype(np.float32)


def forward_f64(recs, col, background, width, height, alpha_factor=None):
    """(F, T_end) of the records with colours col[j]; alpha_factor: {j: factor on its opacity}.  The finite differences of the
    tests run on this; no clamp is applied to a factored opacity beyond the 0.99 of the blend itself."""
    bg = np.asarray(background, dtype=np.float32).astype(np.float64)
    T = np.ones((height, width))
    acc = np.zeros((height, width, 3))
    for j, blk, a, keep, und, alpha in recs:
        k = 1.0 if alpha_factor is None else alpha_factor.get(int(j), 1.0)
        w = weight_ref.weights(a, keep, alpha * k, T[blk])
        acc[blk] += w[..., None] * col[j]
        T[blk] -= w
    return acc + T[..., None] * bg, T


def gradient_f64(frame, width, height, num_points, G, background=(0.0, 0.0, 0.0), opacity_scale=1.0, saturating=False, mutate=None):
    """See the module text.  G: the H x W x 4 clamped plane (plane_G).  mutate: one of MUTATIONS, the wrong formulas bounds() has
    to tell from the right one."""
    assert mutate is None or mutate in MUTATIONS
    recs = list(weight_ref.records(frame, width, height))
    bg = np.asarray(background, dtype=np.float32).astype(np.float64)
    base = removal_ref.base_f64(frame, width, height, bg, records=recs)
    col = removal_ref._colours(frame)
    F, Tend = base["F"], base["T"]
    Gd = np.asarray(G, dtype=np.float32).astype(np.float64)
    assert Gd.shape == (height, width, 4) and np.abs(Gd).max() <= 1.0
    absG = np.abs(Gd)
    live_px = absG.max(axis=-1) > 0
    tail = np.where(Tend < contrib_ref.T_P, contrib_ref.T_P, 0.0) if saturating else np.zeros((height, width))
    acc_err = (base["L"] + 2) * 2.0 ** -23 + 2e-5
    t_err = (base["L"] + 2) * 2.0 ** -24 + 1e-5
    T = np.ones((height, width))
    P = np.zeros((height, width, 3))
    out = {"sum": np.zeros((num_points, 4)), "tol": np.zeros((num_points, 4))}
    out.update({k: np.zeros(num_points, dtype=np.int64) for k in ("pairs", "U", "band", "clamped")})
    amax = 0.0
    so = float(opacity_scale)
    for j, blk, a, keep, und, alpha in recs:
        Tb = T[blk]
        w = weight_ref.weights(a, keep, alpha, Tb)
        Ta = Tb - w
        c = col[j]
        Pa = P[blk] + w[..., None] * c
        g, ag = Gd[blk], absG[blk]
        drawn = keep & (w > 0)
        live = drawn & live_px[blk]
        if live.any():
            # ---- colour
            v = np.where((drawn[..., None]) & (c > 0), w[..., None] * g[..., :3], 0.0)
            tol = np.where(v != 0, np.abs(v) * (1e-5 + 2.0 ** -24) + 2.0 ** -32, 0.0)
            tol += np.where((Tb < contrib_ref.T_P)[..., None], np.abs(v), 0.0)
            out["sum"][j, :3] += v.sum(axis=(0, 1))
            out["tol"][j, :3] += tol.sum(axis=(0, 1))
            # ---- opacity
            b_raw = np.exp(-a) * alpha
            clamped = keep & (b_raw >= B_CLAMP)
            near_clamp = drawn & (np.abs(b_raw - B_CLAMP) <= 2e-5 * B_CLAMP)
            out["clamped"][j] += int((clamped & drawn).sum())
            may = drawn & (Tb >= 2.0 ** -15)                       # pairs the device may count
            counted = drawn & (Tb >= T_MIN)
            if mutate != "clamped_pairs_counted":
                counted = counted & ~clamped
                may = may & (~clamped | near_clamp)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(may, w / (Tb if mutate == "r_over_Tb" else Ta), 0.0)
            d = r[..., None] * (F[blk] - Pa) - w[..., None] * c
            u = r * Tend[blk]
            terms = np.concatenate([g[..., :3] * d, (g[..., 3] * u)[..., None]], axis=-1)
            aa = so * terms.sum(axis=-1)
            vo = -np.clip(aa, -V_CAP, V_CAP)
            if mutate == "sign_flipped":
                vo = -vo
            cm = base["cmax"][blk]
            delta = r * cm * (acc_err[blk] + t_err[blk] + tail[blk]) + (2e-5 + 4 * 2.0 ** -24) * w * cm
            A = np.abs(terms).sum(axis=-1)
            tol_o = so * (delta * ag[..., :3].sum(axis=-1) + ag[..., 3] * (u * (2.0 * t_err[blk] + 2e-5 + 2.0 ** -23) + r * tail[blk]) + 4 * 2.0 ** -24 * A)
            tol_o = tol_o + 2.0 ** -24 * np.abs(vo) + 2.0 ** -32
            in_band = may & live_px[blk] & (((Tb >= 2.0 ** -15) & (Tb <= 2.0 ** -13)) | near_clamp)
            vo_counted = np.where(counted, vo, 0.0)
            tol_o = np.where(may & live_px[blk], tol_o + np.where(in_band, np.abs(vo), 0.0), 0.0)
            out["sum"][j, 3] += vo_counted.sum()
            out["tol"][j, 3] += tol_o.sum()
            out["pairs"][j] += int(live.sum())
            out["U"][j] += int((live & (base["und"][blk] > 0)).sum())
            out["band"][j] += int(in_band.sum())
            if counted.any():
                amax = max(amax, float(np.abs(aa[counted]).max()))
        P[blk] = Pa
        T[blk] = Ta
    out.update({k: base[k] for k in ("F", "T", "L", "und", "cmax")})
    out["amax"] = amax
    return out


def bounds(ref):
    """Tolerance of the four sums per Gaussian, (N, 4): the module text."""
    return ref["tol"]
