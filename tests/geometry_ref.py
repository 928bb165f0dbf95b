"""Float64 references of "Geometry gradients" (include/websplat.h; geometry.h, geometry_spread.h).  Pure numpy; nothing here needs a GPU.

  (a) stage_a_f64     gradient_ref.gradient_f64's walk over a device frame, taken on to the five screen-space sums per Gaussian
                      m0, m1, S00, S01, S11 = sum over counted pairs of kappa (p0, p1, p0 p0, p0 p1, p1 p1), with bounds()
  (b) spread_f64      the chain of k_geom_spread in numpy float64, in the twin's operation order: the five sums, the record's halves,
                      the cloud's position and covariance and the frame's uniforms -> position, covariance, screen_norm, seen
  (c) forward_from_cloud   continuous, unrounded records from k1_edges.k1_f64 and a float64 composite of them: L = sum G . F + G_T
                      T_end.  The finite differences of test_geometry_ref.py run on this; analytic_from_cloud is the same chain as
                      (b) fed with the float64 sums of the same continuous records.

bounds() of (a): DERIVED, per counted pair, for a device that follows geometry.h in f32.  With t = s kappa (s = geometry_scale):
  e_t   = s (delta (|G_r| + |G_g| + |G_b|) + |G_T| u (2 t_err + 2e-5 + 2^-23) [+ |G_T| r 2^-13] + 4 2^-24 A) + 2^-24 |t|
          gradient_ref.bounds' error of opacity_scale * a WITHOUT its truncation, term by term as derived there, s in the place of
          opacity_scale
  e_pk  = 16 2^-24 (|I'_k0| (|dx| + 64) + |I'_k1| (|dy| + 64)) + 8 2^-24 (|I'_k0| (|cx| + W) + |I'_k1| (|cy| + H))
          decode's f32 operations (blend_stage.h): every entry of I' carries at most 12 roundings' worth of relative error (v W, the
          two products and the difference of det -- both products have the sign of det for K1's orthogonal axes, no cancellation --
          the division, the constant, the product), the tile-local centre at most 4 2^-24 (|cx| + W) absolute (the affine map of
          the f16, the subtraction of the tile's origin), c_k = -(I'_k0 cxl + I'_k1 cyl) three more, and p_k = fma(I'_k0, lx,
          fma(I'_k1, ly, c_k)) two more, where |lx| <= 32 and |cxl| <= |dx| + 32.  test_geometry_ref.py checks it against
          ws_debug_stage_splat.
  v_mk  : |p_k| e_t + |t| e_pk + 2^-24 |v| + 2^-32                          the product's two factors, its rounding, the truncation
  v_Skl : |p_k p_l| e_t + |t| (|p_l| e_pk + |p_k| e_pl + e_pk e_pl) + 2 2^-24 |v| + 2^-32      two roundings
  a pair in the band (Tb in [2^-15, 2^-13], or b within 2e-5 relative of 0.99) may count on one side and not on the other: it gets
  its whole |v| on top, as in gradient_ref.  Pixels with an undecided cut-off pair carry no bound: the tests mask them out of the
  plane and assert U == 0.

THE CAP.  geom_value (geometry.hip) turns the f32 value v' of a channel into clamp(v', +-V_CAP), V_CAP = 1 - 2^-24, and the
accumulator into q = trunc(|.| 2^32) with the value's sign: a capped value is the integer +-(2^32 - 256), whatever v' was.  With
v the float64 value of the pair and channel, e = errs[k] the error of the product's factors above and n the product's own
roundings (1 for m, 2 for S), the device's v' = v~ (1 + d_1) .. (1 + d_n) with |v~ - v| <= e, |d_i| <= 2^-24, hence
  |v'| >= (|v| - e) (1 - 2^-24)^n >= |v| - e - n 2^-24 |v|  =: lower            |v'| <= |v| + e + n 2^-24 |v|  =: upper
(to first order in 2^-24, as every term here).  A pair and channel is
  DECIDEDLY CAPPED  iff the pair counts on both sides (counted, and not in the band) and lower >= V_CAP: v' has v's sign (lower >
              0) and |v'| >= V_CAP, so fminf / fmaxf return +-V_CAP exactly; V_CAP 2^32 = 2^32 - 256 is an integer, the truncation
              drops nothing.  The reference adds sign(v) V_CAP, the tolerance of the pair is 0 -- no 2^-32 either.
  STRADDLING        iff it may count, is not decidedly capped, and upper >= V_CAP: either side may or may not be capped.  It keeps
              the treatment of an uncapped pair -- the clamp is a contraction, |clamp(v') - clamp(v)| <= |v' - v| -- and since
              both clamped values lie in [-V_CAP, V_CAP] its tolerance is at most 2 V_CAP.
  any other pair has upper < V_CAP: neither side is capped, nothing changes.
capped[j][k] and straddling[j][k] count them; net[j][k] is the signed count of the decidedly capped (positive minus negative).
A Gaussian and channel whose pairs are all decidedly capped has tol == 0 and sum == net V_CAP exactly (a multiple of 2^-24 below
2^11: exact in float64), and the device's q must be the integer net (2^32 - 256).  Where nothing is capped or straddling, sum and
tol are what they were before this rule to the last bit: the same operations in the same order (test_geometry_ref.py pins them).

STAGE_A_MUTATIONS: the defective walks the bounds have to tell from the right one (mutate=):
  p_swapped              p0 and p1 exchanged before the five products (their errors with them)
  iprime_transposed      I' transposed, in p and in its error
  s01_negated            the sign of the S01 channel
  clamped_pairs_counted  a pair on the 0.99 clamp counts, with the kappa its w gives (gradient_ref's mutant of that name)
  cap_ignored            no clamp to +-V_CAP: every pair keeps the uncapped treatment"""
import numpy as np

import contrib_ref
import removal_ref
import weight_ref

F64 = np.float64
LN2 = float(np.log(2.0))
LOG2E = 1.0 / LN2
SQRT_LOG2E = float(np.sqrt(LOG2E))
T_MIN = 2.0 ** -14
V_CAP = 1.0 - 2.0 ** -24
B_CLAMP = 0.99
CUT_A = 2.0 * 2.3539888583335364          # natural-exponent domain: a pair is kept iff a <= CUT_A (a' = a log2 e)
C_0P1 = float(np.float32(0.1))
MUTATIONS = ("no_jacobian", "offdiag_not_doubled", "dmu_y_not_flipped", "ln2_once")
STAGE_A_MUTATIONS = ("p_swapped", "iprime_transposed", "s01_negated", "clamped_pairs_counted", "cap_ignored")
Q_CAP = 2 ** 32 - 256                      # V_CAP 2^32: what a capped value adds to a q32 sum
E24 = 2.0 ** -24


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def _iprime(h, W, H):
    """I' (2 x 2, exp2 domain), the pixel centre and M's rows from a record's ten halves (float64), by decode's expressions."""
    m00, m01, m10, m11 = h[0] * W, h[2] * W, -h[1] * H, -h[3] * H
    det = m00 * m11 - m01 * m10
    inv = SQRT_LOG2E / det
    I = np.array([[m11 * inv, -m01 * inv], [-m10 * inv, m00 * inv]])
    return I, ((h[4] * 0.5 + 0.5) * W, (0.5 - h[5] * 0.5) * H)


def p_error(I, dx, dy, cx, cy, W, H):
    """e_p0, e_p1 of the module text over a box of offsets dx (row vector) and dy (column vector)."""
    out = []
    for k in range(2):
        a0, a1 = abs(I[k, 0]), abs(I[k, 1])
        out.append(16 * E24 * (a0 * (np.abs(dx) + 64.0) + a1 * (np.abs(dy) + 64.0)) + 8 * E24 * (a0 * (abs(cx) + W) + a1 * (abs(cy) + H)))
    return out


def stage_a_f64(frame, width, height, num_points, G, background=(0.0, 0.0, 0.0), geometry_scale=1.0, saturating=False, mutate=None):
    """See the module text.  G: the H x W x 4 clamped plane (gradient_ref.plane_G).  Returns sum[j][5] (in units of v: s kappa p..),
    tol[j][5], per Gaussian pairs, U, band, clamped as gradient_ref.gradient_f64 does and counted (the pairs that count), and per
    Gaussian and channel capped, net, straddling (THE CAP); open_px [H, W]: the pixels with a pair and channel that may count and
    is not decidedly capped (masked out of the plane, nothing but exact integers is left).  mutate: one of STAGE_A_MUTATIONS."""
    assert mutate is None or mutate in STAGE_A_MUTATIONS
    recs = list(weight_ref.records(frame, width, height))
    bg = np.asarray(background, dtype=np.float32).astype(F64)
    base = removal_ref.base_f64(frame, width, height, bg, records=recs)
    col = removal_ref._colours(frame)
    F, Tend = base["F"], base["T"]
    Gd = np.asarray(G, dtype=np.float32).astype(F64)
    assert Gd.shape == (height, width, 4) and np.abs(Gd).max() <= 1.0
    absG = np.abs(Gd)
    live_px = absG.max(axis=-1) > 0
    tail = np.where(Tend < contrib_ref.T_P, contrib_ref.T_P, 0.0) if saturating else np.zeros((height, width))
    acc_err = (base["L"] + 2) * 2.0 ** -23 + 2e-5
    t_err = (base["L"] + 2) * 2.0 ** -24 + 1e-5
    halves = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(F64)
    slot_of = {int(j): s for s, j in enumerate(frame["src_index"].astype(np.int64)[: len(halves)])}
    W, H = float(width), float(height)
    T = np.ones((height, width))
    P = np.zeros((height, width, 3))
    out = {"sum": np.zeros((num_points, 5)), "tol": np.zeros((num_points, 5))}
    out.update({k: np.zeros(num_points, dtype=np.int64) for k in ("pairs", "U", "band", "clamped", "counted")})
    out.update({k: np.zeros((num_points, 5), dtype=np.int64) for k in ("capped", "net", "straddling")})
    out["open_px"] = np.zeros((height, width), dtype=bool)   # pixels with a judged pair and channel that is not decidedly capped
    s = float(geometry_scale)
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
            b_raw = np.exp(-a) * alpha
            clamped = keep & (b_raw >= B_CLAMP)
            near_clamp = drawn & (np.abs(b_raw - B_CLAMP) <= 2e-5 * B_CLAMP)
            out["clamped"][j] += int((clamped & drawn).sum())
            may = drawn & (Tb >= 2.0 ** -15)
            counted = drawn & (Tb >= T_MIN)
            if mutate != "clamped_pairs_counted":
                may = may & (~clamped | near_clamp)
                counted = counted & ~clamped
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(may, w / Ta, 0.0)
            d = r[..., None] * (F[blk] - Pa) - w[..., None] * c
            u = r * Tend[blk]
            terms = np.concatenate([g[..., :3] * d, (g[..., 3] * u)[..., None]], axis=-1)
            t = s * terms.sum(axis=-1)
            cm = base["cmax"][blk]
            delta = r * cm * (acc_err[blk] + t_err[blk] + tail[blk]) + (2e-5 + 4 * E24) * w * cm
            A = np.abs(terms).sum(axis=-1)
            e_t = s * (delta * ag[..., :3].sum(axis=-1) + ag[..., 3] * (u * (2.0 * t_err[blk] + 2e-5 + 2.0 ** -23) + r * tail[blk]) + 4 * E24 * A)
            e_t = e_t + E24 * np.abs(t)
            # the pair's coordinates, exp2 domain
            I, (cx, cy) = _iprime(halves[slot_of[int(j)]], W, H)
            if mutate == "iprime_transposed":
                I = I.T
            dx = np.arange(blk[1].start, blk[1].stop)[None, :] + 0.5 - cx
            dy = np.arange(blk[0].start, blk[0].stop)[:, None] + 0.5 - cy
            p0 = I[0, 0] * dx + I[0, 1] * dy
            p1 = I[1, 0] * dx + I[1, 1] * dy
            e0, e1 = p_error(I, dx, dy, cx, cy, W, H)
            if mutate == "p_swapped":
                p0, p1, e0, e1 = p1, p0, e1, e0
            in_band = may & live_px[blk] & (((Tb >= 2.0 ** -15) & (Tb <= 2.0 ** -13)) | near_clamp)
            vals = (t * p0, t * p1, t * p0 * p0, t * p0 * p1, t * p1 * p1)
            at = np.abs(t)
            errs = (np.abs(p0) * e_t + at * e0, np.abs(p1) * e_t + at * e1,
                    p0 * p0 * e_t + at * (2 * np.abs(p0) * e0 + e0 * e0), np.abs(p0 * p1) * e_t + at * (np.abs(p1) * e0 + np.abs(p0) * e1 + e0 * e1),
                    p1 * p1 * e_t + at * (2 * np.abs(p1) * e1 + e1 * e1))
            if mutate == "s01_negated":
                vals = vals[:3] + (-vals[3],) + vals[4:]
            judged = may & live_px[blk]
            for k in range(5):
                n_round = 1 if k < 2 else 2
                if mutate == "cap_ignored":
                    v = vals[k]
                    decided = straddle = np.zeros(v.shape, dtype=bool)
                else:
                    v = np.clip(vals[k], -V_CAP, V_CAP)
                    slack = errs[k] + n_round * E24 * np.abs(vals[k])
                    decided = counted & live_px[blk] & ~in_band & (np.abs(vals[k]) - slack >= V_CAP)
                    straddle = judged & ~decided & (np.abs(vals[k]) + slack >= V_CAP)
                tol = errs[k] + n_round * E24 * np.abs(v) + 2.0 ** -32
                tol = np.where(judged, tol + np.where(in_band, np.abs(v), 0.0), 0.0)
                if straddle.any():
                    tol = np.where(straddle, np.minimum(tol, 2.0 * V_CAP), tol)
                if decided.any():
                    tol = np.where(decided, 0.0, tol)
                    out["capped"][j, k] += int(decided.sum())
                    out["net"][j, k] += int((decided & (v > 0)).sum()) - int((decided & (v < 0)).sum())
                out["straddling"][j, k] += int(straddle.sum())
                out["open_px"][blk] |= judged & ~decided
                out["sum"][j, k] += np.where(counted, v, 0.0).sum()
                out["tol"][j, k] += tol.sum()
            out["pairs"][j] += int(live.sum())
            out["counted"][j] += int((counted & live_px[blk]).sum())
            out["U"][j] += int((live & (base["und"][blk] > 0)).sum())
            out["band"][j] += int(in_band.sum())
        P[blk] = Pa
        T[blk] = Ta
    out.update({k: base[k] for k in ("F", "T", "L", "und")})
    return out


def bounds(ref):
    """Tolerance of the five sums per Gaussian, (N, 5): the module text."""
    return ref["tol"]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def _project(xyz, cov6, u):
    """K1's quantities of the chain, as k1_edges.k1_f64 states them (float64; u = k1_edges.uniforms_f64())."""
    view, proj = u["view"], u["proj"]
    x = np.asarray(xyz, dtype=F64)
    cs = x @ view[:, :3].T + view[:, 3]
    clip = cs @ proj.T
    fx, fy = u["focal"]
    cz = cs[:, 2]
    n = len(x)
    jac = np.zeros((n, 2, 3))
    jac[:, 0, 0], jac[:, 0, 2] = fx / cz, -(fx * cs[:, 0]) / (cz * cz)
    jac[:, 1, 1], jac[:, 1, 2] = -fy / cz, (fy * cs[:, 1]) / (cz * cz)
    R = view[:3, :3]
    T = jac @ R
    dd = 5.0 * np.linalg.norm(u["scene_center"] - x, axis=1) / u["scene_extend"]
    t = np.clip(u["walltime"] - dd, 0.0, 1.0)
    scale_mod = np.where(u["walltime"] > dd, t * t * (3.0 - 2.0 * t), 0.0)
    sc2 = (u["gaussian_scaling"] * scale_mod) ** 2
    c = np.asarray(cov6, dtype=F64) * sc2[:, None]
    V = np.empty((n, 3, 3))
    V[:, 0, 0], V[:, 0, 1], V[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
    V[:, 1, 0], V[:, 1, 1], V[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
    V[:, 2, 0], V[:, 2, 1], V[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
    cov2 = T @ V @ np.transpose(T, (0, 2, 1))
    d1, d2 = cov2[:, 0, 0] + u["kernel_size"], cov2[:, 1, 1] + u["kernel_size"]
    lam2 = 0.5 * (d1 + d2) - np.sqrt(((d1 - d2) / 2.0) ** 2 + cov2[:, 0, 1] ** 2)
    return {"cs": cs, "clip": clip, "w": clip[:, 3], "T": T, "V": V, "sc2": sc2, "R": R, "lambda2_raw": lam2, "fx": fx, "fy": fy}


def chain_f64(m, S, I, xyz, cov6, u, width, height, mutate=None):
    """m [n, 2], S [n, 3] (00, 01, 11), I [n, 2, 2] -> position [n, 3], covariance [n, 6], norm [n], free [n] (lambda2 off the
    clamp).  mutate: one of MUTATIONS, the defective chains test_geometry_ref.py has to tell from the right one."""
    assert mutate is None or mutate in MUTATIONS
    W, H = float(width), float(height)
    k = _project(xyz, cov6, u)
    n = len(m)
    Sm = np.empty((n, 2, 2))
    Sm[:, 0, 0], Sm[:, 0, 1], Sm[:, 1, 0], Sm[:, 1, 1] = S[:, 0], S[:, 1], S[:, 1], S[:, 2]
    It = np.transpose(I, (0, 2, 1))
    dmu = -2.0 * LN2 * np.einsum("nab,nb->na", It, m)
    D = -2.0 * (LN2 if mutate == "ln2_once" else LN2 * LN2) * (It @ Sm @ I)
    flip = np.array([[1.0, -1.0], [-1.0, 1.0]])
    DK = D * flip
    gx = 0.5 * W * dmu[:, 0]
    gy = (0.5 if mutate == "dmu_y_not_flipped" else -0.5) * H * dmu[:, 1]
    w, clip = k["w"], k["clip"]
    dclip = np.zeros((n, 4))
    dclip[:, 0], dclip[:, 1], dclip[:, 3] = gx / w, gy / w, -(gx * clip[:, 0] + gy * clip[:, 1]) / (w * w)
    dcs = dclip @ u["proj"]
    free = k["lambda2_raw"] >= C_0P1
    T, V, R = k["T"], k["V"], k["R"]
    Gt = 2.0 * (DK @ T @ V)
    J = Gt @ R.T                                                  # dL/djac [n, 2, 3]
    cs, fx, fy = k["cs"], k["fx"], k["fy"]
    cz = cs[:, 2]
    add = np.zeros((n, 4))
    add[:, 0] = J[:, 0, 2] * (-fx / cz ** 2)
    add[:, 1] = J[:, 1, 2] * (fy / cz ** 2)
    add[:, 2] = J[:, 0, 0] * (-fx / cz ** 2) + J[:, 0, 2] * (2.0 * fx * cs[:, 0] / cz ** 3) + J[:, 1, 1] * (fy / cz ** 2) \
        + J[:, 1, 2] * (-2.0 * fy * cs[:, 1] / cz ** 3)
    if mutate != "no_jacobian":
        dcs = dcs + np.where(free[:, None], add, 0.0)
    position = (dcs @ u["view"])[:, :3]
    Gv = k["sc2"][:, None, None] * (np.transpose(T, (0, 2, 1)) @ DK @ T)
    off = 1.0 if mutate == "offdiag_not_doubled" else 2.0
    cov = np.stack([Gv[:, 0, 0], off * Gv[:, 0, 1], off * Gv[:, 0, 2], Gv[:, 1, 1], off * Gv[:, 1, 2], Gv[:, 2, 2]], axis=1)
    cov = np.where(free[:, None], cov, 0.0)
    return {"position": position, "covariance": cov, "norm": np.sqrt(gx * gx + gy * gy), "free": free}


def half_values(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(F64)


def spread_f64(q5, rec_bits, xyz, cov_bits, u, width, height, geometry_scale=1.0):
    """Rows as ws_geom_spread_rows takes them -> {"position", "covariance", "screen_norm", "seen"}; a row of five zeros adds nothing."""
    q5 = np.asarray(q5, dtype=np.int64)
    n = len(q5)
    h = half_values(rec_bits).reshape(n, 4)
    W, H = float(width), float(height)
    m00, m01, m10, m11 = h[:, 0] * W, h[:, 2] * W, -h[:, 1] * H, -h[:, 3] * H
    with np.errstate(all="ignore"):
        inv = SQRT_LOG2E / (m00 * m11 - m01 * m10)
        I = np.stack([np.stack([m11 * inv, -m01 * inv], axis=1), np.stack([-m10 * inv, m00 * inv], axis=1)], axis=1)
        q = q5.astype(F64) / (2.0 ** 32 * float(np.float32(geometry_scale)))
        got = chain_f64(q[:, :2], q[:, 2:], I, np.asarray(xyz, dtype=np.float32), half_values(cov_bits).reshape(n, 6), u, width, height)
    live = (q5 != 0).any(axis=1)
    z = lambda a: np.where(live.reshape((n,) + (1,) * (a.ndim - 1)), a, 0.0)
    return {"position": z(got["position"]), "covariance": z(got["covariance"]), "screen_norm": z(got["norm"]), "seen": live.astype(np.uint64)}


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def records_from_cloud(xyz, opacity, cov6, sh, u, width, height):
    """Continuous records of every Gaussian from k1_edges.k1_f64: pixel centre mu [n, 2], I' [n, 2, 2] (exp2 domain, from the
    unrounded v1, v2 by decode's expressions), colour [n, 3], opacity [n], depth w [n], and k1_f64's dict."""
    import k1_edges
    k = k1_edges.k1_f64(xyz, opacity, cov6, sh, u)
    W, H = float(width), float(height)
    v1, v2 = k["v1"], k["v2"]                                       # px, y up
    m00, m01, m10, m11 = v1[:, 0], v2[:, 0], -v1[:, 1], -v2[:, 1]
    inv = SQRT_LOG2E / (m00 * m11 - m01 * m10)
    I = np.stack([np.stack([m11 * inv, -m01 * inv], axis=1), np.stack([-m10 * inv, m00 * inv], axis=1)], axis=1)
    mu = np.stack([(k["centre"][:, 0] * 0.5 + 0.5) * W, (0.5 - k["centre"][:, 1] * 0.5) * H], axis=1)
    return {"mu": mu, "I": I, "colour": k["colour"], "opacity": k["opacity"], "w": k["w"], "k1": k}


def composite_f64(rec, order, G, background, width, height, sums=False):
    """The blend of continuous records in float64, near -> far in `order`, no early stop: L = sum_p G_rgb . F + G_T T_end, the
    kept and clamped verdict of every (record, pixel) pair, and -- sums=True -- the five sums per Gaussian by the definition of
    websplat.h (pairs on the clamp not counted; every Tb here is far above 2^-14, asserted)."""
    xs = np.arange(width)[None, :] + 0.5
    ys = np.arange(height)[:, None] + 0.5
    bg = np.asarray(background, dtype=F64)
    Gd = np.asarray(G, dtype=F64)
    n = len(order)
    T = np.ones((height, width))
    acc = np.zeros((height, width, 3))
    kept = np.zeros((len(rec["mu"]), height, width), dtype=bool)
    clamp = np.zeros_like(kept)
    steps = []
    for j in order:
        I, mu = rec["I"][j], rec["mu"][j]
        dx, dy = xs - mu[0], ys - mu[1]
        p0 = I[0, 0] * dx + I[0, 1] * dy
        p1 = I[1, 0] * dx + I[1, 1] * dy
        a2 = p0 * p0 + p1 * p1                                      # exp2 domain
        keep = a2 <= CUT_A * LOG2E
        b_raw = rec["opacity"][j] * np.exp2(-a2)
        kept[j], clamp[j] = keep, keep & (b_raw >= B_CLAMP)
        w = np.where(keep, np.minimum(B_CLAMP, b_raw) * T, 0.0)
        Tb = T
        T = Tb - w
        acc = acc + w[..., None] * rec["colour"][j]
        if sums:
            steps.append((j, p0, p1, w, Tb, T, acc.copy()))
    Fimg = acc + T[..., None] * bg
    out = {"L": float((Gd[..., :3] * Fimg).sum() + (Gd[..., 3] * T).sum()), "kept": kept, "clamped": clamp, "T_end": T}
    if sums:
        m, S = np.zeros((len(rec["mu"]), 2)), np.zeros((len(rec["mu"]), 3))
        for j, p0, p1, w, Tb, Ta, Pa in steps:
            counted = kept[j] & (w > 0) & ~clamp[j]
            assert (Tb[counted] >= 2.0 ** -10).all(), "the cloud of the finite differences must stay far from the stop"
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(counted, w / Ta, 0.0)
            d = r[..., None] * (Fimg - Pa) - w[..., None] * rec["colour"][j]
            kappa = np.where(counted, (Gd[..., :3] * d).sum(axis=-1) + Gd[..., 3] * r * T, 0.0)
            m[j] = (kappa * p0).sum(), (kappa * p1).sum()
            S[j] = (kappa * p0 * p0).sum(), (kappa * p0 * p1).sum(), (kappa * p1 * p1).sum()
        out["m"], out["S"] = m, S
    return out


def forward_from_cloud(xyz, opacity, cov6, sh, u, width, height, G, background, order=None):
    """L and the pairs' verdicts of the cloud under the uniforms u; order: the draw order to keep (default: by depth w, near first)."""
    rec = records_from_cloud(xyz, opacity, cov6, sh, u, width, height)
    if order is None:
        order = np.argsort(rec["w"], kind="stable")
    got = composite_f64(rec, order, G, background, width, height)
    got["order"] = order
    return got


def analytic_from_cloud(xyz, opacity, cov6, sh, u, width, height, G, background, mutate=None):
    """The chain of (b) on the float64 sums of the continuous records: dL/d position [n, 3], dL/d covariance [n, 6], free [n]."""
    rec = records_from_cloud(xyz, opacity, cov6, sh, u, width, height)
    order = np.argsort(rec["w"], kind="stable")
    got = composite_f64(rec, order, G, background, width, height, sums=True)
    out = chain_f64(got["m"], got["S"], rec["I"], xyz, cov6, u, width, height, mutate=mutate)
    out.update(order=order, m=got["m"], S=got["S"], lambda2_raw=rec["k1"]["lambda2_raw"], culled=rec["k1"]["culled"])
    return out
