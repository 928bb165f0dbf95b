"""The frames test_geometry_ref.py (CPU, oracle frames) and test_gpu_geometry.py (device frames) share beyond the isotropic stacks
and lines: what k_geometry's float64 reference is pointed at so that a wrong I', a partly filled quadrant, the 0.99 clamp and the
value cap can show.  Every function here takes a FRAME (dict of splats, sorted, src_index: blend_ref.oracle_frame's or
download_frame's) and is the same code for both tiers.

  general   attrib_frames._cloud_rows(): 3000 anisotropic Gaussians of random rotation, scales 0.01 - 0.08, opacities 0.02 - 0.3,
            under blend_ref's stack camera at 96 x 72 (3 x 2.25 tiles of 32 px): most of the cloud is culled, most visible records
            reach some quadrants only, many centres lie outside the viewport; plane = 0.5 signed_ramp, geometry_scale 0.25
  clamped   _stack(8, [1 - 1e-6] + [0.05] * 7) at 32 x 32: the front layer's core sits on the 0.99 clamp
  cap       _stack(3, 0.3) at 32 x 32 with geometry_scale 2^20: under the plane (1, 0, 0, 0) every value of every pair is far
            beyond the cap; under signed_ramp a pair or two per layer (where kappa changes sign) straddle it"""
import numpy as np

import geometry_ref as ref
import gradient_ref
import removal_ref
import weight_ref
from attrib_frames import BG, F, _cloud_rows, _stack
from gradient_frames import signed_ramp

GENERAL_VIEW = (96, 72)
GENERAL_PLANE_SCALE = 0.5
GENERAL_S = 0.25
GENERAL_MUTANTS = ("p_swapped", "iprime_transposed", "s01_negated")
TILE = (32, 32)
CLAMPED_K = 8
CLAMPED_S = (0.5, 8.0)
CAP_K = 3
CAP_S = 2.0 ** 20
MASK_CAP_GENERAL = 0.02     # share of undecided pixels masked out of the general frame's plane (test_gpu_gradient's cap)
MASK_CAP_OPEN = 0.05        # share of pixels with a pair that is not decidedly capped, masked out of the exact-cap plane


def general_rows():
    return _cloud_rows()


def clamped_rows():
    return _stack(CLAMPED_K, [1.0 - 1e-6] + [0.05] * (CLAMPED_K - 1))


def cap_rows():
    return _stack(CAP_K, 0.3)


def red_plane(width, height):
    """(1, 0, 0, 0) at every pixel."""
    g = np.zeros((height, width, 4), F)
    g[..., 0] = 1
    return g


def masked_ramp(frame, view, cap):
    """(signed_ramp with the undecided pixels of the frame zeroed, the share of pixels masked); the share is asserted <= cap."""
    w, h = view
    ok = ~removal_ref.undecided_mask(removal_ref.base_f64(frame, w, h, BG))
    share = 1.0 - float(ok.mean())
    assert share <= cap, f"{100 * share:.2f} % of the pixels are undecided"
    return (signed_ramp(w, h) * ok[..., None]).astype(F), share


def clamped_corner(frame, view, j=0):
    """H x W bool: the pixels at which Gaussian j's pair sits on the 0.99 clamp (clear of it by 4e-5 relative: no band pair) AND
    has p0 > 0 and p1 > 0.  A clamped pair has a' <= log2(1 / 0.99), |p| <= 0.12, and the core is symmetric about the centre:
    under a plane that covers the whole view the core's pairs are a thousandth of the S sums and cancel in m and S01, far inside
    any bound.  Under a plane that is 0 outside this mask Gaussian j's right sums are exactly 0 with tolerance 0, and a walk that
    counts clamped pairs adds values of one sign in every channel."""
    w, h = view
    halves = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    (slot,) = np.nonzero(frame["src_index"].astype(np.int64)[: len(halves)] == j)
    I, (cx, cy) = ref._iprime(halves[int(slot[0])], float(w), float(h))
    dx = np.arange(w)[None, :] + 0.5 - cx
    dy = np.arange(h)[:, None] + 0.5 - cy
    mask = np.zeros((h, w), dtype=bool)
    for jj, blk, a, keep, und, alpha in weight_ref.records(frame, w, h):
        if int(jj) == j:
            mask[blk] = keep & (np.exp(-a) * alpha >= ref.B_CLAMP * (1.0 + 4e-5))
    return mask & (I[0, 0] * dx + I[0, 1] * dy > 0) & (I[1, 0] * dx + I[1, 1] * dy > 0)


def stage_a(frame, view, n, g, s, plane_scale=1.0, mutate=None):
    return ref.stage_a_f64(frame, view[0], view[1], n, gradient_ref.plane_G(g, plane_scale), BG, geometry_scale=s, mutate=mutate)


def told_apart(sums, wrong, touched=None):
    """(share of the touched Gaussians with at least one of the five `sums` outside the bounds of the mutated reference `wrong`,
    their number, the per-channel outside mask).  touched: default the Gaussians with pairs in the mutated walk."""
    pick = (wrong["pairs"] > 0) if touched is None else touched
    outside = np.abs(sums - wrong["sum"]) > ref.bounds(wrong)
    return float(outside.any(axis=1)[pick].mean()), int(pick.sum()), outside


def exact_cap_plane(frame, view, n, plane):
    """The plane with the pixels masked at which the frame has a pair and channel that is not decidedly capped, and the reference
    under the masked plane: its tolerance is exactly 0, asserted, and so is the share masked (<= MASK_CAP_OPEN)."""
    first = stage_a(frame, view, n, plane, CAP_S)
    share = float(first["open_px"].mean())
    assert share <= MASK_CAP_OPEN, f"{100 * share:.2f} % of the pixels hold a pair that is not decidedly capped"
    g = (plane * ~first["open_px"][..., None]).astype(F)
    want = stage_a(frame, view, n, g, CAP_S) if share > 0 else first
    assert not want["open_px"].any() and not ref.bounds(want).any() and int(want["straddling"].sum()) == 0
    return g, want, share


def summary(q, want):
    """The figures of one compared case (a row of geometry_report.json): q the device's (or any) int64 sums."""
    tol = ref.bounds(want)
    got = q.astype(np.float64) / 2.0 ** 32
    d = np.abs(got - want["sum"])
    nz = np.abs(want["sum"]) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(nz, d / np.abs(want["sum"]), 0.0)
        tol_over = np.where(nz, tol / np.abs(want["sum"]), 0.0)
        used = np.where(tol > 0, d / tol, 0.0)
    met = want["pairs"] > 0   # (a Gaussian the walk never meets has five zeros on both sides and a bound of zero)
    return dict(gaussians=int(q.shape[0]), drawn=int((q != 0).any(axis=1).sum()), worst_excess=float((d - tol)[met].max()),
                largest_diff_over_bound=float(used.max()), largest_rel=float(rel.max()), median_tol_over_value=[float(np.median(tol_over[:, k][nz[:, k]])) if nz[:, k].any() else 0.0 for k in range(5)],
                band_pairs=int(want["band"].sum()), clamped_pairs=int(want["clamped"].sum()), capped=int(want["capped"].sum()),
                straddling=int(want["straddling"].sum()))
