"""Gradients of an image loss (include/websplat.h "Gradients of an image loss"; gradient.hip k_gradient): dL/d(colour) and
dL/d(ln opacity) per Gaussian over a prepared frame.

   1. against float64 (tests/gradient_ref.py), faint stacks at the staging boundaries    6. a saturating stack
   2. against float64, a general cloud and a compressed one, masked where undecided      7. ws_image_error_gradient against numpy, bit for bit
   3. the bitwise ties: g / -g, mask + complement, against accumulate_weighted / _contrib 8. the scene driver and websplat_evaluate --gradient
   4. scale-one and tint-one on the device: rebuilt clouds against the sums              9. no pixel changes; the error cases
   5. clamps: the 0.99 core of an opaque splat, a colour channel on K1's clamp at 0

A module-scoped fixture writes one row per comparison (worst excess over bounds(), largest relative difference, median bound over
value) to gradient_report.json in WEBSPLAT_REPORT_DIR (default: test_reports/ under the repository root, as
tests/test_gpu_removal.py)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref
import gradient_ref
import removal_ref
import scenes
import weight_ref
from attrib_frames import BG, VIEW, F, _cloud_rows, _compressed, _ctx, _Frame, _stack, _stack_frame, _u32
from gradient_frames import gradient, signed_ramp, splat_halves
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = float(L.WS_GRAD_SUM_SCALE)
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "gradient_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _compare(case, q, ref, min_drawn=0):
    """Every one of the four sums of every Gaussian within bounds() of the float64 reference."""
    tol = gradient_ref.bounds(ref)
    s = q.astype(np.float64) / SCALE
    d = np.abs(s - ref["sum"])
    excess = d - tol
    i = np.unravel_index(int(np.argmax(excess)), excess.shape)
    nz = np.abs(ref["sum"]) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(nz, d / np.abs(ref["sum"]), 0.0)
        tol_over = np.where(nz, tol / np.abs(ref["sum"]), 0.0)
    drawn = int((q != 0).any(axis=1).sum())
    row = dict(case=case, gaussians=int(q.shape[0]), drawn=drawn, worst_excess=float(excess[i]), worst_excess_colour=float(excess[:, :3].max()),
               worst_excess_opacity=float(excess[:, 3].max()), largest_diff=float(d.max()), largest_rel_colour=float(rel[:, :3].max()),
               largest_rel_opacity=float(rel[:, 3].max()), median_tol_over_colour=float(np.median(tol_over[:, :3][nz[:, :3]])) if nz[:, :3].any() else 0.0,
               median_tol_over_opacity=float(np.median(tol_over[:, 3][nz[:, 3]])) if nz[:, 3].any() else 0.0, largest_a=float(ref["amax"]),
               band_pairs=int(ref["band"].sum()), clamped_pairs=int(ref["clamped"].sum()))
    REPORT.append(row)
    print(json.dumps(row))
    assert int(ref["U"].sum()) == 0, "a pair that counts at a pixel with an undecided pair: the plane has to mask it"
    assert drawn > min_drawn
    assert np.all(d <= tol), (f"{int((d > tol).sum())} sums out of bound, worst at Gaussian {i[0]} channel {i[1]}: got {s[i]:.9e} "
                             f"ref {ref['sum'][i]:.9e} tol {tol[i]:.3e}")
    return row


def _told_apart(case, q, frame, width, height, n, G, mutations, min_share=0.5, touched=None, **kw):
    """The device's opacity sums leave bounds() of every mutated reference for most Gaussians the mutation can touch."""
    s = q[:, 3].astype(np.float64) / SCALE
    for m in mutations:
        wrong = gradient_ref.gradient_f64(frame, width, height, n, G, BG, mutate=m, **kw)
        pick = (wrong["pairs"] > 0) if touched is None else touched
        share = float((np.abs(s - wrong["sum"][:, 3]) > gradient_ref.bounds(wrong)[:, 3])[pick].mean())
        print(f"{case}: under {m} {100 * share:.1f} % of {int(pick.sum())} Gaussians are out of bounds")
        REPORT.append(dict(case=case, mutation=m, gaussians=int(pick.sum()), share_out_of_bounds=share))
        assert share >= min_share, m


# ---- 1. faint stacks at the staging boundaries ---------------------------------------------------------------------------------
BOUNDARY_CASES = [({}, k) for k in (1, 512, 513, 1025)] + [({"tile_qw": 2, "tile_qh": 2}, k) for k in (256, 257)] + [({"tile_qw": 4, "tile_qh": 2}, 513)]


@pytest.mark.parametrize("cfg,k", BOUNDARY_CASES, ids=[f"{c.get('tile_qw', 4)}x{c.get('tile_qh', 4)}-{k}" for c, k in BOUNDARY_CASES])
def test_against_f64_faint_stacks_at_staging_boundaries(ws, cfg, k):
    """Tile lists of exactly k entries (STAGE = 512 at the 4x4 and 4x2 tiles, 256 at 2x2), every splat over the whole viewport:
    nothing saturates, no pair is near the cut-off or the clamp, no pixel is masked.  (a ~ 1e-3 here: opacity_scale 64 leaves it
    twenty bits above the 2^-32 grid.)"""
    c = _ctx(ws, bin_request=0, **cfg)
    try:
        f = _stack_frame(ws, c, k, 0.002)
        try:
            assert int(f.r.tile_stats()["list_len"].max()) == k
            frame = f.frame()
            g = signed_ramp(32, 32)
            q, base = gradient(f, g, opacity_scale=64.0, base=True)
            G = gradient_ref.plane_G(g)
            ref = gradient_ref.gradient_f64(frame, 32, 32, k, G, BG, opacity_scale=64.0)
            assert int(ref["und"].sum()) == 0 and int(ref["band"].sum()) == 0 and int(ref["clamped"].sum()) == 0 and ref["T"].min() > 2.0 ** -13
            case = f"1-{cfg.get('tile_qw', 4)}x{cfg.get('tile_qh', 4)}-k{k}"
            _compare(case, q, ref)
            assert np.all(q[:, 3] != 0) and np.all((q[:, :3] != 0).any(axis=1))
            tol_f, tol_t = removal_ref.base_bounds(ref)
            assert np.all(np.abs(base[..., :3].astype(np.float64) - ref["F"]).max(axis=-1) <= tol_f) and np.all(np.abs(base[..., 3] - ref["T"]) <= tol_t)
            if k in (1, 513, 257):
                _told_apart(case, q, frame, 32, 32, k, G, ("sign_flipped", "r_over_Tb"), opacity_scale=64.0)
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. a general cloud --------------------------------------------------------------------------------------------------------
OPACITY_COLUMN = 9 + 45
_REF = {}  # K1 and the depth sort do not depend on the tile configuration: one float64 walk serves the cases that share a frame


def _cloud_ref(f):
    """(frame, plane g, its mask, the float64 reference under it) of the general cloud's frame."""
    frame = f.frame()
    hit = _REF.get("cloud")
    if hit is None or not all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
        w, h = VIEW
        ok = ~removal_ref.undecided_mask(removal_ref.base_f64(frame, w, h, BG))
        assert 1.0 - ok.mean() <= 0.02
        g = (signed_ramp(w, h) * ok[..., None]).astype(F)
        hit = _REF["cloud"] = (frame, g, ok, gradient_ref.gradient_f64(frame, w, h, f.n, gradient_ref.plane_G(g, 0.5), BG, opacity_scale=0.25))
    return hit


F64_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}]
_ids = lambda cfgs: ["-".join(f"{k}{v}" for k, v in c.items()) or "default" for c in cfgs]  # noqa: E731


@pytest.mark.parametrize("cfg", F64_CONFIGS, ids=_ids(F64_CONFIGS))
def test_against_f64_general_cloud(ws, cfg):
    c = _ctx(ws, **cfg)
    try:
        f = _Frame(ws, c, *blend_ref.device_scene(ws, _cloud_rows(), VIEW))
        try:
            frame, g, ok, ref = _cloud_ref(f)
            q = gradient(f, g, scale=0.5, opacity_scale=0.25)
            case = "2-cloud-" + _ids([cfg])[0]
            _compare(case, q, ref, 1000)
            if not cfg:
                _told_apart(case, q, frame, *VIEW, f.n, gradient_ref.plane_G(g, 0.5), ("sign_flipped", "r_over_Tb"), opacity_scale=0.25)
        finally:
            f.close()
    finally:
        c.close()


def test_against_f64_compressed_cloud(ws):
    c = _ctx(ws)
    try:
        gpc, args = _compressed(ws, n=3000)
        f = _Frame(ws, c, gpc, args, compressed=True)
        try:
            frame = f.frame()
            ok = ~removal_ref.undecided_mask(removal_ref.base_f64(frame, 400, 300, BG))
            assert 1.0 - ok.mean() <= 0.02
            g = (signed_ramp(400, 300) * ok[..., None]).astype(F)
            q = gradient(f, g, opacity_scale=1.0 / 16)
            _compare("2-compressed", q, gradient_ref.gradient_f64(frame, 400, 300, f.n, gradient_ref.plane_G(g), BG, opacity_scale=1.0 / 16), 1000)
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. the bitwise ties -------------------------------------------------------------------------------------------------------
def _orbit_args(ws, gpc, index):
    cj = synth.orbit_cameras(5, VIEW[0], VIEW[1], float(VIEW[0]), float(VIEW[0]))[index]
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, cj.width, cj.height)
    cam.fit_near_far(gpc.aabb)
    return ws.SplattingArgs(camera=cam, viewport=VIEW, max_sh_deg=3)


def test_bitwise_ties(ws):
    c = _ctx(ws)
    try:
        rows = _cloud_rows()
        rows[::50, 6] = -3.0   # f_dc red: 0.5 + 0.28 f_dc < 0, clamped at 0 by K1 -- sixty Gaussians without a red gradient
        gpc, args = blend_ref.device_scene(ws, rows, VIEW)
        f = _Frame(ws, c, gpc, args)
        w, h = VIEW
        try:
            g = signed_ramp(w, h)
            q = gradient(f, g, opacity_scale=0.25)
            assert ((q != 0).all(axis=1)).sum() > 1000 and (q < 0).any(axis=0).all() and (q > 0).any(axis=0).all()
            # two runs are identical; (a) g and -g give exactly negated sums
            assert np.array_equal(gradient(f, g, opacity_scale=0.25), q)
            assert np.array_equal(gradient(f, -g, opacity_scale=0.25), -q)
            # (b) a 0/1 mask and its complement add up to the whole
            mask = np.zeros((h, w, 1), F)
            mask[9:150, 13:211] = 1
            for x, y in ((300, 200), (250, 3), (5, 233), (317, 239), (0, 0)):
                mask[y, x] = 1
            qa, qb = gradient(f, g * mask, opacity_scale=0.25), gradient(f, g * (1 - mask), opacity_scale=0.25)
            assert (qa != 0).any() and (qb != 0).any() and ((qa != 0) & (qb != 0)).any()
            assert np.array_equal(qa + qb, q)
            # (c) g = (E, 0, 0, 0) against accumulate_weighted, E == 1 against accumulate_contrib, where red is above 0 in the frame
            halves = splat_halves(f.frame(), f.n)
            red = halves[:, 6] > 0
            dark = halves[:, 6] == 0
            print(f"red above 0: {int(red.sum())}, red exactly 0 (K1's clamp): {int(dark.sum())}, not in the frame: {int(np.isnan(halves[:, 6]).sum())}")
            assert red.sum() > 1000 and dark.sum() > 10
            E = np.clip(0.5 + 0.5 * g[..., 1], 0, 1).astype(F)
            for plane, want in ((E, f.weighted(E)[0]), (np.ones((h, w), F), f.plain()[0])):
                ge = np.zeros((h, w, 4), F)
                ge[..., 0] = plane
                got = gradient(f, ge)
                assert np.array_equal(got[red, 0], want[red].astype(np.int64)) and (want[red] > 0).sum() > 1000
                assert not got[dark, 0].any() and (want[dark] > 0).any() and not got[:, 1:3].any() and got[:, 3].any()
            # ws_grad_add of two camera halves equals one accumulator
            both, first, second = (ws.Grad(c, f.n) for _ in range(3))
            try:
                for index, accs in ((0, (both, first)), (2, (both, second))):
                    f.r.prepare(f.pc, _orbit_args(ws, gpc, index))
                    for acc in accs:
                        f.r.accumulate_gradient(f.pc, acc, g, background=BG, opacity_scale=0.25)
                q1, q2, q12 = first.download(), second.download(), both.download()
                assert both.frames == 2 and not np.array_equal(q1, q2) and np.array_equal(q1 + q2, q12)
                first.add(q2)
                assert np.array_equal(first.download(), q12) and first.frames == 1
                first.reset()
                assert first.frames == 0 and not first.download().any()
            finally:
                for acc in (both, first, second):
                    acc.close()
        finally:
            f.close()
    finally:
        c.close()


# ---- 4. scale-one and tint-one on the device -----------------------------------------------------------------------------------
def test_scale_one_and_tint_one_on_the_device(ws):
    """The test that does not depend on the reference's formula: the base planes of the cloud with one Gaussian's opacity scaled,
    and with its colour moved, against the sums.  F is exactly affine in a common factor on the Gaussian's b and exactly linear in
    its colour, so any step is valid: sum_p G . (F' - F, T' - T) = (kappa - 1) opacity[j] and = sum_ch dc_ch colour[j][ch], with
    kappa and dc what K1 stored in the two frames' f16 Splat records."""
    c = _ctx(ws)
    w, h = VIEW
    try:
        rows = _cloud_rows()
        f = _Frame(ws, c, *blend_ref.device_scene(ws, rows, VIEW))
        frames = []
        try:
            frame, _, ok, _ = _cloud_ref(f)
            halves = splat_halves(frame, f.n)
            plain = f.plain()[0]
            logit = rows[:, OPACITY_COLUMN].astype(np.float64)
            alpha = 1.0 / (1.0 + np.exp(-logit))
            good = (plain > 0) & (alpha * 1.3 < 0.99) & (halves[:, 6:9] > 0.2).all(axis=1) & (halves[:, 6:9] < 0.8).all(axis=1)
            j = int(np.argmax(np.where(good, plain, 0)))
            assert good[j]
            scaled, tinted = rows.copy(), rows.copy()
            a1 = alpha[j] * 1.25
            scaled[j, OPACITY_COLUMN] = np.log(a1 / (1.0 - a1))
            tinted[j, 6:9] += np.array([0.4, -0.3, 0.25], F)
            refs = [removal_ref.base_f64(frame, w, h, BG)]
            for other in (scaled, tinted):
                fo = _Frame(ws, c, *blend_ref.device_scene(ws, other, VIEW))
                frames.append(fo)
                fr = fo.frame()
                assert np.array_equal(fr["sorted"], frame["sorted"]) and np.array_equal(fr["src_index"], frame["src_index"])
                refs.append(removal_ref.base_f64(fr, w, h, BG))
                ok = ok & ~removal_ref.undecided_mask(refs[-1])
            g = (signed_ramp(w, h) * ok[..., None]).astype(F)
            G = gradient_ref.plane_G(g).astype(np.float64)
            q, base = gradient(f, g, base=True)
            ref = gradient_ref.gradient_f64(frame, w, h, f.n, gradient_ref.plane_G(g), BG)
            assert int(ref["U"][j]) == 0 and int(ref["clamped"][j]) == 0
            s = q[j].astype(np.float64) / SCALE
            tol_own = gradient_ref.bounds(ref)[j]
            for name, fo, ref_o in (("scale", frames[0], refs[1]), ("tint", frames[1], refs[2])):
                _, base_o = gradient(fo, g, base=True)
                ho = splat_halves(fo.frame(), f.n)
                same = np.ones(10, bool)
                same[[9] if name == "scale" else [6, 7, 8]] = False
                assert np.array_equal(ho[j, same], halves[j, same]) and np.array_equal(np.delete(ho, j, 0), np.delete(halves, j, 0), equal_nan=True)
                touched = (np.abs(ref_o["F"] - refs[0]["F"]).max(axis=-1) > 0) | (ref_o["T"] != refs[0]["T"])
                assert np.array_equal(_u32(base_o[~touched]), _u32(base[~touched])), "a pixel j does not reach changed"
                dplane = base_o.astype(np.float64) - base.astype(np.float64)
                lhs = float((G * dplane)[touched].sum())
                tol_planes = 0.0
                for r_ in (refs[0], ref_o):
                    tol_f, tol_t = removal_ref.base_bounds(r_)
                    tol_planes += float(((np.abs(G[..., :3]).sum(axis=-1) * tol_f + np.abs(G[..., 3]) * tol_t) * touched).sum())
                if name == "scale":
                    kappa = ho[j, 9] / halves[j, 9]
                    rhs, tol = (kappa - 1.0) * s[3], abs(kappa - 1.0) * tol_own[3]
                    assert 1.1 < kappa < 1.4 and halves[j, 9] * kappa < 0.99
                else:
                    dc = ho[j, 6:9] - halves[j, 6:9]
                    rhs, tol = float((dc * s[:3]).sum()), float((np.abs(dc) * tol_own[:3]).sum())
                    assert (np.abs(dc) > 0.05).all() and (ho[j, 6:9] > 0).all()
                row = dict(case=f"4-{name}-one-{j}", planes=lhs, sums=rhs, diff=abs(lhs - rhs), allowance=tol + tol_planes, allowance_sums=tol,
                           pixels=int(touched.sum()))
                REPORT.append(row)
                print(json.dumps(row))
                assert abs(rhs) > 10 * (tol + tol_planes), "the step is too small to show anything"
                assert abs(lhs - rhs) <= tol + tol_planes
        finally:
            for fo in frames:
                fo.close()
            f.close()
    finally:
        c.close()


# ---- 5. clamps -----------------------------------------------------------------------------------------------------------------
def test_clamped_core_and_a_colour_on_the_clamp_at_zero(ws):
    """Eight layers over the whole 32 x 32 view; the front one has alpha 1, so b = 0.99 in its core (a <= 0.01: the few pixels
    around the centre) and every pair there is clamped: its opacity sum counts the rim only.  Layer 3 has a green of exactly 0."""
    c = _ctx(ws, bin_request=0)
    try:
        k = 8
        rows = _stack(k, [1.0 - 1e-6] + [0.05] * (k - 1))
        rows[3, 7] = -3.0   # f_dc green: 0.5 + 0.28 f_dc < 0, clamped at 0 by K1
        f = _Frame(ws, c, *blend_ref.device_scene(ws, rows, (32, 32)))
        try:
            frame = f.frame()
            halves = splat_halves(frame, k)
            assert halves[0, 9] == 1.0 and halves[3, 7] == 0.0 and (halves[:, 6] > 0).all()
            g = signed_ramp(32, 32)
            G = gradient_ref.plane_G(g)
            q = gradient(f, g, opacity_scale=0.5)
            ref = gradient_ref.gradient_f64(frame, 32, 32, k, G, BG, opacity_scale=0.5)
            print(f"clamped pairs per layer {ref['clamped'].tolist()}, band pairs {int(ref['band'].sum())}, largest |opacity_scale a| {ref['amax']:.3f}")
            assert 4 <= ref["clamped"][0] <= 16 and not ref["clamped"][1:].any() and int(ref["band"].sum()) == 0 and int(ref["und"].sum()) == 0
            assert ref["amax"] < 1.0   # (nothing reaches the cap)
            _compare("5-clamped-core", q, ref)
            _told_apart("5-clamped-core", q, frame, 32, 32, k, G, ("clamped_pairs_counted",), min_share=1.0, touched=ref["clamped"] > 0, opacity_scale=0.5)
            _told_apart("5-clamped-core", q, frame, 32, 32, k, G, ("sign_flipped",), opacity_scale=0.5)
            # the colour sums do not see the clamp: red of g = (1, 0, 0, 0) is the contribution sum, core included
            ones = np.zeros((32, 32, 4), F)
            ones[..., 0] = 1
            assert np.array_equal(gradient(f, ones)[:, 0], f.plain()[0].astype(np.int64))
            # green on K1's clamp: exactly nothing, whatever the plane; its other channels count
            assert q[3, 1] == 0 and q[3, 0] != 0 and q[3, 2] != 0 and q[3, 3] != 0 and np.all(q[[0, 1, 2, 4, 5, 6, 7], 1] != 0)
        finally:
            f.close()
    finally:
        c.close()


# ---- 6. saturation -------------------------------------------------------------------------------------------------------------
def test_saturating_stack(ws):
    """The opaque 32 x 32 stack with k = 513 (test_gpu_removal's): every quadrant saturates after a few layers and the walk and the
    batch loop take their early exits; what is walked behind the first all-saturated layer scores 0 in the opacity sum by the
    Tb >= 2^-14 rule and below 2^-32 per pair in the colour sums."""
    c = _ctx(ws, bin_request=0)
    try:
        f = _stack_frame(ws, c, 513, 0.9)
        try:
            frame = f.frame()
            g = signed_ramp(32, 32)
            G = gradient_ref.plane_G(g)
            q = gradient(f, g, opacity_scale=1.0 / 16)
            ref = gradient_ref.gradient_f64(frame, 32, 32, 513, G, BG, opacity_scale=1.0 / 16, saturating=True)
            assert int(ref["und"].sum()) == 0 and int(ref["clamped"].sum()) == 0
            _compare("6-saturating-513", q, ref)
            _told_apart("6-saturating-513", q, frame, 32, 32, 513, G, ("sign_flipped", "r_over_Tb"), touched=np.arange(513) < 3,
                        opacity_scale=1.0 / 16, saturating=True)
            T = np.ones((32, 32))
            first = None
            for i, (j, blk, a, keep, und, alpha) in enumerate(weight_ref.records(frame, 32, 32)):
                if first is None and T.max() < 2.0 ** -14:
                    first = i
                T[blk] -= weight_ref.weights(a, keep, alpha, T[blk])
            print(f"first all-saturated layer {first}; Gaussians with a non-zero sum {int((q != 0).any(axis=1).sum())}")
            assert first is not None and first + 8 < 513 and np.all(q[:first // 2, 3] != 0)
            assert not q[first + 8:].any()
            assert np.array_equal(gradient(f, g, opacity_scale=1.0 / 16), q)
        finally:
            f.close()
    finally:
        c.close()


# ---- 7. the loss gradient of the image error --------------------------------------------------------------------------------------
def _pixel_values(img, bg):
    """(value before the clamp, pixel value) H x W x 3 float32 of "Image metrics": three separately rounded f32 operations."""
    if img.dtype == np.uint8:
        v = img.astype(F) / F(255)
    else:
        v = img.astype(F)
    raw = v[..., :3]
    if bg is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            raw = raw + np.asarray(bg, F) * (F(1) - v[..., 3:4])
    with np.errstate(invalid="ignore"):
        val = np.where(np.isnan(raw), F(0), np.clip(raw, F(0), F(1))).astype(F)
    return raw.astype(F), val


def _error_gradient_numpy(a, b, bg_a, bg_b, kind):
    raw, x = _pixel_values(a, bg_a)
    _, y = _pixel_values(b, bg_b)
    d = x - y
    g = (F(2) * d) / F(3) if kind == "sq" else np.where(d == 0, F(0), np.copysign(F(1) / F(3), d)).astype(F)
    with np.errstate(invalid="ignore"):
        inside = (raw >= 0) & (raw <= 1)
    out = np.zeros(a.shape[:2] + (4,), F)
    out[..., :3] = np.where(inside, g, F(0))
    return out


@pytest.mark.parametrize("fmt_a,fmt_b", [(np.float32, np.uint8), (np.float16, np.float16), (np.uint8, np.float32)], ids=["f32-u8", "f16-f16", "u8-f32"])
def test_image_error_gradient_against_numpy_bit_for_bit(ws, fmt_a, fmt_b):
    c = _ctx(ws)
    w, h, pad = 33, 17, 3
    rng = np.random.default_rng(7)
    ptrs = []
    try:
        def image(dtype):
            if dtype == np.uint8:
                return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
            im = rng.uniform(-0.3, 1.3, size=(h, w, 4)).astype(dtype)
            im[2, 5, 1] = np.nan
            im[..., 3] = rng.uniform(0, 1, size=(h, w)).astype(dtype)
            im[4, 4] = (0.0, 1.0, 0.5, 1.0)    # opaque, exactly on the clamp's ends: inside
            return im
        a, b = image(fmt_a), image(fmt_b)
        b[7, 7] = a[7, 7] if fmt_a == fmt_b else b[7, 7]   # (d == 0 somewhere where the formats allow it)
        if fmt_b != np.uint8:
            b[4, 4, :3] = (0.5, 0.25, 0.75)   # (... and not where a sits on the clamp's ends)
        bg_a = None if fmt_a == np.uint8 else (0.2, 0.4, 0.1)
        bg_b = (0.3, 0.1, 0.6) if fmt_b == np.float16 else None
        views = []
        for im, bg in ((a, bg_a), (b, bg_b)):
            texel = im.itemsize * 4
            padded = np.zeros((h, w + pad, 4), im.dtype)
            padded[:, :w] = im
            ptrs.append(c.malloc(padded.nbytes))
            c.upload(ptrs[-1], padded)
            views.append(ws.ImageView(ptrs[-1], {1: "rgba8unorm", 2: "rgba16float", 4: "rgba32float"}[im.itemsize], (w + pad) * texel, bg).to_c())
        pitch = (w + 5) * 16
        ptrs.append(c.malloc(pitch * h))
        for kind in ("sq", "abs"):
            c.upload(ptrs[-1], np.full((h, w + 5, 4), -7.5, F))
            rc = ws.lib.ws_image_error_gradient(c.handle, C.byref(views[0]), C.byref(views[1]), w, h, ws.api.ERROR_KINDS[kind], 0, C.c_void_p(ptrs[-1]), pitch, None)
            assert rc == L.WS_OK, ws.lib.ws_last_error()
            c.sync()
            got = c.download(ptrs[-1], (h, w + 5, 4), F)
            want = _error_gradient_numpy(a, b, bg_a, bg_b, kind)
            assert np.array_equal(_u32(got[:, :w]), _u32(want)), kind
            assert np.all(got[:, w:] == F(-7.5)) and not got[:, :w, 3].any()
            raw, _ = _pixel_values(a, bg_a)
            with np.errstate(invalid="ignore"):
                outside = ~((raw >= 0) & (raw <= 1))
            assert not got[:, :w, :3][outside].any() and (fmt_a == np.uint8 or outside.sum() > 50) and (got[:, :w, :3] != 0).sum() > 500
            if fmt_a != np.uint8:
                assert np.isnan(raw[2, 5, 1]) and (got[4, 4, :3] != 0).all()
            # the python helper (tight pitches) agrees
            assert np.array_equal(_u32(ws.image_error_gradient(c, a, b, kind=kind, background_a=bg_a, background_b=bg_b)), _u32(want))
        # QUANTIZE_U8 is refused, and so are unknown flags, bad kinds and pitches
        def call(kind=0, flags=0, ptr=ptrs[-1], p=pitch):
            return ws.lib.ws_image_error_gradient(c.handle, C.byref(views[0]), C.byref(views[1]), w, h, kind, flags, C.c_void_p(ptr), p, None)
        assert call(flags=L.WS_METRICS_QUANTIZE_U8) == L.WS_ERR_INVALID and b"QUANTIZE" in ws.lib.ws_last_error()
        assert call(flags=2) == L.WS_ERR_INVALID and call(kind=L.WS_ERROR_DSSIM) == L.WS_ERR_INVALID
        assert call(p=w * 16 - 16) == L.WS_ERR_INVALID and call(p=w * 16 + 8) == L.WS_ERR_INVALID and call(ptr=ptrs[-1] + 4) == L.WS_ERR_INVALID
    finally:
        c.sync()
        for p in ptrs:
            c.free(p)
        c.close()


# ---- 8. the scene driver, the tool -------------------------------------------------------------------------------------------
SMALL = (160, 120)


def test_scene_driver_equals_the_manual_loop_and_the_tool_lists_it(ws, tmp_path):
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=10_000, seed=0)
        keep = np.arange(rows.shape[0]) % 3 != 2   # every third Gaussian dropped: the pruned cloud against its parent
        ply, sub_ply, cj = tmp_path / "parent.ply", tmp_path / "pruned.ply", tmp_path / "cameras.json"
        synth.write_ply(str(ply), rows)
        synth.write_ply(str(sub_ply), rows[keep])
        parent, pc = ws.PointCloud.load(c, str(ply)), ws.PointCloud.load(c, str(sub_ply))   # (the tool's own loader)
        n = pc.num_points()
        cams = synth.orbit_cameras(3, SMALL[0], SMALL[1], 150.0, 150.0, radius=3.0, height_off=0.4)
        text = json.dumps([cam.to_json() for cam in cams])
        scene = ws.Scene.from_json_text(text)
        driver, manual, scratch = (ws.Grad(c, n) for _ in range(3))
        r, rb = ws.GaussianRenderer(c, "rgba16float", pc.sh_deg(), False), ws.GaussianRenderer(c, "rgba16float", parent.sh_deg(), False)
        try:
            assert ws.accumulate_gradient_scene(c, pc, scene, None, driver, ref=parent, kind="sq") == 3 and driver.frames == 3
            bg = pc.background_color() or (0.0, 0.0, 0.0)
            r.enable_contrib(True)
            rb.set_blend_mode("target")
            for cam in scene.cameras(None):   # the frames of ws_render_views: ws_scene_accumulate_error's set-up
                args = lambda cloud: ws.SplattingArgs(camera=cam.to_perspective().fit_near_far(cloud.bbox()), viewport=SMALL,  # noqa: E731
                                                      max_sh_deg=cloud.sh_deg(), walltime=100.0)
                rb.prepare(parent, args(parent))
                rb.render(parent)
                b = rb.download_target()
                r.prepare(pc, args(pc))
                r.accumulate_gradient(pc, scratch, np.zeros((SMALL[1], SMALL[0], 4), F), background=bg, base=True)   # (pass 1's image)
                base = r.download_removal_base()
                plane = ws.image_error_gradient(c, base, b, kind="sq", background_b=bg)
                r.accumulate_gradient(pc, manual, plane, background=bg)
            assert r.errors()[0] == 0 and not scratch.download().any()
            qd, qm = driver.download(), manual.download()
            assert (qd != 0).all(axis=1).sum() > 1000 and np.array_equal(qd, qm)
            # the tool: the five largest |opacity gradient| of the test split, their four values, the count of all-zero Gaussians
            cj.write_text(text)
            exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
            out = subprocess.run([exe, str(sub_ply), str(cj), "--ref", str(ply), "--gradient", "5", "--split", "test"], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            head = [i for i, ln in enumerate(lines) if ln.startswith("gradient (sq error")]
            assert len(head) == 1 and "PSNR" in out.stdout
            driver.reset()
            frames = ws.accumulate_gradient_scene(c, pc, scene, "test", driver, ref=parent)
            qs = driver.download()
            assert f"over {frames} frames" in lines[head[0]]
            order = sorted(range(n), key=lambda i: (-abs(int(qs[i, 3])), i))[:5]
            for ln, i in zip(lines[head[0] + 2:head[0] + 7], order):
                cols = ln.split()
                assert int(cols[0]) == i
                want = qs[i, [3, 0, 1, 2]].astype(np.float64) / SCALE
                assert np.allclose([float(x) for x in cols[1:]], want, rtol=1e-8, atol=0)
            m = re.fullmatch(r"gradient: (\d+) of (\d+) drawn Gaussians have all four sums exactly 0", lines[-1])
            plain = ws.Contrib(c, n)
            try:
                ws.accumulate_contrib_scene(c, pc, scene, "test", plain)
                drawn = plain.download()[1] > 0
            finally:
                plain.close()
            assert m and int(m.group(2)) == int(drawn.sum()) and int(m.group(1)) == int((drawn & ~qs.any(axis=1)).sum())
            # the driver's own errors
            with pytest.raises(ws.WebSplatError) as e:
                ws.accumulate_gradient_scene(c, pc, scene, None, driver)
            assert e.value.code == L.WS_ERR_INVALID and "exactly one" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                ws.accumulate_gradient_scene(c, parent, scene, None, driver, ref=pc)
            assert e.value.code == L.WS_ERR_INVALID and "number of points" in str(e.value)
        finally:
            for a in (driver, manual, scratch):
                a.close()
            r.close()
            rb.close()
            scene.close()
            pc.close()
            parent.close()
    finally:
        c.close()


# ---- 9. no pixel changes; errors ---------------------------------------------------------------------------------------------------
def test_gradient_call_changes_no_pixel(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=VIEW)
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        acc = ws.Grad(c, pc.num_points())
        try:
            r.enable_contrib(True)
            r.prepare(pc, sc.args)
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            before = r.download_target().copy()
            r.accumulate_gradient(pc, acc, signed_ramp(*VIEW), background=BG, base=True)
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            after = r.download_target().copy()
            assert (before[..., 3] > 0.5).mean() > 0.05
            assert np.array_equal(_u32(before), _u32(after))
            assert acc.frames == 1 and (acc.download() != 0).all(axis=1).sum() > 1000
        finally:
            acc.close()
            r.close()
            pc.close()
    finally:
        c.close()


def test_error_cases_and_padded_pitches(ws):
    c = _ctx(ws)
    cut = _ctx(ws, debug_cut=2)
    try:
        gpc, args = blend_ref.device_scene(ws, _cloud_rows(), VIEW)
        pc, pc_cut = ws.PointCloud(c, gpc), ws.PointCloud(cut, gpc)
        n = pc.num_points()
        w, h = VIEW
        r, r_cut = ws.GaussianRenderer(c, "rgba32float", 3, False), ws.GaussianRenderer(cut, "rgba32float", 3, False)
        acc, small, acc_cut = ws.Grad(c, n), ws.Grad(c, n - 1), ws.Grad(cut, n)
        pad = 5
        d_base, d_plane = c.malloc((w + pad) * h * 16), c.malloc((w + pad) * h * 16 + 16)
        g = signed_ramp(w, h)

        def code_of(fn):
            with pytest.raises(ws.WebSplatError) as e:
                fn()
            assert "ws_renderer_accumulate_gradient" in str(e.value)
            return e.value.code

        try:
            # not prepared; prepared without contributions; another size; debug_cut
            r.enable_contrib(True)
            assert code_of(lambda: r.accumulate_gradient(pc, acc, g)) == L.WS_ERR_STATE
            r.enable_contrib(False)
            r.prepare(pc, args)
            assert code_of(lambda: r.accumulate_gradient(pc, acc, g)) == L.WS_ERR_STATE
            r.enable_contrib(True)
            r.prepare(pc, args)
            assert code_of(lambda: r.accumulate_gradient(pc, small, g)) == L.WS_ERR_INVALID
            r_cut.enable_contrib(True)
            r_cut.prepare(pc_cut, args)
            assert code_of(lambda: r_cut.accumulate_gradient(pc_cut, acc_cut, g)) == L.WS_ERR_UNSUPPORTED
            # pitches below the row, misaligned pitches and pointers
            assert code_of(lambda: r.accumulate_gradient(pc, acc, g, base_ptr=d_base, base_pitch=(w - 1) * 16)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, d_plane, plane_pitch=(w - 1) * 16)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, d_plane, plane_pitch=w * 16 + 8)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, d_plane + 4, plane_pitch=(w + pad) * 16)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, None, plane_pitch=(w + pad) * 16)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, g, scale=0.0)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_gradient(pc, acc, g, opacity_scale=float("inf"))) == L.WS_ERR_INVALID
            assert acc.frames == 0 and not acc.download().any()
            # padded rows are honoured: NaN behind the plane's rows is never read, a sentinel behind the base's never written; the
            # plane's values beyond +-1 are clamped, NaN inside the plane counts as 0
            plane = (g * F(1.5)).astype(F)
            plane[10, 20] = np.nan
            r.accumulate_gradient(pc, acc, plane, background=BG, opacity_scale=0.25, base=True)
            want_base, want_q = r.download_removal_base(), acc.download()
            assert (want_q != 0).all(axis=1).sum() > 1000
            clamped = np.clip(plane, -1, 1)
            clamped[10, 20] = 0
            acc.reset()
            r.accumulate_gradient(pc, acc, clamped, background=BG, opacity_scale=0.25)
            assert np.array_equal(acc.download(), want_q)
            acc.reset()
            padded = np.full((h, w + pad, 4), np.nan, F)
            padded[:, :w] = plane
            c.upload(d_plane, padded)
            c.upload(d_base, np.full((h, w + pad, 4), -7.5, F))
            r.accumulate_gradient(pc, acc, d_plane, plane_pitch=(w + pad) * 16, background=BG, opacity_scale=0.25, base_ptr=d_base, base_pitch=(w + pad) * 16)
            got = c.download(d_base, (h, w + pad, 4), F)
            assert np.array_equal(acc.download(), want_q) and acc.frames == 1
            assert np.array_equal(_u32(got[:, :w]), _u32(want_base)) and np.all(got[:, w:] == F(-7.5))
            # an all-zero plane adds nothing but counts as a frame
            r.accumulate_gradient(pc, acc, np.zeros((h, w, 4), F), background=BG)
            assert acc.frames == 2 and np.array_equal(acc.download(), want_q)
        finally:
            c.sync()
            c.free(d_base)
            c.free(d_plane)
            for a in (acc, small, acc_cut):
                a.close()
            r.close()
            r_cut.close()
            pc.close()
            pc_cut.close()
    finally:
        cut.close()
        c.close()
