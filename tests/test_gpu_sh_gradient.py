"""SH gradients (include/websplat.h "SH gradients"; sh_gradient.hip k_sh_spread): per Gaussian and frame, the colour sums of
k_gradient times the SH basis of the frame's view direction, added to every coefficient of a ws_shgrad.

   1. one frame, bit for bit against tests/sh_refit_ref.py, per cloud and active degree      4. signs, merging, reset
   2. wave and block edges                                                                   5. a finite difference on the device
   3. frames add; the scratch comes back clean                                               6. refusals"""
import numpy as np
import pytest

import scenes
import sh_refit_ref as ref
from attrib_frames import BG, F, _compressed, _ctx, _Frame
from gradient_frames import gradient, signed_ramp, splat_halves
from sh_frames import TILE, _cam32, _line, _oblique, _xyz
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

SMALL = (160, 120)


def _c1(ws, oracle, sh_deg, active, eye=None):
    """synth.scene_c1(n=2000) at 160 x 120 from synth.camera_c1's place (or from `eye`), the DC triple of every 50th Gaussian pushed
    to -2.5: 0.5 - 2.5 C0 is negative whatever the rest adds at these magnitudes, so every degree has colours on the clamp."""
    rows = synth.scene_c1(n=2000, seed=0, sh_deg=sh_deg)
    rows[::50, 6:9] = -2.5
    cj = synth.camera_c1(*SMALL) if eye is None else synth.look_at_camera(0, list(eye), [0.0, 0.0, 0.0], SMALL[0], SMALL[1], 320.0, 320.0)
    cj.fx = cj.fy = 2.0 * SMALL[0]   # (a focal length of two widths: about half of the cube is outside the frustum and culled)
    return scenes.Scene(ws, oracle, rows, sh_deg, cj, SMALL, max_sh_deg=active)


def _sh_gradient(f, plane, sh_deg, **kw):
    acc = f.ws.ShGrad(f.c, f.n, sh_deg)
    try:
        f.r.accumulate_sh_gradient(f.pc, acc, plane, **kw)
        assert acc.frames == 1 and acc.sh_deg == sh_deg and acc.num_points() == f.n
        return acc.download()
    finally:
        acc.close()


def _compare(f, args, plane, sh_deg, active):
    """ties (a) and the rest sums of one frame; returns (the ShGrad download, the Grad sums)"""
    got = _sh_gradient(f, plane, sh_deg, background=BG)
    q4 = gradient(f, plane)
    assert np.array_equal(got["sh"][:, 0, :], q4[:, :3]) and np.array_equal(got["opacity"], q4[:, 3]), "tie (a)"
    want_sh, want_o = ref.spread(q4, _xyz(f.pc), _cam32(args), active, sh_deg)
    bad = np.argwhere(got["sh"] != want_sh)
    assert bad.size == 0, f"{bad.shape[0]} rest sums differ, first at (Gaussian, coefficient, channel) {bad[0]}"
    assert np.array_equal(got["opacity"], want_o)
    nact = (min(sh_deg, active) + 1) ** 2
    assert not got["sh"][:, nact:, :].any(), "a coefficient above the active degree was touched"
    return got, q4


# ---- 1. one frame, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_deg,active", [(3, 3), (3, 1), (2, 2), (1, 1), (0, 0)])
def test_one_frame_bit_for_bit(ws, oracle, sh_deg, active):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, sh_deg, active)
        f = _Frame(ws, c, sc.gpc, sc.args)
        try:
            assert f.pc.sh_deg() == sh_deg
            got, q4 = _compare(f, sc.args, signed_ramp(*SMALL), sh_deg, active)
            rows = np.concatenate([got["sh"].reshape(f.n, -1), got["opacity"][:, None]], axis=1)
            nonzero = (rows != 0).any(axis=1)
            assert nonzero.sum() >= 500 and (~nonzero).sum() >= 100, (int(nonzero.sum()), int((~nonzero).sum()))
            colour = splat_halves(f.frame(), f.n)[:, 6:9]
            clamped = (colour == 0).any(axis=1)
            assert clamped.any(), "no Gaussian of the frame has a channel on the clamp"
            # a channel on the clamp has no sum in any coefficient (k_gradient counts none of its pairs)
            for ch in range(3):
                on = np.nan_to_num(colour[:, ch], nan=1.0) == 0
                assert not got["sh"][on, :, ch].any()
            if active > 0:
                seen = (got["sh"][:, 0, :] != 0).any(axis=1)
                assert ((got["sh"][seen, 1:(active + 1) ** 2, :] != 0).any(axis=(1, 2))).mean() > 0.95
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. wave and block edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_edges(ws, n):
    c = _ctx(ws)
    try:
        gpc, args = _oblique(ws, _line(n, 0.03), 3)
        f = _Frame(ws, c, gpc, args)
        try:
            assert f.r.frame_stats()["num_visible"] == n
            got, q4 = _compare(f, args, signed_ramp(*TILE), 3, 3)
            assert (q4 != 0).any(axis=1).all() and (got["sh"][:, 1:, :] != 0).any(axis=(1, 2)).all()   # every Gaussian, first and last included
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. frames add -----------------------------------------------------------------------------------------------------------------
def test_frames_add_and_the_scratch_comes_back_clean(ws, oracle):
    c = _ctx(ws)
    try:
        views = [_c1(ws, oracle, 3, 3), _c1(ws, oracle, 3, 3, eye=(2.2, -0.8, -1.9))]
        pc = ws.PointCloud(c, views[0].gpc)
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        r.enable_contrib(True)
        alone = [ws.ShGrad(c, n, 3) for _ in views]
        both = ws.ShGrad(c, n, 3)
        plane = signed_ramp(*SMALL)
        try:
            for sc, acc in zip(views, alone):
                r.prepare(pc, sc.args)
                r.accumulate_sh_gradient(pc, acc, plane, background=BG)
                r.accumulate_sh_gradient(pc, both, plane, background=BG)
            a, b, ab = alone[0].download(), alone[1].download(), both.download()
            assert both.frames == 2 and alone[0].frames == alone[1].frames == 1
            assert not np.array_equal(a["sh"], b["sh"]) and (a["sh"][:, 1:, :] != 0).any() and (b["sh"][:, 1:, :] != 0).any()
            assert np.array_equal(ab["sh"], a["sh"] + b["sh"]) and np.array_equal(ab["opacity"], a["opacity"] + b["opacity"]), "tie (b)"
            # a plane of zeros adds nothing -- neither of its own nor anything a frame before left in the scratch
            r.accumulate_sh_gradient(pc, both, np.zeros((SMALL[1], SMALL[0], 4), F), background=BG)
            z = both.download()
            assert both.frames == 3 and np.array_equal(z["sh"], ab["sh"]) and np.array_equal(z["opacity"], ab["opacity"])
            assert r.errors()[0] == 0
        finally:
            for acc in alone + [both]:
                acc.close()
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 4. signs and merging ------------------------------------------------------------------------------------------------------------
def test_signs_merging_and_reset(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, 3, 3)
        f = _Frame(ws, c, sc.gpc, sc.args)
        acc = ws.ShGrad(c, f.n, 3)
        try:
            plane = signed_ramp(*SMALL)
            pos = _sh_gradient(f, plane, 3, background=BG)
            neg = _sh_gradient(f, -plane, 3, background=BG)
            assert (pos["sh"] != 0).sum() > 10_000
            assert np.array_equal(neg["sh"], -pos["sh"]) and np.array_equal(neg["opacity"], -pos["opacity"]), "tie (c)"
            f.r.accumulate_sh_gradient(f.pc, acc, plane, background=BG)
            acc.add(**acc.download())
            twice = acc.download()
            assert np.array_equal(twice["sh"], 2 * pos["sh"]) and np.array_equal(twice["opacity"], 2 * pos["opacity"]) and acc.frames == 1
            acc.add(sh=neg["sh"])                 # either array alone
            acc.add(opacity=neg["opacity"])
            once = acc.download()
            assert np.array_equal(once["sh"], pos["sh"]) and np.array_equal(once["opacity"], pos["opacity"])
            acc.reset()
            zero = acc.download()
            assert not zero["sh"].any() and not zero["opacity"].any() and acc.frames == 0
            with pytest.raises(ValueError):
                acc.add(sh=pos["sh"][:, :4, :])
            with pytest.raises(ws.WebSplatError):
                acc.add(sh=pos["sh"][:-1])        # fewer rows than the accumulator has points
        finally:
            acc.close()
            f.close()
    finally:
        c.close()


# ---- 5. a finite difference on the device --------------------------------------------------------------------------------------------
def test_finite_difference_on_the_device(ws):
    """The frame is linear in a rest coefficient while the colour stays off the clamp: F(+0.25) - F(-0.25) = 0.5 basis_k w per
    pixel, so sum_p g dF = 0.5 sum / 2^32.  Allowed: the two clouds' colours are rounded to f16, below 2 an error of at most 2^-10
    each, 2^-9 together, weighted like the colour itself: 2^-9 sum_p w |G| of that Gaussian, from accumulate_weighted with |g| as
    the plane; and one unit of 2^-32 per pair for each of the two truncating accumulators (at most 1024 pairs)."""
    c = _ctx(ws, bin_request=0)
    try:
        g = signed_ramp(*TILE)
        zeros = np.zeros(TILE[::-1] + (4,), F)
        j = 1
        worst = 0.0
        for k in (1, 2, 3):
            ch = (k - 1) % 2   # (red, green, red: the ramp's blue component changes sign across the tile and its sum nearly cancels)
            rows = _line(4, 0.3, sh_deg=1)
            rows[:, 6:9] = np.random.default_rng(5).uniform(-0.2, 0.2, size=(4, 3)).astype(F)   # colours 0.5 +- 0.06 +- 0.13
            planes = []
            for delta in (0.0, 0.25, -0.25):
                moved = rows.copy()
                moved[j, 9 + ch * 3 + (k - 1)] = delta
                gpc, args = _oblique(ws, moved, 1, max_sh_deg=1)
                f = _Frame(ws, c, gpc, args)
                try:
                    colour = splat_halves(f.frame(), 4)[:, 6:9]
                    assert (colour > 0.3).all() and (colour < 0.7).all()
                    if delta == 0.0:
                        sums = _sh_gradient(f, g, 1, background=BG)["sh"]
                        weight, _ = f.weighted(np.abs(g[..., ch]))
                        bas = ref.basis(ref.direction(_xyz(f.pc), _cam32(args)))[j, k]
                        assert abs(float(bas)) > 0.1
                    else:
                        acc = ws.Grad(c, 4)
                        try:
                            f.r.accumulate_gradient(f.pc, acc, zeros, background=BG, base=True)   # (pass 1's image; nothing is added)
                        finally:
                            acc.close()
                        planes.append(f.r.download_removal_base().astype(np.float64))
                finally:
                    f.close()
            lhs = float((g[..., ch].astype(np.float64) * (planes[0][..., ch] - planes[1][..., ch])).sum())
            rhs = 0.5 * float(sums[j, k, ch]) / 2.0 ** 32
            allowed = 2.0 ** -9 * float(weight[j]) / 2.0 ** 32 + 2.0 * 1024 / 2.0 ** 32
            print(f"coefficient {k}, channel {ch}: sum g dF = {lhs:+.6f}, 0.5 sum / 2^32 = {rhs:+.6f}, gap {abs(lhs - rhs):.2e} (allowed {allowed:.2e})")
            assert abs(rhs) > 10 * allowed, "the derivative is too small for the comparison to say anything"
            assert abs(lhs - rhs) <= allowed
            worst = max(worst, abs(lhs - rhs) / allowed)
        print(f"largest gap: {worst:.3f} of the allowance")
    finally:
        c.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, 3, 3)
        f = _Frame(ws, c, sc.gpc, sc.args)
        gpc_c, args_c = _compressed(ws, n=3000)
        fc = _Frame(ws, c, gpc_c, args_c, compressed=True)
        plain = ws.GaussianRenderer(c, "rgba32float", 3, False)
        accs = dict(small=ws.ShGrad(c, f.n - 1, 3), low=ws.ShGrad(c, f.n, 2), good=ws.ShGrad(c, f.n, 3), packed=ws.ShGrad(c, fc.n, 3))
        plane = signed_ramp(*SMALL)
        try:
            def refused(r, pc, acc, code, text, p=plane):
                with pytest.raises(ws.WebSplatError) as e:
                    r.accumulate_sh_gradient(pc, acc, p, background=BG)
                assert e.value.code == code and text in str(e.value) and "ws_renderer_accumulate_sh_gradient" in str(e.value), str(e.value)

            refused(f.r, f.pc, accs["small"], L.WS_ERR_INVALID, "number of points")
            refused(f.r, f.pc, accs["low"], L.WS_ERR_INVALID, "SH degree")
            refused(fc.r, fc.pc, accs["packed"], L.WS_ERR_UNSUPPORTED, "compressed", p=signed_ramp(400, 300))
            plain.prepare(f.pc, sc.args)
            refused(plain, f.pc, accs["good"], L.WS_ERR_STATE, "enable_contrib")
            with pytest.raises(ws.WebSplatError) as e:
                ws.ShGrad(c, 10, 4)
            assert e.value.code == L.WS_ERR_UNSUPPORTED
            for acc in accs.values():
                got = acc.download()
                assert acc.frames == 0 and not got["sh"].any() and not got["opacity"].any()
        finally:
            for acc in accs.values():
                acc.close()
            plain.close()
            fc.close()
            f.close()
    finally:
        c.close()
