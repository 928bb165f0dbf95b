"""Refitting the higher SH coefficients (include/websplat.h "Refitting colour and opacity", the rest coefficients; refit.hip
k_refit_step_sh): Adam steps on every SH half and the opacity of a resident cloud, in place, along a ShGrad's sums.

   1. the step, bit for bit against tests/sh_refit_ref.py, at wave and block edges and per degree     5. refusals
   2. the lr_sh = 0 tie with Refit.step                                                               6. the loop wins back a view-dependent error
   3. frozen groups, each alone, and the fixed point                                                  7. the scene driver, the tool, the saved file
   4. the clamps of the rest group

Test 6 writes its two loss trajectories to profiles/sh_refit/convergence.json."""
import json
import os
import subprocess

import numpy as np
import pytest

import refit_ref
import sh_refit_ref as ref
from attrib_frames import BG, F, _ctx, _u32
from sh_frames import EYE, TILE, _line, _oblique
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 2.0 ** -32
ADAM = dict(lr_colour=0.0025, lr_opacity=0.05, opacity_min=2.0 ** -7, lr_sh=0.002)   # (x is 0 or at least 2^-7: g / x stays far from overflow)


def _rows(n, seed, sh_deg=3, special=True):
    """test_gpu_refit._rows at any degree: random DC in [-1.5, 1.5], rest coefficients not zero, opacities in (0.01, 1); from 63
    Gaussians on, one opacity the row conversion takes to exactly 1.0 and one it takes to exactly 0."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(F)
    log_scale = rng.uniform(np.log(0.01), np.log(0.08), size=(n, 3)).astype(F)
    rot = rng.standard_normal(size=(n, 4)).astype(F)
    f_dc = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(F)
    f_rest = (rng.standard_normal(size=(n, 3 * (ref.ncoef(sh_deg) - 1))) * 0.1).astype(F)
    op = rng.uniform(0.01, 0.999, size=n)
    logit = np.log(op / (1.0 - op)).astype(F)
    if special and n >= 63:
        logit[5], logit[n - 2] = 30.0, -np.inf
    return synth._rows(xyz, f_dc, f_rest, logit, log_scale, rot)


def _cloud(ws, rows, sh_deg=3, seed=1):
    """The loader's blobs of the rows; the two bytes of padding beside every opacity and every SH half above the cloud's degree
    filled with noise (normal f16 values: K1 reads the whole record) -- no step may touch either."""
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, sh_deg)
    rng = np.random.default_rng(seed)
    n = rows.shape[0]
    gpc.gaussians[:, 14:16] = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    used = 3 * ref.ncoef(sh_deg)
    if used < 48:
        assert not gpc.sh_coefs[:, 2 * used:].any()
        noise = rng.uniform(-0.5, 0.5, size=(n, 48 - used)).astype(np.float16)
        gpc.sh_coefs[:, 2 * used:] = noise.view(np.uint8).reshape(n, -1)
    return gpc


def _sh16(s):
    """(N, 48) uint16: the 96-B SH records as halves"""
    return np.ascontiguousarray(s).view(np.uint16).reshape(s.shape[0], 48)


def _halves(g, s):
    """(N, 4) float16: the DC triple and the opacity as the blobs hold them."""
    dc = np.ascontiguousarray(s[:, :6]).view(np.float16)
    op = np.ascontiguousarray(g[:, 12:14]).view(np.float16)
    return np.concatenate([dc, op], axis=1)


def _rest(s, sh_deg):
    """(N, ncoef - 1, 3) float16: the rest coefficients as the blob holds them"""
    nc = ref.ncoef(sh_deg)
    return _sh16(s)[:, 3:3 * nc].view(np.float16).reshape(s.shape[0], nc - 1, 3)


def _elsewhere(g, s, sh_deg):
    """the blobs without the bytes a step may write: the opacity half and the first 3 ncoef SH halves"""
    return np.concatenate([g[:, :12], g[:, 14:], s[:, 6 * ref.ncoef(sh_deg):]], axis=1)


def _h16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _sums(rng, shape):
    """int64 sums shaped like test_gpu_refit._sums: magnitudes from 2^8 to 2^61 with up to 61 significant bits, both signs, exact zeros."""
    v = rng.integers(2 ** 60, 2 ** 61, size=shape, dtype=np.int64) >> rng.integers(0, 53, size=shape, dtype=np.int64)
    v *= rng.choice(np.array([-1, 1], np.int64), size=shape)
    v[rng.uniform(size=shape) < 0.1] = 0
    return v


def _same(got, st, keys=("master", "m", "v"), prefix=""):
    return all(np.array_equal(_u32(got[k]), _u32(getattr(st, prefix + k))) for k in keys)


class _Fit:
    """A context's cloud with its Refit (rest coefficients enabled), a ShGrad of its size and the numpy twin."""

    def __init__(self, ws, c, gpc, sh_deg=3, enable=True):
        self.sh_deg = sh_deg
        self.pc = ws.PointCloud(c, gpc)
        self.n = self.pc.num_points()
        self.refit = ws.Refit(c, self.pc)
        if enable:
            self.refit.enable_sh(self.pc)
        self.grad = ws.ShGrad(c, self.n, sh_deg)
        self.g0, self.s0 = self.pc.download()
        self.st = ref.ShState(_halves(self.g0, self.s0), _rest(self.s0, sh_deg))

    def load(self, q_sh, q_o):
        self.grad.reset()
        self.grad.add(sh=q_sh, opacity=q_o)

    def step(self, q_sh, q_o, trace=None, **adam):
        self.load(q_sh, q_o)
        self.refit.step_sh(self.pc, self.grad, colour_unit=UNIT, opacity_unit=UNIT, **adam)
        ref.step_sh(self.st, q_sh, q_o, UNIT, UNIT, trace=trace, **adam)
        return self.refit.download(), self.refit.download_sh()

    def agrees(self, got, got_sh):
        g1, s1 = self.pc.download()
        return (_same(got, self.st) and _same(got_sh, self.st, prefix="sh_")
                and np.array_equal(_h16(_halves(g1, s1)), _h16(self.st.halves()))
                and np.array_equal(_h16(_rest(s1, self.sh_deg)), _h16(self.st.rest_halves()))
                and np.array_equal(_elsewhere(g1, s1, self.sh_deg), _elsewhere(self.g0, self.s0, self.sh_deg)))

    def close(self):
        self.grad.close()
        self.refit.close()
        self.pc.close()


# ---- 1. the step, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_deg,n", [(3, 1), (3, 63), (3, 64), (3, 65), (3, 255), (3, 256), (3, 257), (3, 1000), (0, 257), (1, 257), (2, 257)])
def test_step_bit_for_bit_at_wave_and_block_edges(ws, sh_deg, n):
    c = _ctx(ws)
    try:
        gpc = _cloud(ws, _rows(n, 100 + n + sh_deg, sh_deg), sh_deg)
        f = _Fit(ws, c, gpc, sh_deg)
        try:
            nc = ref.ncoef(sh_deg)
            assert np.array_equal(f.g0, gpc.gaussians) and np.array_equal(f.s0, gpc.sh_coefs)
            got, got_sh = f.refit.download(), f.refit.download_sh()
            assert got_sh["master"].shape == (n, nc - 1, 3)
            assert np.array_equal(_u32(got_sh["master"]), _u32(_rest(f.s0, sh_deg).astype(F))) and not got_sh["m"].any() and not got_sh["v"].any()
            assert f.refit.steps == 0
            rng = np.random.default_rng(n + sh_deg)
            for k in range(5):
                q_sh, q_o = _sums(rng, (n, nc, 3)), _sums(rng, (n,))
                if n > 1:
                    assert (np.abs(q_sh) > 2 ** 53).any() and (q_sh == 0).any() and (q_sh < 0).any() and (q_sh > 0).any()
                trace = []
                got, got_sh = f.step(q_sh, q_o, trace=trace, **ADAM)
                assert refit_ref.all_zero_or_normal(trace), "the reference met a denormal, an infinity or a NaN: not pinned"
                assert f.refit.steps == k + 1 == f.st.steps
                assert _same(got, f.st), f"DC and opacity, step {k + 1}"
                assert _same(got_sh, f.st, prefix="sh_"), f"rest masters or moments, step {k + 1}"
                g1, s1 = f.pc.download()
                assert np.array_equal(_h16(_halves(g1, s1)), _h16(got["master"].astype(np.float16))), f"stored DC / opacity halves, step {k + 1}"
                assert np.array_equal(_h16(_rest(s1, sh_deg)), _h16(got_sh["master"].astype(np.float16))), f"stored rest halves, step {k + 1}"
                assert np.array_equal(_elsewhere(g1, s1, sh_deg), _elsewhere(f.g0, f.s0, sh_deg)), f"a byte outside the step's changed, step {k + 1}"
            assert not np.array_equal(_h16(_halves(g1, s1)), _h16(_halves(f.g0, f.s0)))
            if sh_deg:
                assert (_h16(_rest(s1, sh_deg)) != _h16(_rest(f.s0, sh_deg))).mean() > 0.5
            if sh_deg in (1, 2):   # the padding halves of the last plane the degree needs: 4 and 5 of them, noise, untouched
                used = 3 * nc
                pad = _sh16(s1)[:, used:8 * ((used + 7) // 8)]
                assert pad.shape[1] == {1: 4, 2: 5}[sh_deg] and pad.any() and np.array_equal(pad, _sh16(f.s0)[:, used:used + pad.shape[1]])
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. the lr_sh = 0 tie ------------------------------------------------------------------------------------------------------------
def test_frozen_rest_group_is_refit_step(ws):
    c = _ctx(ws)
    n = 300
    try:
        gpc = _cloud(ws, _rows(n, 7))
        a = _Fit(ws, c, gpc)
        pc_b = ws.PointCloud(c, gpc)
        fit_b, grad_b = ws.Refit(c, pc_b), ws.Grad(c, n)
        try:
            rng = np.random.default_rng(8)
            for _ in range(3):
                q_sh, q_o = _sums(rng, (n, 16, 3)), _sums(rng, (n,))
                got, got_sh = a.step(q_sh, q_o, **dict(ADAM, lr_sh=0.0))
                grad_b.reset()
                grad_b.add(np.concatenate([q_sh[:, 0, :], q_o[:, None]], axis=1))
                fit_b.step(pc_b, grad_b, colour_unit=UNIT, opacity_unit=UNIT, **{k: v for k, v in ADAM.items() if k != "lr_sh"})
                want = fit_b.download()
                assert all(np.array_equal(_u32(got[k]), _u32(want[k])) for k in want)
                (ga, sa), (gb, sb) = a.pc.download(), pc_b.download()
                assert np.array_equal(ga, gb) and np.array_equal(sa, sb)
                assert a.agrees(got, got_sh) and not got_sh["m"].any() and not got_sh["v"].any()
            assert a.refit.steps == fit_b.steps == 3 and not np.array_equal(sa[:, :6], a.s0[:, :6]) and np.array_equal(sa[:, 6:], a.s0[:, 6:])
        finally:
            grad_b.close()
            fit_b.close()
            pc_b.close()
            a.close()
    finally:
        c.close()


# ---- 3. frozen groups, the fixed point ------------------------------------------------------------------------------------------------
def test_frozen_groups_each_alone_and_the_fixed_point(ws):
    c = _ctx(ws)
    n = 300
    fits = []
    try:
        rng = np.random.default_rng(2)
        f = _Fit(ws, c, _cloud(ws, _rows(n, 21)))
        fits.append(f)
        off = dict(lr_colour=0.0, lr_opacity=0.0, lr_sh=0.0, opacity_min=2.0 ** -7)
        prev, prev_sh = f.refit.download(), f.refit.download_sh()
        gp, sp = f.g0, f.s0
        for group in ("lr_sh", "lr_colour", "lr_opacity"):
            got, got_sh = f.step(_sums(rng, (n, 16, 3)), _sums(rng, (n,)), **dict(off, **{group: 0.01}))
            g1, s1 = f.pc.download()
            assert f.agrees(got, got_sh), group
            dc_same = all(np.array_equal(_u32(got[k][:, :3]), _u32(prev[k][:, :3])) for k in got)
            op_same = all(np.array_equal(_u32(got[k][:, 3]), _u32(prev[k][:, 3])) for k in got)
            sh_same = all(np.array_equal(_u32(got_sh[k]), _u32(prev_sh[k])) for k in got_sh)
            assert (dc_same, op_same, sh_same) == (group != "lr_colour", group != "lr_opacity", group != "lr_sh"), group
            assert np.array_equal(g1, gp) == (group != "lr_opacity") and np.array_equal(s1[:, :6], sp[:, :6]) == (group != "lr_colour")
            assert np.array_equal(s1[:, 6:], sp[:, 6:]) == (group != "lr_sh")
            prev, prev_sh, gp, sp = got, got_sh, g1, s1
        # all sums 0 on a fresh object: every byte of the cloud and every master stays (opacity_min is not above any opacity)
        z = _Fit(ws, c, _cloud(ws, _rows(n, 22)))
        fits.append(z)
        got, got_sh = z.step(np.zeros((n, 16, 3), np.int64), np.zeros(n, np.int64), lr_colour=0.5, lr_opacity=0.5, lr_sh=0.5, opacity_min=0.0)
        gz, sz = z.pc.download()
        assert np.array_equal(gz, z.g0) and np.array_equal(sz, z.s0) and z.refit.steps == 1
        assert np.array_equal(_u32(got_sh["master"]), _u32(_rest(z.s0, 3).astype(F))) and not got_sh["m"].any() and not got_sh["v"].any()
        assert np.array_equal(_u32(got["master"]), _u32(_halves(z.g0, z.s0).astype(F))) and not got["m"].any()
        # ... and a Gaussian of zero sums among moving ones
        q_sh, q_o = _sums(rng, (n, 16, 3)), _sums(rng, (n,))
        still = np.arange(n) % 7 == 3
        q_sh[still], q_o[still] = 0, 0
        got2, got2_sh = z.step(q_sh, q_o, lr_colour=0.01, lr_opacity=0.01, lr_sh=0.01, opacity_min=0.0)
        g2, s2 = z.pc.download()
        assert z.agrees(got2, got2_sh)
        assert np.array_equal(_u32(got2_sh["master"][still]), _u32(got_sh["master"][still])) and not got2_sh["m"][still].any() and not got2_sh["v"][still].any()
        assert np.array_equal(g2[still], z.g0[still]) and np.array_equal(s2[still], z.s0[still])
        assert (got2_sh["master"][~still] != got_sh["master"][~still]).any(axis=(1, 2)).all()
    finally:
        for f in fits:
            f.close()
        c.close()


# ---- 4. the clamps -------------------------------------------------------------------------------------------------------------------
def test_clamps_of_the_rest_group(ws):
    c = _ctx(ws)
    n = 40
    try:
        f = _Fit(ws, c, _cloud(ws, _rows(n, 31, special=False)))
        try:
            up = np.arange(n) % 2 == 0
            q_sh = np.zeros((n, 16, 3), np.int64)
            q_sh[:, 1:, :] = np.where(up[:, None, None], -(2 ** 40), 2 ** 40)   # a negative gradient raises the coefficient
            got, got_sh = f.step(q_sh, np.zeros(n, np.int64), lr_colour=0.0, lr_opacity=0.0, lr_sh=1e6, opacity_min=0.0)
            assert f.agrees(got, got_sh)
            assert (got_sh["master"][up] == F(65504.0)).all() and (got_sh["master"][~up] == F(-65504.0)).all()
            _, s1 = f.pc.download()
            h = _h16(_rest(s1, 3))
            assert np.isfinite(_rest(s1, 3).astype(F)).all() and (h[up] == 0x7BFF).all() and (h[~up] == 0xFBFF).all()
            assert np.array_equal(s1[:, :6], f.s0[:, :6])
        finally:
            f.close()
    finally:
        c.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(ws):
    c = _ctx(ws)
    n = 64
    try:
        f = _Fit(ws, c, _cloud(ws, _rows(n, 41)), enable=False)
        other = ws.PointCloud(c, _cloud(ws, _rows(n, 42)))
        small, low, plain = ws.ShGrad(c, n - 1, 3), ws.ShGrad(c, n, 2), ws.Grad(c, n)
        late = ws.Refit(c, other)
        try:
            def refused(call, text):
                with pytest.raises(ws.WebSplatError) as e:
                    call()
                assert e.value.code == L.WS_ERR_INVALID and text in str(e.value), str(e.value)

            units = dict(colour_unit=UNIT, opacity_unit=UNIT)
            refused(lambda: f.refit.step_sh(f.pc, f.grad, **units), "ws_refit_enable_sh")       # before enable_sh
            refused(lambda: f.refit.download_sh(), "ws_refit_enable_sh")
            refused(lambda: f.refit.enable_sh(other), "created for")
            f.refit.enable_sh(f.pc)
            f.refit.enable_sh(f.pc)                                                          # a second call is a no-op
            refused(lambda: f.refit.step_sh(other, f.grad, **units), "created for")
            refused(lambda: f.refit.step_sh(f.pc, small, **units), "number of points")
            refused(lambda: f.refit.step_sh(f.pc, low, **units), "SH degree")
            refused(lambda: f.refit.step_sh(f.pc, f.grad, lr_sh=-1.0, **units), "lr_sh")
            with pytest.raises(ValueError):
                f.refit.step_sh(f.pc, f.grad)   # no frame in the accumulator and no unit given
            assert f.refit.steps == 0
            g, s = f.pc.download()
            assert np.array_equal(g, f.g0) and np.array_equal(s, f.s0)
            # enable_sh after a step: the powers are shared
            plain.add(np.ones((n, 4), np.int64))
            late.step(other, plain, **units)
            refused(lambda: late.enable_sh(other), "steps have been taken")
            # ... and the two steps may be mixed once the rest coefficients are in
            f.load(np.ones((n, 16, 3), np.int64) << 30, np.ones(n, np.int64) << 30)
            f.refit.step_sh(f.pc, f.grad, **units)
            f.refit.step(f.pc, plain, **units)
            assert f.refit.steps == 2
        finally:
            late.close()
            for a in (small, low, plain):
                a.close()
            other.close()
            f.close()
    finally:
        c.close()


# ---- 6. it does what it is for -----------------------------------------------------------------------------------------------------
STEPS = 30
OPACITY_SCALE = 1.0 / 128
RATES = dict(lr_colour=0.01, lr_opacity=0.005)
LR_SH = 0.02
EYES = (EYE, np.array([2.1, 0.9, -1.94], np.float64), np.array([0.3, -2.2, -2.02], np.float64))


def test_loop_wins_back_a_view_dependent_error(ws):
    """The four-layer stack at degree 1 under three cameras.  Target: the cloud with degree-1 coefficients of +-0.3; the fitted
    cloud starts with them 0 and everything else equal.  The same number of steps twice from that start: DC + opacity only
    (Refit.step) and with the rest coefficients (Refit.step_sh).  The SH run ends strictly below its start and strictly below the
    DC-only run; at every step its masters are the reference's, fed with the device's own sums.  The figures are recorded."""
    c = _ctx(ws, bin_request=0)
    try:
        rows = _line(4, 0.3, sh_deg=1, length=0.3)   # (short: in view from all three cameras)
        rows[:, 6:9] = np.random.default_rng(5).uniform(-0.2, 0.2, size=(4, 3)).astype(F)
        target_rows = rows.copy()
        target_rows[:, 9:18] = np.random.default_rng(6).choice(np.array([-0.3, 0.3], F), size=(4, 9))
        views = [_oblique(ws, rows, 1, max_sh_deg=1, eye=eye)[1] for eye in EYES]
        gpc_t = ws.GenericGaussianPointCloud.from_ply_rows(target_rows, 1)
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 1)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        r.enable_contrib(True)
        scratch = ws.Grad(c, 4)
        zeros = np.zeros(TILE[::-1] + (4,), F)

        def base_of(pc, args):
            r.prepare(pc, args)
            r.accumulate_gradient(pc, scratch, zeros, background=BG, base=True)   # (pass 1's image; nothing is added)
            return r.download_removal_base()

        pc_t = ws.PointCloud(c, gpc_t)
        targets = [base_of(pc_t, a) for a in views]
        pc_t.close()
        loss = lambda pc: sum(float(((base_of(pc, a)[..., :3].astype(np.float64) - t[..., :3].astype(np.float64)) ** 2).sum())  # noqa: E731
                              for a, t in zip(views, targets))
        cu = 1.0 / (L.WS_GRAD_SUM_SCALE * len(views))
        ou = 1.0 / (L.WS_GRAD_SUM_SCALE * float(F(OPACITY_SCALE)) * len(views))
        runs = {}
        mismatches = []
        for name in ("dc_only", "sh"):
            pc = ws.PointCloud(c, gpc)
            fit = ws.Refit(c, pc)
            grad = ws.ShGrad(c, 4, 1) if name == "sh" else ws.Grad(c, 4)
            g0, s0 = pc.download()
            st = ref.ShState(_halves(g0, s0), _rest(s0, 1))
            if name == "sh":
                fit.enable_sh(pc)
            losses = []
            try:
                for k in range(STEPS):
                    losses.append(loss(pc))
                    grad.reset()
                    for a, t in zip(views, targets):
                        plane = ws.image_error_gradient(c, base_of(pc, a), t, kind="sq")
                        if name == "sh":
                            r.accumulate_sh_gradient(pc, grad, plane, background=BG, opacity_scale=OPACITY_SCALE)
                        else:
                            r.accumulate_gradient(pc, grad, plane, background=BG, opacity_scale=OPACITY_SCALE)
                    assert grad.frames == len(views)
                    if name == "sh":
                        q = grad.download()
                        fit.step_sh(pc, grad, lr_sh=LR_SH, opacity_scale=OPACITY_SCALE, **RATES)   # (the units: three frames, these scales)
                        ref.step_sh(st, q["sh"], q["opacity"], cu, ou, lr_sh=LR_SH, **RATES)
                        if not (_same(fit.download(), st) and _same(fit.download_sh(), st, prefix="sh_")):
                            mismatches.append(k + 1)
                    else:
                        fit.step(pc, grad, opacity_scale=OPACITY_SCALE, **RATES)
                losses.append(loss(pc))
                runs[name] = losses
                assert fit.steps == STEPS
            finally:
                grad.close()
                fit.close()
                pc.close()
        assert not scratch.download().any()
        scratch.close()
        r.close()
        sh, dc = runs["sh"], runs["dc_only"]
        out = os.path.join(ROOT, "profiles", "sh_refit")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "convergence.json"), "w") as fh:
            json.dump(dict(scene="four isotropic Gaussians on a line at 32x32, degree 1, three cameras; target: rest coefficients of +-0.3, start: 0",
                           steps=STEPS, lr_sh=LR_SH, opacity_scale=OPACITY_SCALE, views=len(views), **RATES,
                           loss="sum over views, pixels and colour channels of (base - target)^2, float64",
                           start=sh[0], sh_after=sh[-1], dc_only_after=dc[-1], sh_ratio=sh[-1] / sh[0], dc_only_ratio=dc[-1] / dc[0],
                           sh_over_dc_only=sh[-1] / dc[-1], trajectory_sh=sh, trajectory_dc_only=dc), fh, indent=1)
        print(f"loss at the start {sh[0]:.6f}; after {STEPS} steps: DC + opacity only {dc[-1]:.6f}, with the rest coefficients {sh[-1]:.6f} "
              f"(ratio {sh[-1] / dc[-1]:.4f})")
        assert mismatches == [], f"masters differ from the reference after steps {mismatches}"
        assert sh[0] == dc[0] > 0 and sh[-1] < sh[0] and sh[-1] < dc[-1]
    finally:
        c.close()


# ---- 7. the scene driver, the tool, the file -------------------------------------------------------------------------------------------
SMALL = (160, 120)


def test_scene_driver_equals_the_manual_loop_the_tool_refits_and_saves(ws, tmp_path):
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=2000, seed=0)
        keep = np.arange(rows.shape[0]) % 4 != 3   # 1 500 of the 2 000: the pruned cloud against its parent
        ply, sub_ply, cj, saved = tmp_path / "parent.ply", tmp_path / "pruned.ply", tmp_path / "cameras.json", tmp_path / "refitted.ply"
        synth.write_ply(str(ply), rows)
        synth.write_ply(str(sub_ply), rows[keep])
        parent = ws.PointCloud.load(c, str(ply))   # (the tool's own loader)
        pcs = [ws.PointCloud.load(c, str(sub_ply)) for _ in range(2)]
        n = pcs[0].num_points()
        cams = synth.orbit_cameras(6, SMALL[0], SMALL[1], 150.0, 150.0, radius=3.0, height_off=0.4)   # file position 0 is the test camera
        text = json.dumps([cam.to_json() for cam in cams])
        scene = ws.Scene.from_json_text(text)
        fits = [ws.Refit(c, pc) for pc in pcs]
        grad, scratch = ws.ShGrad(c, n, 3), ws.Grad(c, n)
        r, rb = ws.GaussianRenderer(c, "rgba16float", 3, False), ws.GaussianRenderer(c, "rgba16float", 3, False)
        adam = dict(lr_colour=0.005, lr_opacity=0.01, lr_sh=0.00025)
        try:
            # (the driver enables the rest coefficients itself)
            assert ws.refit_scene(c, pcs[0], scene, "train", fits[0], ref=parent, epochs=2, views_per_step=2, sh=True, **adam) == 6 and fits[0].steps == 6
            pc, fit = pcs[1], fits[1]
            fit.enable_sh(pc)
            bg = pc.background_color() or (0.0, 0.0, 0.0)
            r.enable_contrib(True)
            rb.set_blend_mode("target")
            train = scene.cameras("train")
            for _ in range(2):
                for i, cam in enumerate(train):
                    args = lambda cloud: ws.SplattingArgs(camera=cam.to_perspective().fit_near_far(cloud.bbox()), viewport=SMALL,  # noqa: E731
                                                          max_sh_deg=cloud.sh_deg(), walltime=100.0)
                    rb.prepare(parent, args(parent))
                    rb.render(parent)
                    b = rb.download_target()
                    r.prepare(pc, args(pc))
                    r.accumulate_gradient(pc, scratch, np.zeros((SMALL[1], SMALL[0], 4), F), background=bg, base=True)   # (pass 1's image)
                    plane = ws.image_error_gradient(c, r.download_removal_base(), b, kind="sq", background_b=bg)
                    r.accumulate_sh_gradient(pc, grad, plane, background=bg, opacity_scale=1.0 / 128)
                    if grad.frames == 2 or i == len(train) - 1:
                        fit.step_sh(pc, grad, opacity_scale=1.0 / 128, **adam)
                        grad.reset()
            assert r.errors()[0] == 0 and fit.steps == 6
            (gd, sd), (gm, sm) = pcs[0].download(), pcs[1].download()
            d, m = fits[0].download(), fits[1].download()
            dsh, msh = fits[0].download_sh(), fits[1].download_sh()
            assert all(np.array_equal(_u32(d[k]), _u32(m[k])) for k in d) and all(np.array_equal(_u32(dsh[k]), _u32(msh[k])) for k in dsh)
            assert (dsh["v"] != 0).any(axis=(1, 2)).sum() > 500
            assert np.array_equal(gd, gm) and np.array_equal(sd, sm)
            fresh = ws.PointCloud.load(c, str(sub_ply))
            try:
                g0, s0 = fresh.download()
            finally:
                fresh.close()
            assert np.array_equal(_elsewhere(gd, sd, 3), _elsewhere(g0, s0, 3)) and (_sh16(sd)[:, 3:] != _sh16(s0)[:, 3:]).any(axis=1).sum() > 500
            with pytest.raises(ValueError):
                ws.refit_scene(c, pcs[0], scene, "train", fits[0], ref=parent, lr_sh=0.1)   # lr_sh without sh=True
            # the tool: the table, the refit on the train split, the table again, the file
            cj.write_text(text)
            exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
            out = subprocess.run([exe, str(sub_ply), str(cj), "--ref", str(ply), "--refit", "2", "--views-per-step", "2", "--lr-colour", "0.005",
                                  "--refit-sh", "--lr-sh", "0.00025", "--save", str(saved)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            means = [i for i, ln in enumerate(lines) if ln.startswith("mean over 1 images: PSNR")]
            after = [i for i, ln in enumerate(lines) if ln.startswith("after refit:")]
            print(out.stdout)
            assert len(means) == 2 and len(after) == 1 and means[0] < after[0] < means[1]
            assert lines[after[0]] == "after refit: 2 epochs, 6 steps, SH degree 3"
            assert lines[means[0] - 1].split()[:2] == lines[means[1] - 1].split()[:2] and lines[means[0]] != lines[means[1]]
            assert lines[-1].startswith(f"saved {saved}: 1500 Gaussians")
            back = ws.PointCloud.load(c, str(saved))
            try:
                gs, ss = back.download()
            finally:
                back.close()
            assert np.array_equal(ss, sd) and np.array_equal(gs[:, 12:14], gd[:, 12:14]), "the saved file does not hold the refitted halves"
            # --lr-sh without --refit-sh is a usage error
            out = subprocess.run([exe, str(sub_ply), str(cj), "--ref", str(ply), "--refit", "1", "--lr-sh", "0.1"], capture_output=True, text=True, timeout=120)
            assert out.returncode == 2 and "usage" in out.stderr
        finally:
            for a in fits + [grad, scratch]:
                a.close()
            r.close()
            rb.close()
            scene.close()
            for pc in pcs:
                pc.close()
            parent.close()
    finally:
        c.close()
