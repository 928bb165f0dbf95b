"""Refitting colour and opacity (include/websplat.h "Refitting colour and opacity"; refit.hip k_refit_step): Adam steps on the DC
colours and the opacities of a resident cloud, in place.

   1. the step, bit for bit against tests/refit_ref.py, at wave and block edges      5. the loop lowers the loss it descends
   2. frozen groups and the fixed point                                              6. the scene driver equals the manual loop; the tool
   3. the clamps                                                                     7. a refitted cloud survives download + re-creation
   4. refusals on the device                                                            and subsetting

Test 5 writes its loss trajectory to profiles/refit/convergence.json."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import blend_ref
import refit_ref
from attrib_frames import BG, F, _compressed, _ctx, _stack, _u32
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPACITY_COLUMN = 9 + 45
UNIT = 2.0 ** -32
ADAM = dict(lr_colour=0.0025, lr_opacity=0.05, opacity_min=2.0 ** -7)   # (x is 0 or at least 2^-7: g / x stays far from overflow)


def _rows(n, seed, special=True):
    """Random DC in [-1.5, 1.5], the higher SH coefficients not zero, opacities in (0.01, 1); from 63 Gaussians on, one opacity that
    the row conversion takes to exactly 1.0 and one it takes to exactly 0."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(F)
    log_scale = rng.uniform(np.log(0.01), np.log(0.08), size=(n, 3)).astype(F)
    rot = rng.standard_normal(size=(n, 4)).astype(F)
    f_dc = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(F)
    f_rest = (rng.standard_normal(size=(n, 45)) * 0.1).astype(F)
    op = rng.uniform(0.01, 0.999, size=n)
    logit = np.log(op / (1.0 - op)).astype(F)
    if special and n >= 63:
        logit[5], logit[n - 2] = 30.0, -np.inf
    return synth._rows(xyz, f_dc, f_rest, logit, log_scale, rot)


def _cloud(ws, rows, seed=1):
    """The loader's blobs of the rows, the two bytes of padding beside every opacity filled with noise."""
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 3)
    gpc.gaussians[:, 14:16] = np.random.default_rng(seed).integers(0, 256, size=(rows.shape[0], 2), dtype=np.uint8)
    return gpc


def _halves(g, s):
    """(N, 4) float16: the DC triple and the opacity as the blobs hold them."""
    dc = np.ascontiguousarray(s[:, :6]).view(np.float16)
    op = np.ascontiguousarray(g[:, 12:14]).view(np.float16)
    return np.concatenate([dc, op], axis=1)


def _h16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _elsewhere(g, s):
    """the blobs without the 8 bytes a step may write"""
    return np.concatenate([g[:, :12], g[:, 14:], s[:, 6:]], axis=1)


def _sums(rng, n):
    """(N, 4) int64: magnitudes from 2^8 to 2^61 with up to 61 significant bits (int64 -> double rounds), both signs, exact zeros."""
    v = rng.integers(2 ** 60, 2 ** 61, size=(n, 4), dtype=np.int64) >> rng.integers(0, 53, size=(n, 4), dtype=np.int64)
    v *= rng.choice(np.array([-1, 1], np.int64), size=(n, 4))
    v[rng.uniform(size=(n, 4)) < 0.1] = 0
    return v


def _load(grad, q):
    grad.reset()
    grad.add(q)


def _same_state(got, st):
    return all(np.array_equal(_u32(got[k]), _u32(getattr(st, k))) for k in ("master", "m", "v"))


class _Fit:
    """A context's cloud with its Refit, a Grad of its size and the numpy twin of the Refit."""

    def __init__(self, ws, c, gpc):
        self.pc = ws.PointCloud(c, gpc)
        self.n = self.pc.num_points()
        self.refit = ws.Refit(c, self.pc)
        self.grad = ws.Grad(c, self.n)
        self.g0, self.s0 = self.pc.download()
        self.st = refit_ref.State(_halves(self.g0, self.s0))

    def step(self, q, trace=None, **adam):
        _load(self.grad, q)
        self.refit.step(self.pc, self.grad, colour_unit=UNIT, opacity_unit=UNIT, **adam)
        refit_ref.step(self.st, q, UNIT, UNIT, trace=trace, **adam)
        return self.refit.download()

    def close(self):
        self.grad.close()
        self.refit.close()
        self.pc.close()


# ---- 1. the step, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_step_bit_for_bit_at_wave_and_block_edges(ws, n):
    c = _ctx(ws)
    try:
        gpc = _cloud(ws, _rows(n, 100 + n))
        f = _Fit(ws, c, gpc)
        try:
            assert np.array_equal(f.g0, gpc.gaussians) and np.array_equal(f.s0, gpc.sh_coefs)
            h0 = _halves(f.g0, f.s0)
            if n >= 63:   # the row conversion takes a logit of 30 to exactly 1.0 and one of -inf to exactly 0 (+0.0)
                assert _h16(h0)[5, 3] == 0x3C00 and _h16(h0)[n - 2, 3] == 0x0000
            got = f.refit.download()
            assert np.array_equal(_u32(got["master"]), _u32(h0.astype(F))) and not got["m"].any() and not got["v"].any() and f.refit.steps == 0
            rng = np.random.default_rng(n)
            for k in range(5):
                q = _sums(rng, n)
                if n > 1:
                    assert (np.abs(q) > 2 ** 53).any() and (q == 0).any() and (q < 0).any() and (q > 0).any()
                trace = []
                got = f.step(q, trace=trace, **ADAM)
                assert refit_ref.all_zero_or_normal(trace), "the reference met a denormal, an infinity or a NaN: not pinned"
                assert f.refit.steps == k + 1 == f.st.steps
                assert _same_state(got, f.st), f"step {k + 1}"
                g1, s1 = f.pc.download()
                assert np.array_equal(_h16(_halves(g1, s1)), _h16(got["master"].astype(np.float16))), f"stored halves, step {k + 1}"
                assert np.array_equal(_elsewhere(g1, s1), _elsewhere(f.g0, f.s0)), f"a byte outside the eight changed, step {k + 1}"
            assert not np.array_equal(_h16(_halves(g1, s1)), _h16(h0))
            if n >= 63:
                assert (got["master"][:, 3] == F(2.0 ** -7)).any()   # (the lower clamp was met)
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. frozen groups, the fixed point ------------------------------------------------------------------------------------------------
def test_frozen_groups_and_the_fixed_point(ws):
    c = _ctx(ws)
    n = 300
    fits = []
    try:
        rng = np.random.default_rng(2)
        f = _Fit(ws, c, _cloud(ws, _rows(n, 21)))
        fits.append(f)
        start = f.refit.download()
        # colour frozen: opacity moves alone
        a = f.step(_sums(rng, n), **dict(ADAM, lr_colour=0.0))
        ga, sa = f.pc.download()
        assert _same_state(a, f.st)
        for k in ("master", "m", "v"):
            assert np.array_equal(_u32(a[k][:, :3]), _u32(start[k][:, :3]))
        assert np.array_equal(sa, f.s0) and (a["master"][:, 3] != start["master"][:, 3]).sum() > n // 2 and a["v"][:, 3].any()
        assert not np.array_equal(ga[:, 12:14], f.g0[:, 12:14])
        # opacity frozen: colour moves alone
        b = f.step(_sums(rng, n), **dict(ADAM, lr_opacity=0.0))
        gb, sb = f.pc.download()
        assert _same_state(b, f.st)
        for k in ("master", "m", "v"):
            assert np.array_equal(_u32(b[k][:, 3]), _u32(a[k][:, 3]))
        assert np.array_equal(gb, ga) and (b["master"][:, :3] != a["master"][:, :3]).sum() > n and not np.array_equal(sb[:, :6], sa[:, :6])
        assert np.array_equal(_elsewhere(gb, sb), _elsewhere(f.g0, f.s0))
        # all sums 0 on a fresh object: every byte of the cloud and every master stays (opacity_min is not above any opacity)
        z = _Fit(ws, c, _cloud(ws, _rows(n, 22)))
        fits.append(z)
        got = z.step(np.zeros((n, 4), np.int64), lr_colour=0.5, lr_opacity=0.5, opacity_min=0.0)
        gz, sz = z.pc.download()
        assert np.array_equal(gz, z.g0) and np.array_equal(sz, z.s0) and z.refit.steps == 1
        assert np.array_equal(_u32(got["master"]), _u32(_halves(z.g0, z.s0).astype(F))) and not got["m"].any() and not got["v"].any()
        # ... and a Gaussian of zero sums among moving ones
        q = _sums(rng, n)
        still = np.arange(n) % 7 == 3
        q[still] = 0
        got2 = z.step(q, lr_colour=0.01, lr_opacity=0.01, opacity_min=0.0)
        g2, s2 = z.pc.download()
        assert _same_state(got2, z.st)
        assert np.array_equal(_u32(got2["master"][still]), _u32(got["master"][still])) and not got2["m"][still].any() and not got2["v"][still].any()
        assert np.array_equal(g2[still], z.g0[still]) and np.array_equal(s2[still], z.s0[still])
        assert (got2["master"][~still] != got["master"][~still]).any(axis=1).all()
    finally:
        for f in fits:
            f.close()
        c.close()


# ---- 3. the clamps -------------------------------------------------------------------------------------------------------------------
def test_clamps(ws):
    c = _ctx(ws)
    n = 40
    try:
        f = _Fit(ws, c, _cloud(ws, _rows(n, 31, special=False)))
        try:
            up = np.arange(n) % 2 == 0
            q = np.zeros((n, 4), np.int64)
            q[:, 3] = np.where(up, -(2 ** 61), 2 ** 61)    # a negative gradient raises the opacity
            q[:, :3] = np.where(up[:, None], -(2 ** 40), 2 ** 40)
            got = f.step(q, lr_colour=1e6, lr_opacity=10.0, opacity_min=0.125)
            assert _same_state(got, f.st)
            assert (got["master"][up, 3] == F(1.0)).all() and (got["master"][~up, 3] == F(0.125)).all()
            assert (got["master"][up, :3] == F(65504.0)).all() and (got["master"][~up, :3] == F(-65504.0)).all()
            h = _halves(*f.pc.download())
            assert np.isfinite(h.astype(F)).all()
            assert (_h16(h)[up, :3] == 0x7BFF).all() and (_h16(h)[~up, :3] == 0xFBFF).all()
            assert (_h16(h)[up, 3] == 0x3C00).all() and (_h16(h)[~up, 3] == 0x3000).all()
        finally:
            f.close()
    finally:
        c.close()


# ---- 4. refusals on the device -------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(ws):
    c = _ctx(ws)
    n = 64
    try:
        gpc_c, _ = _compressed(ws, n=3000)
        packed = ws.PointCloud(c, gpc_c)
        f = _Fit(ws, c, _cloud(ws, _rows(n, 41)))
        other = ws.PointCloud(c, _cloud(ws, _rows(n, 42)))
        small = ws.Grad(c, n - 1)
        try:
            with pytest.raises(ws.WebSplatError) as e:
                ws.Refit(c, packed)
            assert e.value.code == L.WS_ERR_UNSUPPORTED and "compressed" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                f.refit.step(other, f.grad, colour_unit=UNIT, opacity_unit=UNIT)
            assert e.value.code == L.WS_ERR_INVALID and "created for" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                f.refit.step(f.pc, small, colour_unit=UNIT, opacity_unit=UNIT)
            assert e.value.code == L.WS_ERR_INVALID and "number of points" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                f.refit.step(f.pc, f.grad, colour_unit=UNIT, opacity_unit=UNIT, beta1=1.0)
            assert e.value.code == L.WS_ERR_INVALID and "beta1" in str(e.value)
            with pytest.raises(ValueError):
                f.refit.step(f.pc, f.grad)   # no frame in the accumulator and no unit given
            assert f.refit.steps == 0 and f.refit.num_points() == n
            g, s = f.pc.download()
            assert np.array_equal(g, f.g0) and np.array_equal(s, f.s0)
        finally:
            small.close()
            other.close()
            f.close()
            packed.close()
    finally:
        c.close()


# ---- 5. the loop does what it is for; 7. the refitted cloud survives ---------------------------------------------------------------
STEPS = 40
OPACITY_SCALE = 1.0 / 128


@pytest.fixture(scope="module")
def fitted(ws):
    """Forty steps of the manual loop on the four-layer stack, the colours and opacities pushed off: target = the base plane of
    the stack itself.  Yields what the tests look at; the cloud and its renderer stay open for test 7."""
    c = _ctx(ws, bin_request=0)
    rows = _stack(4, 0.3)
    gpc_t, args = blend_ref.device_scene(ws, rows, (32, 32))
    off = rows.copy()
    off[:, 6:9] += np.array([0.6, -0.5, 0.4], F)
    off[:, OPACITY_COLUMN] = np.log(0.2 / 0.8)
    gpc, _ = blend_ref.device_scene(ws, off, (32, 32))
    r = ws.GaussianRenderer(c, "rgba32float", 3, False)
    r.enable_contrib(True)
    scratch = ws.Grad(c, 4)
    zeros = np.zeros((32, 32, 4), F)

    def base_of(pc):
        r.prepare(pc, args)
        r.accumulate_gradient(pc, scratch, zeros, background=BG, base=True)   # (pass 1's image; nothing is added)
        return r.download_removal_base()

    pc_t = ws.PointCloud(c, gpc_t)
    target = base_of(pc_t)
    pc_t.close()
    f = _Fit(ws, c, gpc)
    loss = lambda base: float(((base[..., :3].astype(np.float64) - target[..., :3].astype(np.float64)) ** 2).sum())  # noqa: E731
    out = dict(c=c, f=f, r=r, args=args, gpc=gpc, losses=[], mismatches=[], moved=0)
    for k in range(STEPS):
        base = base_of(f.pc)
        out["losses"].append(loss(base))
        plane = ws.image_error_gradient(c, base, target, kind="sq")
        f.grad.reset()
        r.accumulate_gradient(f.pc, f.grad, plane, background=BG, opacity_scale=OPACITY_SCALE)
        q = f.grad.download()
        assert f.grad.frames == 1
        out["moved"] += int((q != 0).any(axis=1).all())
        f.refit.step(f.pc, f.grad, lr_colour=0.02, lr_opacity=0.01, opacity_scale=OPACITY_SCALE)   # (the units: one frame, these scales)
        refit_ref.step(f.st, q, UNIT, UNIT * 128.0, lr_colour=0.02, lr_opacity=0.01)
        if not _same_state(f.refit.download(), f.st):
            out["mismatches"].append(k + 1)
    out["losses"].append(loss(base_of(f.pc)))
    assert not scratch.download().any()
    yield out
    scratch.close()
    r.close()
    f.close()
    c.close()


def test_loop_lowers_the_loss(fitted):
    """At every step the masters are refit_ref's, fed with the device's own sums (units, C0, the division by the opacity, the
    order); and the summed squared error of the base plane against the target is strictly lower after the last step than before
    the first.  The ratio is recorded, not gated."""
    losses = fitted["losses"]
    out = os.path.join(ROOT, "profiles", "refit")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "convergence.json"), "w") as fh:
        json.dump(dict(scene="attrib_frames._stack(4, 0.3) at 32x32, f_dc shifted by (+0.6, -0.5, +0.4), opacities 0.2", steps=STEPS, lr_colour=0.02,
                       lr_opacity=0.01, opacity_scale=OPACITY_SCALE, loss="sum over pixels and colour channels of (base - target)^2, float64",
                       before=losses[0], after=losses[-1], ratio=losses[-1] / losses[0], trajectory=losses), fh, indent=1)
    print(f"loss before {losses[0]:.6f}, after {STEPS} steps {losses[-1]:.6f} (ratio {losses[-1] / losses[0]:.4f})")
    assert fitted["mismatches"] == [], f"masters differ from the reference after steps {fitted['mismatches']}"
    assert fitted["moved"] == STEPS and fitted["f"].refit.steps == STEPS
    assert losses[0] > 0 and losses[-1] < losses[0]


def test_refitted_cloud_survives_download_recreation_and_subsetting(ws, fitted):
    c, f, args = fitted["c"], fitted["f"], fitted["args"]
    g, s = f.pc.download()
    master = f.refit.download()["master"]
    assert np.array_equal(_h16(_halves(g, s)), _h16(master.astype(np.float16))) and not np.array_equal(_halves(g, s), _halves(f.g0, f.s0))
    again = ws.PointCloud(c, dataclasses.replace(fitted["gpc"], gaussians=g, sh_coefs=s))
    sub = f.pc.subset([0, 2, 3])
    r = ws.GaussianRenderer(c, "rgba32float", 3, False)
    try:
        images = []
        for pc in (f.pc, again):
            r.prepare(pc, args)
            r.render(pc, background=(0.1, 0.2, 0.3, 1.0))
            images.append(r.download_target().copy())
        assert np.array_equal(_u32(images[0]), _u32(images[1])) and np.ptp(images[0][..., :3]) > 0.01
        gs, ss = sub.download()
        assert np.array_equal(gs, g[[0, 2, 3]]) and np.array_equal(ss, s[[0, 2, 3]])
    finally:
        r.close()
        sub.close()
        again.close()


# ---- 6. the scene driver, the tool ------------------------------------------------------------------------------------------------
SMALL = (160, 120)


def test_scene_driver_equals_the_manual_loop_and_the_tool_refits(ws, tmp_path):
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=2000, seed=0)
        keep = np.arange(rows.shape[0]) % 4 != 3   # 1 500 of the 2 000: the pruned cloud against its parent
        ply, sub_ply, cj = tmp_path / "parent.ply", tmp_path / "pruned.ply", tmp_path / "cameras.json"
        synth.write_ply(str(ply), rows)
        synth.write_ply(str(sub_ply), rows[keep])
        parent = ws.PointCloud.load(c, str(ply))   # (the tool's own loader)
        pcs = [ws.PointCloud.load(c, str(sub_ply)) for _ in range(2)]
        n = pcs[0].num_points()
        assert n == 1500
        cams = synth.orbit_cameras(6, SMALL[0], SMALL[1], 150.0, 150.0, radius=3.0, height_off=0.4)   # file position 0 is the test camera
        text = json.dumps([cam.to_json() for cam in cams])
        scene = ws.Scene.from_json_text(text)
        assert len(scene.cameras("train")) == 5
        fits = [ws.Refit(c, pc) for pc in pcs]
        grad, scratch = ws.Grad(c, n), ws.Grad(c, n)
        r, rb = ws.GaussianRenderer(c, "rgba16float", 3, False), ws.GaussianRenderer(c, "rgba16float", 3, False)
        adam = dict(lr_colour=0.005, lr_opacity=0.01)
        try:
            assert ws.refit_scene(c, pcs[0], scene, "train", fits[0], ref=parent, epochs=2, views_per_step=2, **adam) == 6 and fits[0].steps == 6
            # the same by hand: the frames of ws_scene_accumulate_gradient, a step after every second one and at the epoch's end
            pc, fit = pcs[1], fits[1]
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
                    r.accumulate_gradient(pc, grad, plane, background=bg, opacity_scale=1.0 / 128)
                    if grad.frames == 2 or i == len(train) - 1:
                        fit.step(pc, grad, opacity_scale=1.0 / 128, **adam)
                        grad.reset()
            assert r.errors()[0] == 0 and fit.steps == 6
            (gd, sd), (gm, sm) = pcs[0].download(), pcs[1].download()
            d, m = fits[0].download(), fits[1].download()
            assert all(np.array_equal(_u32(d[k]), _u32(m[k])) for k in d) and (d["v"] != 0).all(axis=1).sum() > 500
            assert np.array_equal(gd, gm) and np.array_equal(sd, sm)
            fresh = ws.PointCloud.load(c, str(sub_ply))
            try:
                g0, s0 = fresh.download()
            finally:
                fresh.close()
            assert np.array_equal(_elsewhere(gd, sd), _elsewhere(g0, s0)) and not np.array_equal(_halves(gd, sd), _halves(g0, s0))
            # one step per epoch
            assert ws.refit_scene(c, pcs[0], scene, "train", fits[0], ref=parent, epochs=2, views_per_step=0, **adam) == 2 and fits[0].steps == 8
            # the driver's own refusals
            with pytest.raises(ws.WebSplatError) as e:
                ws.refit_scene(c, pcs[0], scene, "train", fits[0], ref=pcs[0])
            assert e.value.code == L.WS_ERR_INVALID and "ref_pc" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                ws.refit_scene(c, pcs[0], scene, "train", fits[0])
            assert e.value.code == L.WS_ERR_INVALID and "exactly one" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                ws.refit_scene(c, pcs[0], scene, "train", fits[1], ref=parent)
            assert e.value.code == L.WS_ERR_INVALID and "created for" in str(e.value)
            # the tool: the table, the refit on the train split, the table again
            cj.write_text(text)
            exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
            out = subprocess.run([exe, str(sub_ply), str(cj), "--ref", str(ply), "--refit", "2", "--views-per-step", "2", "--lr-colour", "0.005"],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            means = [i for i, ln in enumerate(lines) if ln.startswith("mean over 1 images: PSNR")]
            after = [i for i, ln in enumerate(lines) if ln.startswith("after refit:")]
            print(out.stdout)
            assert len(means) == 2 and len(after) == 1 and means[0] < after[0] < means[1]
            assert lines[after[0]] == "after refit: 2 epochs, 6 steps"
            assert lines[means[0] - 1].split()[:2] == lines[means[1] - 1].split()[:2] and lines[means[0]] != lines[means[1]]
            # ... and a compressed scene is refused with the library's message
            npz = tmp_path / "packed.npz"
            synth.write_npz(str(npz), synth.c3dgs_arrays(n=2000, n_geometry=256, n_sh=256))
            out = subprocess.run([exe, str(npz), str(cj), "--ref", str(npz), "--refit", "1"], capture_output=True, text=True, timeout=120)
            assert out.returncode != 0 and "ws_refit_create" in out.stderr and "compressed" in out.stderr
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
