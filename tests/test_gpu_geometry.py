"""Geometry gradients on the device (include/websplat.h "Geometry gradients"; geometry.hip k_geometry, geometry_spread.hip
k_geom_spread).

   1. stage A's five scratch sums against float64 (tests/geometry_ref.py): one 32 x 32 tile, a 64 x 48 viewport (partial tiles, several
      tiles), a tile list of 513 entries (two and three staged batches), a saturating stack; every tile shape, WS_BIN_SHIFT 0 and 1
   2. the three bit-for-bit properties                         4. frames add; the scratch comes back clean; a plane of zeros
   3. k_geom_spread against its host twin, word for word       5. merging, reset and refusals
   6. the scene driver over a two-camera cameras.json against two explicit calls; websplat_evaluate --densify

The scratch sums are read through the test hooks ws_debug_geometry_stage_a / ws_debug_geomgrad_scratch.  The smallest frames that
reach every path: each case prepares one frame of at most 513 Gaussians; a float64 reference is computed once per frame and shared
by the configurations that walk it (K1 and the depth sort do not depend on the tile configuration)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref
import geometry_ref as ref
import gradient_ref
import k1_edges
import removal_ref
from attrib_frames import BG, F, _compressed, _ctx, _Frame, _stack, _stack_frame
from gradient_frames import signed_ramp
from sh_frames import TILE, _line, _oblique
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 32
WIDE = (64, 48)
SHAPES = {"4x4": {}, "4x2": {"tile_qw": 4, "tile_qh": 2}, "2x2": {"tile_qw": 2, "tile_qh": 2}}
_REF = {}


def _frame(ws, c, scene):
    """scene -> (_Frame, SplattingArgs, viewport, geometry_scale, saturating)"""
    if scene == "tile":
        gpc, args = _oblique(ws, _line(24, 0.03), 3)
        return _Frame(ws, c, gpc, args), args, TILE, 8.0, False
    if scene == "wide":
        gpc, args = _oblique(ws, _line(24, 0.03), 3, viewport=WIDE)
        return _Frame(ws, c, gpc, args), args, WIDE, 8.0, False
    k, opacity, s, sat = {"long": (513, 0.002, 64.0, False), "saturating": (513, 0.9, 1.0 / 128, True)}[scene]
    gpc, args = blend_ref.device_scene(ws, _stack(k, opacity), TILE)
    return _Frame(ws, c, gpc, args), args, TILE, s, sat


def _stage_a(f, plane, s, scale=1.0):
    """(N, 5) int64: k_geometry's scratch sums of one frame; the scratch is cleared again."""
    acc = f.ws.GeomGrad(f.c, f.n)
    try:
        f.r.accumulate_geometry_gradient(f.pc, acc, plane, background=BG, scale=scale, geometry_scale=s, _stage_a_only=True)
        assert acc.frames == 0
        q = acc._debug_scratch()
        acc._debug_clear_scratch()
        assert not acc._debug_scratch().any()
        return q
    finally:
        acc.close()


def _reference(scene, f, view, s, sat):
    """(frame, plane g, float64 reference) of the scene's frame: undecided pixels masked out of the plane."""
    frame = f.frame()
    hit = _REF.get(scene)
    if hit is None or not all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
        w, h = view
        base = removal_ref.base_f64(frame, w, h, BG)
        # (a saturating frame keeps its pixels of T_end < 2^-13: bounds() carries their tail; only undecided pairs are masked)
        ok = (base["und"] == 0) if sat else ~removal_ref.undecided_mask(base)
        assert 1.0 - ok.mean() <= 0.05
        g = (signed_ramp(w, h) * ok[..., None]).astype(F)
        hit = _REF[scene] = (frame, g, ref.stage_a_f64(frame, w, h, f.n, gradient_ref.plane_G(g), BG, geometry_scale=s, saturating=sat))
    return hit


def _compare(case, q, want, min_drawn, tight=True):
    tol = ref.bounds(want)
    got = q.astype(np.float64) / SCALE
    d = np.abs(got - want["sum"])
    i = np.unravel_index(int(np.argmax(d - tol)), d.shape)
    nz = np.abs(want["sum"]) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(nz, d / np.abs(want["sum"]), 0.0)
        tol_over = np.where(nz, tol / np.abs(want["sum"]), 0.0)
    drawn = int((q != 0).any(axis=1).sum())
    print(f"{case}: {drawn} Gaussians with sums, worst excess {float((d - tol).max()):.3e}, largest relative difference {float(rel.max()):.3e}, "
          f"median bound / value {float(np.median(tol_over[nz])):.3e}, band pairs {int(want['band'].sum())}, clamped {int(want['clamped'].sum())}")
    assert int(want["U"].sum()) == 0, "a pair that counts at a pixel with an undecided pair: the plane has to mask it"
    assert drawn >= min_drawn
    assert np.all(d <= tol), (f"{int((d > tol).sum())} sums out of bound, worst at Gaussian {i[0]} sum {i[1]}: got {got[i]:.9e} "
                             f"ref {want['sum'][i]:.9e} tol {tol[i]:.3e}")
    # the bound says something: a sum with the wrong sign, or m's and S's exchanged, is outside it for most Gaussians
    if tight:
        big = np.abs(want["sum"]) > 4 * tol
        assert big[:, 2].mean() > 0.5 and big[:, 4].mean() > 0.5, "the bound is wider than the sums it judges"


# ---- 1. stage A against float64 -------------------------------------------------------------------------------------------------
CASES = [(scene, shape, b) for scene in ("tile", "wide") for shape in SHAPES for b in (0, 1)]
CASES += [("long", shape, 0) for shape in SHAPES] + [("saturating", "4x4", 0), ("saturating", "2x2", 1), ("saturating", "4x2", 0)]


@pytest.mark.parametrize("scene,shape,bin_request", CASES, ids=[f"{s}-{sh}-bin{b}" for s, sh, b in CASES])
def test_stage_a_against_f64(ws, scene, shape, bin_request):
    c = _ctx(ws, bin_request=bin_request, **SHAPES[shape])
    try:
        f, args, view, s, sat = _frame(ws, c, scene)
        try:
            if scene in ("long", "saturating"):
                assert int(f.r.tile_stats()["list_len"].max()) == 513     # two staged batches at STAGE 512, three at 256
            frame, g, want = _reference(scene, f, view, s, sat)
            q = _stage_a(f, g, s)
            _compare(f"{scene}-{shape}-bin{bin_request}", q, want, 3 if sat else f.n, tight=not sat)
            if sat:
                assert not q[200:].any() and want["T"].max() < 2.0 ** -14    # every quadrant stops: the far layers add nothing
            else:
                assert int(want["band"].sum()) == 0 and int(want["clamped"].sum()) == 0
            assert np.array_equal(_stage_a(f, g, s), q)                       # repetition: the same words
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. the bit-for-bit properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_properties(ws, shape):
    c = _ctx(ws, **SHAPES[shape])
    try:
        f, args, view, s, _ = _frame(ws, c, "wide")
        try:
            w, h = view
            g = signed_ramp(w, h)
            q = _stage_a(f, g, s)
            assert (q != 0).all(axis=1).sum() >= f.n - 2
            assert np.array_equal(_stage_a(f, -g, s), -q), "g and -g give exactly negated sums"
            mask = ((np.arange(w)[None, :] // 3 + np.arange(h)[:, None] // 5) % 2).astype(F)[..., None]
            a, b = _stage_a(f, g * mask, s), _stage_a(f, g * (1 - mask), s)
            assert a.any() and b.any() and np.array_equal(a + b, q), "a 0/1 mask and its complement add up to the whole"
            assert np.array_equal(_stage_a(f, g, s), q), "two runs give the same words"
            # a second renderer's frame of the same cloud, prepared afresh: the same words again
            r2 = ws.GaussianRenderer(c, "rgba32float", 3, False)
            acc = ws.GeomGrad(c, f.n)
            try:
                r2.enable_contrib(True)
                r2.prepare(f.pc, args)
                r2.accumulate_geometry_gradient(f.pc, acc, g, background=BG, geometry_scale=s, _stage_a_only=True)
                assert np.array_equal(acc._debug_scratch(), q)
            finally:
                acc.close()
                r2.close()
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. the spread against its host twin ------------------------------------------------------------------------------------------
def _twin_rows(f, args, frame, q5, s):
    """ws_geom_spread_rows on the frame's rows: the record's halves per SOURCE Gaussian, the cloud's position and covariance halves."""
    g, _ = f.pc.download()
    xyz = np.ascontiguousarray(g[:, :12]).view(F).reshape(-1, 3)
    cov_bits = np.ascontiguousarray(g[:, 16:28]).view(np.uint16).reshape(-1, 6)
    rec = np.zeros((f.n, 4), np.uint16)
    src = frame["src_index"].astype(np.int64)
    rec[src] = np.ascontiguousarray(frame["splats"]).view(np.uint16).reshape(-1, 10)[: src.size, :4]
    cu = args.camera.uniform(args.viewport)
    rs = f.pc.settings_uniform(args)
    return f.ws.geom_spread_rows(q5, rec, xyz, cov_bits, cu, rs, geometry_scale=s), (xyz, cov_bits, rec, cu, rs)


@pytest.mark.parametrize("scene,shape", [("wide", "4x4"), ("wide", "2x2"), ("tile", "4x2"), ("saturating", "4x4")])
def test_spread_equals_the_host_twin_word_for_word(ws, oracle, scene, shape):
    c = _ctx(ws, **SHAPES[shape])
    try:
        f, args, view, s, _ = _frame(ws, c, scene)
        acc = ws.GeomGrad(c, f.n)
        try:
            g = signed_ramp(*view)
            q5 = _stage_a(f, g, s)
            f.r.accumulate_geometry_gradient(f.pc, acc, g, background=BG, geometry_scale=s)
            got = acc.download()
            assert acc.frames == 1 and not acc._debug_scratch().any(), "the scratch comes back clean"
            want, (xyz, cov_bits, rec, cu, rs) = _twin_rows(f, args, f.frame(), q5, s)
            live = (q5 != 0).any(axis=1)
            assert np.array_equal(got["seen"], live.astype(np.uint64)) and np.array_equal(want["seen"], got["seen"]) and live.sum() >= 3
            for key in ("position", "covariance", "screen_norm"):
                assert np.isfinite(got[key]).all()
                bad = np.argwhere(got[key].view(np.uint64) != want[key].view(np.uint64))
                assert bad.size == 0, f"{key}: {bad.shape[0]} words differ from the host twin, first at {bad[0]}"
                assert (np.abs(got[key][live]).reshape(int(live.sum()), -1).max(axis=1) > 0).all()
            # ... and the twin is the float64 chain (the CPU tier compares them on random rows; here on a device frame's)
            u = k1_edges.uniforms_f64(oracle.copy_struct(oracle.CameraUniform, cu), oracle.copy_struct(oracle.SettingsUniform, rs))
            f64 = ref.spread_f64(q5, rec, xyz, cov_bits, u, *view, geometry_scale=s)
            for key in ("position", "covariance", "screen_norm"):
                a, b = got[key].reshape(f.n, -1), f64[key].reshape(f.n, -1)
                assert (np.abs(a - b) <= 1e-12 * np.abs(b).max(axis=1, keepdims=True)).all(), key
        finally:
            acc.close()
            f.close()
    finally:
        c.close()


# ---- 4. frames add; a plane of zeros ----------------------------------------------------------------------------------------------
def test_frames_add_and_a_zero_plane_adds_nothing(ws):
    c = _ctx(ws)
    try:
        rows = _line(24, 0.03)
        views = [_oblique(ws, rows, 3, viewport=WIDE), _oblique(ws, rows, 3, viewport=WIDE, eye=np.array([2.2, -0.8, -1.9]))]
        pc = ws.PointCloud(c, views[0][0])
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        r.enable_contrib(True)
        alone = [ws.GeomGrad(c, n) for _ in views]
        both = ws.GeomGrad(c, n)
        g = signed_ramp(*WIDE)
        try:
            for (_, args), acc in zip(views, alone):
                r.prepare(pc, args)
                r.accumulate_geometry_gradient(pc, acc, g, background=BG, geometry_scale=8.0)
                r.accumulate_geometry_gradient(pc, both, g, background=BG, geometry_scale=8.0)
                assert not both._debug_scratch().any(), "a second frame starts from a clean scratch"
            a, b, ab = alone[0].download(), alone[1].download(), both.download()
            assert both.frames == 2 and alone[0].frames == alone[1].frames == 1
            assert not np.array_equal(a["position"], b["position"]) and a["seen"].sum() >= n - 2 and b["seen"].sum() >= n - 2
            for key in ("position", "covariance", "screen_norm", "seen"):
                assert np.array_equal(ab[key], a[key] + b[key]), key      # (0 + a) + b: one rounded addition either way
            # a plane of zeros adds nothing, to the sums or to seen -- neither of its own nor anything a frame left in the scratch
            r.accumulate_geometry_gradient(pc, both, np.zeros((WIDE[1], WIDE[0], 4), F), background=BG)
            z = both.download()
            assert both.frames == 3 and all(np.array_equal(z[k].view(np.uint64), ab[k].view(np.uint64)) for k in z)
            fresh = ws.GeomGrad(c, n)
            try:
                r.accumulate_geometry_gradient(pc, fresh, np.zeros((WIDE[1], WIDE[0], 4), F), background=BG)
                zero = fresh.download()
                assert fresh.frames == 1 and not any(zero[k].view(np.uint64).any() for k in zero)
            finally:
                fresh.close()
            assert r.errors()[0] == 0
        finally:
            for acc in alone + [both]:
                acc.close()
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 5. merging, reset, refusals --------------------------------------------------------------------------------------------------
def test_merging_reset_and_refusals(ws):
    c = _ctx(ws)
    try:
        f, args, view, s, _ = _frame(ws, c, "wide")
        gpc_c, args_c = _compressed(ws, n=3000)
        fc = _Frame(ws, c, gpc_c, args_c, compressed=True)
        plain = ws.GaussianRenderer(c, "rgba32float", 3, False)
        accs = dict(small=ws.GeomGrad(c, f.n - 1), good=ws.GeomGrad(c, f.n), packed=ws.GeomGrad(c, fc.n))
        g = signed_ramp(*view)
        try:
            def refused(r, pc, acc, code, text, p=g):
                with pytest.raises(ws.WebSplatError) as e:
                    r.accumulate_geometry_gradient(pc, acc, p, background=BG)
                assert e.value.code == code and text in str(e.value) and "ws_renderer_accumulate_geometry_gradient" in str(e.value), str(e.value)

            refused(f.r, f.pc, accs["small"], L.WS_ERR_INVALID, "number of points")
            refused(fc.r, fc.pc, accs["packed"], L.WS_ERR_UNSUPPORTED, "compressed", p=signed_ramp(400, 300))
            plain.prepare(f.pc, args)
            refused(plain, f.pc, accs["good"], L.WS_ERR_STATE, "enable_contrib")
            for acc in accs.values():
                got = acc.download()
                assert acc.frames == 0 and not any(got[k].view(np.uint64).any() for k in got) and not acc._debug_scratch().any()
            acc = accs["good"]
            f.r.accumulate_geometry_gradient(f.pc, acc, g, background=BG, geometry_scale=s)
            one = acc.download()
            acc.add(**one)
            two = acc.download()
            assert acc.frames == 1 and all(np.array_equal(two[k], 2 * one[k]) for k in one) and one["seen"].max() == 1
            acc.add(seen=one["seen"])                      # any array alone
            acc.add(position=-one["position"])
            three = acc.download()
            assert np.array_equal(three["seen"], 3 * one["seen"]) and np.array_equal(three["position"], one["position"])
            assert np.array_equal(three["covariance"], two["covariance"])
            with pytest.raises(ValueError):
                acc.add(covariance=one["covariance"][:, :5])
            with pytest.raises(ws.WebSplatError):
                acc.add(position=one["position"][:-1])     # fewer rows than the accumulator has points
            acc.reset()
            zero = acc.download()
            assert acc.frames == 0 and not any(zero[k].view(np.uint64).any() for k in zero)
        finally:
            for acc in accs.values():
                acc.close()
            plain.close()
            fc.close()
            f.close()
    finally:
        c.close()


# ---- 6. the scene driver, the tool ------------------------------------------------------------------------------------------------
SMALL = (96, 72)


def test_scene_driver_equals_two_explicit_calls_and_the_tool_lists_it(ws, tmp_path):
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=2000, seed=3)
        keep = np.arange(rows.shape[0]) % 3 != 2   # every third Gaussian dropped: the pruned cloud against its parent
        ply, sub_ply, cj = tmp_path / "parent.ply", tmp_path / "pruned.ply", tmp_path / "cameras.json"
        synth.write_ply(str(ply), rows)
        synth.write_ply(str(sub_ply), rows[keep])
        parent, pc = ws.PointCloud.load(c, str(ply)), ws.PointCloud.load(c, str(sub_ply))   # (the tool's own loader)
        n = pc.num_points()
        cams = synth.orbit_cameras(2, SMALL[0], SMALL[1], 90.0, 90.0, radius=3.0, height_off=0.4)
        text = json.dumps([cam.to_json() for cam in cams])
        scene = ws.Scene.from_json_text(text)
        driver, manual, scratch = (ws.GeomGrad(c, n) for _ in range(3))
        r, rb = ws.GaussianRenderer(c, "rgba16float", pc.sh_deg(), False), ws.GaussianRenderer(c, "rgba16float", parent.sh_deg(), False)
        try:
            assert ws.accumulate_geometry_gradient_scene(c, pc, scene, None, driver, ref=parent, kind="sq", geometry_scale=0.5) == 2 and driver.frames == 2
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
                r.accumulate_geometry_gradient(pc, scratch, np.zeros((SMALL[1], SMALL[0], 4), F), background=bg, base=True)   # (pass 1's image)
                base = r.download_removal_base()
                plane = ws.image_error_gradient(c, base, b, kind="sq", background_b=bg)
                r.accumulate_geometry_gradient(pc, manual, plane, background=bg, geometry_scale=0.5)
            zero = scratch.download()
            assert r.errors()[0] == 0 and not any(zero[k].view(np.uint64).any() for k in zero)
            qd, qm = driver.download(), manual.download()
            assert (qd["seen"] > 0).sum() > 300 and qd["seen"].max() == 2
            assert all(np.array_equal(qd[k].view(np.uint64), qm[k].view(np.uint64)) for k in qd)
            # the tool: the five largest screen_norm / seen of the test split
            cj.write_text(text)
            exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
            out = subprocess.run([exe, str(sub_ply), str(cj), "--ref", str(ply), "--densify", "5", "--split", "test"], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            head = [i for i, ln in enumerate(lines) if ln.startswith("densify (sq error")]
            assert len(head) == 1 and "PSNR" in out.stdout
            driver.reset()
            frames = ws.accumulate_geometry_gradient_scene(c, pc, scene, "test", driver, ref=parent)
            qs = driver.download()
            assert f"over {frames} frames" in lines[head[0]]
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = np.where(qs["seen"] > 0, qs["screen_norm"] / qs["seen"], 0.0)
            order = sorted(range(n), key=lambda i: (-mean[i], i))[:5]
            for ln, i in zip(lines[head[0] + 2:head[0] + 7], order):
                cols = ln.split()
                assert int(cols[0]) == i and int(cols[2]) == int(qs["seen"][i])
                assert np.allclose([float(cols[1]), float(cols[3])], [mean[i], np.linalg.norm(qs["position"][i])], rtol=1e-8, atol=0)
            m = re.fullmatch(r"densify: (\d+) of (\d+) seen Gaussians have a norm of exactly 0", lines[-1])
            assert m and int(m.group(2)) == int((qs["seen"] > 0).sum()) and int(m.group(1)) == int(((qs["seen"] > 0) & (qs["screen_norm"] == 0)).sum())
            # the driver's own errors
            with pytest.raises(ws.WebSplatError) as e:
                ws.accumulate_geometry_gradient_scene(c, pc, scene, None, driver)
            assert e.value.code == L.WS_ERR_INVALID and "exactly one" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                ws.accumulate_geometry_gradient_scene(c, pc, scene, None, driver, ref=parent, geometry_scale=0.0)
            assert e.value.code == L.WS_ERR_INVALID and "geometry_scale" in str(e.value)
            with pytest.raises(ws.WebSplatError) as e:
                ws.accumulate_geometry_gradient_scene(c, parent, scene, None, driver, ref=pc)
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
