"""Geometry gradients on the device (include/websplat.h "Geometry gradients"; geometry.hip k_geometry, geometry_spread.hip
k_geom_spread).

   1. stage A's five scratch sums against float64 (tests/geometry_ref.py): one 32 x 32 tile, a 64 x 48 viewport (partial tiles, several
      tiles), a tile list of 513 entries (two and three staged batches), a saturating stack; every tile shape, WS_BIN_SHIFT 0 and 1
   2. the three bit-for-bit properties                         4. frames add; the scratch comes back clean; a plane of zeros
   3. k_geom_spread against its host twin, word for word       5. merging, reset and refusals
   6. the scene driver over a two-camera cameras.json against two explicit calls; websplat_evaluate --densify
   7. the frames of geometry_frames.py: the general anisotropic cloud at 96 x 72 (stage A within bounds and outside three mutants'
      on every tile shape and bin shift, the bitwise properties, the spread on a frame where most of the cloud is culled), the
      clamped core, the value cap to the bit

The frames of 1 - 6 are isotropic Gaussians that cover the whole viewport: an orthogonal mix-up of (p0, p1), a record that reaches
some quadrants only, the 0.99 clamp and the value cap cannot show on them; 7 is where they can.  NaN -> 0 in geom_value: a NaN in the
plane is 0 in grad_plane_value, the scales and the background are refused unless finite, T > 0 on a counted pair; a NaN reaches it
only through a record whose f16 colour is infinite (F = inf from k_removal_base, F - P = inf - inf): that is the last case of 7.

A module-scoped fixture writes one row per case compared in 7 to geometry_report.json in WEBSPLAT_REPORT_DIR (default:
test_reports/ under the repository root, as tests/test_gpu_gradient.py); profiles/geometry/errors.json is an MI355X run's copy.

The scratch sums are read through the test hooks ws_debug_geometry_stage_a / ws_debug_geomgrad_scratch.  The smallest frames that
reach every path: each case prepares one frame of at most 513 Gaussians (7: the cloud of 3000); a float64 reference is computed once per frame and shared
by the configurations that walk it (K1 and the depth sort do not depend on the tile configuration)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref
import geometry_frames as gf
import geometry_ref as ref
import gradient_ref
import k1_edges
import removal_ref
from attrib_frames import BG, F, _compressed, _ctx, _Frame, _stack, _stack_frame
from gradient_frames import signed_ramp, splat_halves
from sh_frames import TILE, _line, _oblique
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 2.0 ** 32
WIDE = (64, 48)
SHAPES = {"4x4": {}, "4x2": {"tile_qw": 4, "tile_qh": 2}, "2x2": {"tile_qw": 2, "tile_qh": 2}}
_REF = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "geometry_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


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


def _compare(case, q, want, min_drawn, tight=True, report=False):
    """Every one of the five sums of every Gaussian within bounds() of the float64 reference.  report: the case's row of
    geometry_report.json (returned, so that the caller can add its mutant shares), written before anything is asserted."""
    row = None
    if report:
        row = dict(case=case, **gf.summary(q, want))
        REPORT.append(row)
        print(json.dumps(row))
    _assert_within(case, q, want, min_drawn, tight)
    return row


def _assert_within(case, q, want, min_drawn, tight):
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
    # (of the Gaussians the walk meets: one that K1 culled has five zeros and a bound of zero)
    if tight:
        big = (np.abs(want["sum"]) > 4 * tol)[want["pairs"] > 0]
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


# ---- 7. anisotropic splats, the clamped core, the value cap ---------------------------------------------------------------------
def _same_frame(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("splats", "sorted", "src_index"))


def _shared(key, frame, make):
    """One float64 reference per frame, shared by the configurations that walk it (_REF): make() -> anything, kept beside the frame."""
    hit = _REF.get(key)
    if hit is None or not _same_frame(hit[0], frame):
        hit = _REF[key] = (frame, make())
    return hit[1]


def _bitwise(f, g, s, q, scale=1.0):
    """Section 2's properties on the frame at hand: repetition, g against -g, a 0/1 mask and its complement."""
    w, h = f.view
    assert np.array_equal(_stage_a(f, g, s, scale), q), "two runs give the same words"
    assert np.array_equal(_stage_a(f, -g, s, scale), -q), "g and -g give exactly negated sums"
    mask = ((np.arange(w)[None, :] // 3 + np.arange(h)[:, None] // 5) % 2).astype(F)[..., None]
    a, b = _stage_a(f, g * mask, s, scale), _stage_a(f, g * (1 - mask), s, scale)
    assert a.any() and b.any() and np.array_equal(a + b, q), "a 0/1 mask and its complement add up to the whole"


def _general_ref(f):
    """(plane, reference, {mutant: mutated reference} -- filled by the case that needs them) of the general cloud's frame."""
    frame = f.frame()

    def make():
        g, share = gf.masked_ramp(frame, gf.GENERAL_VIEW, gf.MASK_CAP_GENERAL)
        return g, gf.stage_a(frame, gf.GENERAL_VIEW, f.n, g, gf.GENERAL_S, gf.GENERAL_PLANE_SCALE), {}, share
    return (frame,) + _shared("general", frame, make)


GENERAL_CASES = [(shape, shift) for shape in SHAPES for shift in (0, 1)]


@pytest.mark.parametrize("shape,bin_shift", GENERAL_CASES, ids=[f"{sh}-shift{b}" for sh, b in GENERAL_CASES])
def test_stage_a_against_f64_general_cloud(ws, shape, bin_shift):
    """3000 anisotropic Gaussians at 96 x 72: 705 visible, most of them reaching some quadrants of some tiles only, a third with
    their centre outside the viewport.  WS_BIN_SHIFT 0 and 1 (bin_request 0 = never, 2 = always bin at twice the blend's tile):
    with 64-px bins the view has 2 x 2 lists, each shared by up to four 32-px tiles."""
    c = _ctx(ws, bin_request=2 * bin_shift, **SHAPES[shape])
    try:
        f = _Frame(ws, c, *blend_ref.device_scene(ws, gf.general_rows(), gf.GENERAL_VIEW))
        try:
            if shape == "4x4":
                assert f.r.tile_stats()["list_len"].size == (4 if bin_shift else 9)
            frame, g, want, wrongs, share = _general_ref(f)
            assert f.n - len(frame["src_index"]) > 2000
            s, ps = gf.GENERAL_S, gf.GENERAL_PLANE_SCALE
            q = _stage_a(f, g, s, ps)
            case = f"7-general-{shape}-shift{bin_shift}"
            row = _compare(case, q, want, min_drawn=500, tight=True, report=True)
            row["masked_share"] = share
            assert int(want["band"].sum()) == 0 and int(want["clamped"].sum()) == 0 and not want["capped"].any() and not want["straddling"].any()
            big = (np.abs(want["sum"]) > 4 * ref.bounds(want))[want["pairs"] > 0].mean(axis=0)
            assert (big > 0.9).all(), big
            _bitwise(f, g, s, q, ps)
            if shape == "4x4" and bin_shift == 0:
                drawn = (q != 0).any(axis=1)
                row["mutant_shares"] = {}
                for m in gf.GENERAL_MUTANTS:
                    if m not in wrongs:
                        wrongs[m] = gf.stage_a(frame, gf.GENERAL_VIEW, f.n, g, s, ps, mutate=m)
                    out_share, count, _ = gf.told_apart(q.astype(np.float64) / SCALE, wrongs[m], touched=drawn)
                    print(f"{case}: under {m} {100 * out_share:.1f} % of {count} drawn Gaussians are out of bounds")
                    row["mutant_shares"][m] = out_share
                    assert out_share >= 0.5, m
        finally:
            f.close()
    finally:
        c.close()


def test_spread_on_the_general_cloud(ws, oracle):
    """The full call on a frame where more than two thirds of the cloud are culled: the spread goes through src_index, and nothing
    of a Gaussian that is not in the frame is read or written."""
    c = _ctx(ws)
    try:
        gpc, args = blend_ref.device_scene(ws, gf.general_rows(), gf.GENERAL_VIEW)
        f = _Frame(ws, c, gpc, args)
        acc = ws.GeomGrad(c, f.n)
        try:
            frame, g, _, _, _ = _general_ref(f)
            s, ps = gf.GENERAL_S, gf.GENERAL_PLANE_SCALE
            q5 = _stage_a(f, g, s, ps)
            f.r.accumulate_geometry_gradient(f.pc, acc, g, background=BG, scale=ps, geometry_scale=s)
            got = acc.download()
            assert acc.frames == 1 and not acc._debug_scratch().any(), "the scratch comes back clean"
            live = (q5 != 0).any(axis=1)
            culled = np.ones(f.n, bool)
            culled[frame["src_index"].astype(np.int64)] = False
            assert culled.sum() > 2000 and live.sum() >= 500 and not live[culled].any()
            assert np.array_equal(got["seen"], live.astype(np.uint64))
            for key in ("position", "covariance", "screen_norm"):
                assert not got[key][culled].view(np.uint64).any(), f"{key}: a culled Gaussian has a sum"
            want, (xyz, cov_bits, rec, cu, rs) = _twin_rows(f, args, frame, q5, s)
            assert np.array_equal(want["seen"], got["seen"])
            u = k1_edges.uniforms_f64(oracle.copy_struct(oracle.CameraUniform, cu), oracle.copy_struct(oracle.SettingsUniform, rs))
            f64 = ref.spread_f64(q5, rec, xyz, cov_bits, u, *gf.GENERAL_VIEW, geometry_scale=s)
            for key in ("position", "covariance", "screen_norm"):
                assert np.isfinite(got[key]).all()
                bad = np.argwhere(got[key].view(np.uint64) != want[key].view(np.uint64))
                assert bad.size == 0, f"{key}: {bad.shape[0]} words differ from the host twin, first at {bad[0]}"
                a, b = got[key].reshape(f.n, -1), f64[key].reshape(f.n, -1)
                assert (np.abs(a - b) <= 1e-12 * np.abs(b).max(axis=1, keepdims=True)).all(), key
            assert (np.abs(got["position"][live]).max(axis=1) > 0).mean() > 0.99 and (got["screen_norm"][live] > 0).mean() > 0.99
        finally:
            acc.close()
            f.close()
    finally:
        c.close()


@pytest.mark.parametrize("shape", ["4x4", "2x2"])
def test_clamped_core(ws, shape):
    """Eight layers over the whole 32 x 32 view, the front one with alpha 1: the pairs of its core (a <= 0.01) are on the 0.99
    clamp and do not count.  Under the whole signed ramp they would move layer 0's sums by half the bound at most (|p| <= 0.12
    there, and the core is symmetric: geometry_frames.clamped_corner), so the rule is pinned under the corner plane, where layer
    0's sums are exactly 0 and a walk that counts clamped pairs is outside its own bounds in all five channels."""
    c = _ctx(ws, bin_request=0, **SHAPES[shape])
    try:
        f = _Frame(ws, c, *blend_ref.device_scene(ws, gf.clamped_rows(), gf.TILE))
        try:
            frame = f.frame()
            n = f.n

            def make():
                g, _ = gf.masked_ramp(frame, gf.TILE, gf.MASK_CAP_GENERAL)
                corner = gf.clamped_corner(frame, gf.TILE)
                gc = (signed_ramp(*gf.TILE) * corner[..., None]).astype(F)
                refs = {}
                for s in gf.CLAMPED_S:
                    refs[s] = (gf.stage_a(frame, gf.TILE, n, g, s), gf.stage_a(frame, gf.TILE, n, gc, s),
                               gf.stage_a(frame, gf.TILE, n, g, s, mutate="clamped_pairs_counted"),
                               gf.stage_a(frame, gf.TILE, n, gc, s, mutate="clamped_pairs_counted"))
                return g, gc, int(corner.sum()), refs
            g, gc, corner_px, refs = _shared("clamped", frame, make)
            assert splat_halves(frame, n)[0, 9] == 1.0
            for s in gf.CLAMPED_S:
                whole, right, whole_wrong, wrong = refs[s]
                case = f"7-clamped-core-{shape}-s{s:g}"
                assert 4 <= whole["clamped"][0] <= 16 and not whole["clamped"][1:].any() and int(whole["band"].sum()) == 0
                q = _stage_a(f, g, s)
                row = _compare(case, q, whole, min_drawn=n, tight=True, report=True)
                with np.errstate(divide="ignore", invalid="ignore"):
                    moved = np.abs(q.astype(np.float64) / SCALE - whole_wrong["sum"])[0] / ref.bounds(whole_wrong)[0]
                row["layer0_over_mutant_bound_whole_ramp"] = moved.tolist()
                # the corner plane
                assert corner_px >= 2 and int(right["pairs"][0]) == corner_px and int(right["counted"][0]) == 0 and int(right["band"].sum()) == 0
                assert not right["sum"][0].any() and not ref.bounds(right)[0].any()
                qc = _stage_a(f, gc, s)
                assert not qc[0].any(), f"layer 0 counts a clamped pair: {[hex(int(v) & (2 ** 64 - 1)) for v in qc[0]]}"
                row = _compare(case + "-corner", qc, right, min_drawn=n - 1, tight=True, report=True)
                share, count, outside = gf.told_apart(qc.astype(np.float64) / SCALE, wrong, touched=right["clamped"] > 0)
                print(f"{case}-corner: under clamped_pairs_counted layer 0 is outside in channels {outside[0].tolist()}")
                row["mutant_shares"] = {"clamped_pairs_counted": share}
                assert count == 1 and outside[0].all()
                assert np.array_equal(_stage_a(f, -gc, s), -qc)
        finally:
            f.close()
    finally:
        c.close()


def _hex_rows(q, expected):
    """The differing words of an exact comparison, in hex, with the count of lost (-) or doubled (+) capped lanes they amount to."""
    bad = np.argwhere(q != expected)
    return [f"[{j}][{k}] got {int(q[j, k]) & (2 ** 64 - 1):#018x} want {int(expected[j, k]) & (2 ** 64 - 1):#018x} "
            f"diff {(int(q[j, k]) - int(expected[j, k])) / ref.Q_CAP:+.6f} lanes" for j, k in bad[:20]]


@pytest.mark.parametrize("shape", ["4x4", "2x2"])
def test_value_cap_exact(ws, shape):
    """_stack(3, 0.3) at geometry_scale 2^20: every lane of every wave hands AccumS32x5 +-(1 - 2^-24) in all five channels -- the
    largest lo26 and hi7 sums its biased wave reductions can carry, and |v| 2^32 one ulp from overflow.  The reference's tolerance
    is 0 there: the device's words are net (2^32 - 256), exactly."""
    c = _ctx(ws, bin_request=0, **SHAPES[shape])
    try:
        gpc, args = blend_ref.device_scene(ws, gf.cap_rows(), gf.TILE)
        f = _Frame(ws, c, gpc, args)
        acc = ws.GeomGrad(c, f.n)
        try:
            frame = f.frame()
            n, s = f.n, gf.CAP_S

            def make():
                ramp, _ = gf.masked_ramp(frame, gf.TILE, gf.MASK_CAP_GENERAL)
                return gf.exact_cap_plane(frame, gf.TILE, n, gf.red_plane(*gf.TILE)), (ramp, gf.stage_a(frame, gf.TILE, n, ramp, s)), \
                    gf.exact_cap_plane(frame, gf.TILE, n, ramp)
            (g, want, share), (ramp, ramp_want), (gx, want_x, share_x) = _shared("cap", frame, make)
            # (1, 0, 0, 0): exact
            case = f"7-cap-red-{shape}"
            q = _stage_a(f, g, s)
            expected = want["net"] * ref.Q_CAP
            assert want["counted"].min() >= 1024 * (1 - gf.MASK_CAP_OPEN) and (want["capped"] == want["counted"][:, None]).all()
            row = dict(case=case, masked_share=share, words_differing=int((q != expected).sum()), **gf.summary(q, want))
            REPORT.append(row)
            print(json.dumps(row))
            assert np.array_equal(q, expected), "\n".join(_hex_rows(q, expected))
            assert np.array_equal(_stage_a(f, -g, s), -q)
            most = want["counted"][:, None] * ref.Q_CAP
            assert (np.abs(q) <= most).all() and np.array_equal(np.abs(q[:, [2, 4]]), np.repeat(most, 2, axis=1))
            # the full call on these sums (2^42: exact in f64): the spread equals the twin word for word, everything finite
            f.r.accumulate_geometry_gradient(f.pc, acc, g, background=BG, geometry_scale=s)
            got = acc.download()
            assert acc.frames == 1 and not acc._debug_scratch().any()
            twin, _ = _twin_rows(f, args, frame, q, s)
            assert np.array_equal(got["seen"], np.ones(n, np.uint64)) and np.array_equal(twin["seen"], got["seen"])
            for key in ("position", "covariance", "screen_norm"):
                assert np.isfinite(got[key]).all() and np.array_equal(got[key].view(np.uint64), twin[key].view(np.uint64)), key
            assert (got["covariance"] != 0).any(axis=1).all()
            # the signed ramp: a pair or two per layer straddle the cap; within the cap-aware bounds
            q2 = _stage_a(f, ramp, s)
            row = _compare(f"7-cap-ramp-{shape}", q2, ramp_want, min_drawn=n, tight=True, report=True)
            assert int(ramp_want["band"].sum()) == 0 and (ramp_want["capped"] >= 1000).all()
            # ... and with the open pixels masked, exact again; here m0, m1 and S01 are not 0
            q3 = _stage_a(f, gx, s)
            expected_x = want_x["net"] * ref.Q_CAP
            assert (want_x["net"] != 0).all() and np.array_equal(q3, expected_x), "\n".join(_hex_rows(q3, expected_x))
            row["masked_share_exact"] = share_x
        finally:
            acc.close()
            f.close()
    finally:
        c.close()


def test_nan_becomes_zero_and_infinity_the_cap(ws):
    """The one way a NaN reaches geom_value through the public call: a record whose f16 colour is infinite.  _stack(3, 0.3) with the
    middle layer's red far above 65504, under (1, 0, 0, 0).  F_r = inf at every pixel.  Layer 0 (in front): d_r = r (inf - P) -
    w c = +inf, t = +inf, every value +-inf with the sign of its p factors: capped, five exact integers.  Layers 1 and 2: P_r = inf,
    F_r - P_r is NaN, every value NaN: exactly 0."""
    c = _ctx(ws, bin_request=0)
    try:
        rows = gf.cap_rows()
        rows[1, 6] = 1e6            # f_dc red: 0.5 + 0.28 f_dc ~ 2.8e5, beyond binary16
        gpc, args = blend_ref.device_scene(ws, rows, gf.TILE)
        f = _Frame(ws, c, gpc, args)
        acc = ws.GeomGrad(c, f.n)
        try:
            frame = f.frame()
            h = splat_halves(frame, f.n)
            assert np.isposinf(h[1, 6]) and np.isfinite(np.delete(h, 1, 0)).all() and np.isfinite(h[1, [0, 1, 2, 3, 4, 5, 7, 8, 9]]).all()
            g = gf.red_plane(*gf.TILE)
            q = _stage_a(f, g, 1.0)
            # the signs of layer 0's p0, p1 at every pixel, from its record in float64 (|p| >= 0.03 at the pixel centres: far from 0)
            slot = int(np.nonzero(frame["src_index"].astype(np.int64) == 0)[0][0])
            halves = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
            I, (cx, cy) = ref._iprime(halves[slot], 32.0, 32.0)
            dx, dy = np.arange(32)[None, :] + 0.5 - cx, np.arange(32)[:, None] + 0.5 - cy
            p0, p1 = I[0, 0] * dx + I[0, 1] * dy, I[1, 0] * dx + I[1, 1] * dy
            e0, e1 = ref.p_error(I, dx, dy, cx, cy, 32.0, 32.0)
            assert (np.abs(p0) > 100 * e0).all() and (np.abs(p1) > 100 * e1).all() and (p0 * p0 + p1 * p1 < ref.CUT_A * ref.LOG2E * 0.9).all()
            net = [int(np.sign(p0).sum()), int(np.sign(p1).sum()), 1024, int(np.sign(p0 * p1).sum()), 1024]
            expected = np.zeros((3, 5), np.int64)
            expected[0] = np.array(net, np.int64) * ref.Q_CAP
            assert np.array_equal(q, expected), "\n".join(_hex_rows(q, expected))
            assert np.array_equal(_stage_a(f, -g, 1.0), -q)
            # the full call stays finite, and only layer 0 is seen
            f.r.accumulate_geometry_gradient(f.pc, acc, g, background=BG)
            got = acc.download()
            assert got["seen"].tolist() == [1, 0, 0] and all(np.isfinite(got[k]).all() for k in ("position", "covariance", "screen_norm"))
            assert not acc._debug_scratch().any() and f.r.errors()[0] == 0
        finally:
            acc.close()
            f.close()
    finally:
        c.close()
