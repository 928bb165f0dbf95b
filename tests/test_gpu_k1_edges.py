"""K1's cull comparisons and splat maths on the device (web-splat_amd/csrc/preprocess.hip k1_project / k1_math) on the chosen
Gaussians of tests/k1_edges.py; tests/test_k1_edges.py shows on the CPU that every window straddles its threshold, that every
case reaches the branch it is named for and that the f32 oracle alone meets the float64 caps used here.

  (a) cull decisions, exact: on every threshold window the device keeps exactly the Gaussians the oracle keeps -- uncompressed
      and compressed, packed and tile-count footprint, plain and DEPTH form, axis and oblique camera; K1c keeps z == 0 and
      z == 1, K1 does not
  (b) records: every case frame within the project's oracle bounds (tests/k1_patterns.py compare_frame "oracle"); the
      degenerates, whose value is a convention and not a computation, to the bit; the finite cases within the float64 caps;
      one-hot SH colours against the closed-form basis for max_sh_deg 0 .. 3
  (c) hostile Gaussians (NaN position, NaN / inf covariance, axes beyond f16, zero covariance with kernel_size 0) reach no tile
      and leave the image bit-identical to the one of the ordinary Gaussians alone
  (d) fade-in: walltime == dd, the shortcut's boundary (walltime 10.999 / 11.0), and a declared centre outside the bbox

Each test is a few prepare() calls on 2101 Gaussians.  The figures go to k1_edges.json in WEBSPLAT_REPORT_DIR (default:
test_reports/ under the repository root, as tests/test_gpu_metrics.py)."""
import json
import os

import numpy as np
import pytest

import k1_edges as ke
import k1_patterns as kp
from variants import exp_param

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3, 0.4)
MODES = ("capture", "depth")
FORMS = [(cam, vp) for cam in ke.CAMERAS for vp in ke.VIEWPORTS]
FORM_IDS = [f"{cam}-{vp[0]}x{vp[1]}" for cam, vp in FORMS]

REPORT = {"tests": set(), "cases": [], "slots": 0, "tally": {}, "oracle_vs_float64": {}, "device_vs_float64": {}}


def _renderer(ws, ctx, compressed, mode="capture"):
    r = ws.GaussianRenderer(ctx, "rgba32float", ke.SH_DEG, compressed)
    if mode == "capture":
        r.enable_capture(True)
    else:
        r.enable_contrib(True)
        r.enable_depth(True)
    return r


def _prepare(r, pc, args):
    r.prepare(pc, args)
    fr = r.download_frame(with_src_index=True)
    fr["stats"] = r.frame_stats()
    fr["errors"] = r.errors()[0]
    return fr


def _against_oracle(cl, oracle, fr, want, what):
    """compare_frame "oracle" (the project's bounds: halves within 1 ulp, equal NaN pattern, keys within 2 / 1), tallied.  The
    NaN pattern covers K1's keys as well: the depth key of a NaN position is a NaN on both sides, of either sign."""
    tally = {}
    diffs = kp.compare_frame(fr, want, "oracle", key_ulp=1 if cl.compressed else 2, tally=tally, nan_keys=not cl.compressed)
    assert not diffs, (what, diffs)
    assert fr["errors"] == 0, (what, fr["errors"])
    if not cl.compressed and int(fr["num_visible"]):
        # K1's NaN keys sort behind every real depth, whatever their sign: every other key is at most +inf as a u32, and the
        # slots with a NaN key are the tail of the sorted order
        gk = np.asarray(fr["keys"]).astype(np.int64)
        knan = (gk & 0x7FFFFFFF) > 0x7F800000
        assert not (~knan).any() or gk[~knan].max() <= 0x7F800000, what
        n_nan = int(knan.sum())
        assert n_nan == 0 or knan[np.asarray(fr["sorted"])[-n_nan:]].all(), (what, "a NaN key is not at the end of the order")
    REPORT["tests"].add(os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0])
    t = REPORT["tally"]
    for k, x in tally.items():
        t[k] = max(t.get(k, 0), x) if k == "key_max" else t.get(k, 0) + x
    REPORT["slots"] += int(want["num_visible"])
    REPORT["cases"].append("/".join(str(x) for x in what))


def _halves(frame, cl, name):
    slot = np.nonzero(np.asarray(frame["src_index"]) == cl.index[name])[0]
    assert len(slot) == 1, (name, "not visible")
    return np.ascontiguousarray(frame["splats"]).view(np.uint16).reshape(-1, 10)[slot[0]]


def _deviation(cl, f, frame, names, who):
    rows = np.array([cl.index[n] for n in names])
    src = np.asarray(frame["src_index"])
    slots = np.array([np.nonzero(src == r)[0][0] for r in rows])
    fields = {k: v[slots] for k, v in ke.splat_fields(frame["splats"], cl.viewport).items()}
    dev = ke.f64_deviation(fields, f, rows)
    for q, x in dev.items():
        REPORT[who][q] = max(REPORT[who].get(q, 0.0), x)
    return dev


# ---- (a) cull decisions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ke.LAYOUTS)
@pytest.mark.parametrize("cam,vp", FORMS, ids=FORM_IDS)
def test_cull_windows_equal_the_oracle(ws, ctx, oracle, cam, vp, layout, mode):
    r = _renderer(ws, ctx, layout == "compressed", mode)
    try:
        for kind in ("frustum", "box"):
            cl = ke.window_cloud(ws, oracle, kind, cam, vp, layout)
            want = cl.oracle_frame(oracle)
            pc = ws.PointCloud(ctx, cl.gpc)
            try:
                assert bytes(pc.settings_uniform(cl.args)) == bytes(cl.uniforms(oracle)[1])
                fr = _prepare(r, pc, cl.args)
            finally:
                pc.close()
            what = ("windows", kind, cam, f"{vp[0]}x{vp[1]}", layout, mode)
            got, exp = ke.window_verdicts(cl, fr["src_index"]), ke.window_verdicts(cl, want["src_index"])
            for w in cl.info["windows"]:
                assert np.array_equal(got[w.name], exp[w.name]), (what, w.name, got[w.name], exp[w.name])
            assert np.array_equal(fr["src_index"], want["src_index"]), what
            _against_oracle(cl, oracle, fr, want, what)
    finally:
        r.close()


@pytest.mark.parametrize("vp", ke.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_k1c_keeps_the_exact_planes_and_k1_does_not(ws, ctx, oracle, vp):
    """Camera depth 0.5 = znear gives clip z == 0 exactly; some floats under zfar give clip z == w exactly."""
    seen = {}
    for layout in ke.LAYOUTS:
        cl = ke.window_cloud(ws, oracle, "frustum", "axis", vp, layout)
        pc = ws.PointCloud(ctx, cl.gpc)
        r = _renderer(ws, ctx, cl.compressed)
        try:
            seen[layout] = ke.window_verdicts(cl, _prepare(r, pc, cl.args)["src_index"])
        finally:
            r.close()
            pc.close()
    near = next(w for w in cl.info["windows"] if w.name == "near")
    at = int(np.nonzero(near.values == np.float32(ke.AXIS_ZNEAR))[0][0])
    assert not seen["uncompressed"]["near"][at] and seen["compressed"]["near"][at]
    assert np.array_equal(np.delete(seen["uncompressed"]["near"], at), np.delete(seen["compressed"]["near"], at))
    apart = seen["uncompressed"]["far"] != seen["compressed"]["far"]
    assert apart.any() and seen["compressed"]["far"][apart].all() and not seen["uncompressed"]["far"][apart].any()


def _no_index(fr):
    return dict(fr, src_index=np.zeros(0, dtype=np.uint32))


@pytest.mark.parametrize("group", [exp_param(2)])
def test_grouped_k1_culls_the_same(ws, oracle, monkeypatch, group):
    """WS_BATCH_K1=2 (experimental build): two views share one K1 launch (k_preprocess_multi).  Per window cloud the two views
    are the cloud with its own clipping box and with the other kind's.  A grouped prepare refuses capture, so there is no
    src_index; the SET is pinned through the store-ordered frame instead: each slot's splats, keys and sorted order equal, bit
    for bit, those of a plain renderer of the same view, which in turn hold the oracle's visible set in the oracle's order
    (as many slots, every record and key within the oracle bounds at its own slot: the windows' Gaussians differ in position,
    so a swapped survivor moves a centre or a key by far more than a bound).  The library has no counter that tells whether
    the group path ran; what makes it fall back silently (a frame graph, timers, capture, contrib, depth) is ruled out here."""
    monkeypatch.setenv("WS_BATCH_K1", str(group))
    monkeypatch.delenv("WS_GRAPH", raising=False)
    cfg = ws.config_from_env()
    assert cfg.exp_batch_k1 == group and cfg.use_graph == 0 and cfg.debug_cut == 0
    w, h = 640, 480
    c = ws.Context(0)
    try:
        for layout in ke.LAYOUTS:
            for kind in ("frustum", "box"):
                cl = ke.window_cloud(ws, oracle, kind, "axis", (w, h), layout)
                lo, hi, _ = ke.user_box("axis", (w, h))
                other = None if kind == "box" else ws.Aabb([float(v) for v in lo], [float(v) for v in hi])
                views = [cl.args, cl.with_args(ws, clipping_box=other)]
                pc = ws.PointCloud(c, cl.gpc)
                r = ws.GaussianRenderer(c, "rgba32float", ke.SH_DEG, cl.compressed)
                batch = ws.ViewBatch(c, "rgba32float", ke.SH_DEG, cl.compressed, frames_in_flight=2)
                bufs = [c.malloc(w * h * 16) for _ in views]
                try:
                    assert batch.frames_in_flight == 2
                    alone = []
                    for i, v in enumerate(views):
                        r.prepare(pc, v)
                        fr = _no_index(r.download_frame())
                        r.render(pc, background=BG)
                        fr["image"] = r.download_target().copy()
                        want = _no_index(cl.oracle_frame(oracle, v))
                        diffs = kp.compare_frame(fr, want, "oracle", key_ulp=1 if cl.compressed else 2)
                        assert not diffs, (layout, kind, i, diffs)
                        alone.append(fr)
                    assert alone[0]["num_visible"] != alone[1]["num_visible"]
                    batch.render(pc, views, bufs, w * 16, background=BG)
                    batch.sync()
                    assert batch.errors() == 0
                    for i in range(len(views)):
                        got = _no_index(batch.renderer(i).download_frame())
                        diffs = kp.compare_frame(got, alone[i], "bitwise")
                        assert not diffs, (layout, kind, i, diffs)
                        img = c.download(bufs[i], (h, w, 4), np.float32)
                        assert np.array_equal(img.view(np.uint32), alone[i]["image"].view(np.uint32)), (layout, kind, i)
                finally:
                    for b in bufs:
                        c.free(b)
                    batch.close()
                    r.close()
                    pc.close()
    finally:
        c.close()


# ---- (b) records -------------------------------------------------------------------------------------------------------------
def _finite_names(frame):
    skip = () if frame in ("k0", "scaling_zero") else ("wide_on_axis", "needle")        # their axis is rounding noise unless exact
    return [n for n in ke.FINITE if n not in skip]


def _maths_frames(ws, ctx, oracle, vp):
    cl = ke.maths_cloud(ws, "uncompressed", vp)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, False)
    out = {}
    try:
        for frame, kw in ke.MATHS_FRAMES.items():
            args = cl.with_args(ws, **kw)
            assert bytes(pc.settings_uniform(args)) == bytes(cl.uniforms(oracle, args)[1])
            fr, want = _prepare(r, pc, args), cl.oracle_frame(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("maths", frame, f"{vp[0]}x{vp[1]}"))
            out[frame] = (fr, want, cl.f64(oracle, args))
    finally:
        r.close()
        pc.close()
    return cl, out


def test_maths_cases_640x480(ws, ctx, oracle):
    cl, frames = _maths_frames(ws, ctx, oracle, (640, 480))
    # the degenerates: a convention, so to the bit
    fr, want, f = frames["k0"]
    s1 = _halves(want, cl, "iso_on_axis")
    for nm in ("iso_on_axis", "wide_on_axis"):                       # v1 = (s1, 0), v2 = (0, -s2)
        h, o = _halves(fr, cl, nm), _halves(want, cl, nm)
        assert np.array_equal(h[0:4], o[0:4]), (nm, h, o)
        assert h[0] & 0x7FFF and not h[0] & 0x8000 and (h[1] & 0x7FFF) == 0 and (h[2] & 0x7FFF) == 0 and h[3] & 0x8000, (nm, h)
    assert _halves(fr, cl, "iso_on_axis")[0] == s1[0]
    h = _halves(fr, cl, "zero_cov")                                   # v1 = (0, 0); v2 = (0, -sqrt(0.2))
    assert h[0] == 0 and (h[1] & 0x7FFF) == 0 and (h[2] & 0x7FFF) == 0, h
    assert np.array_equal(h[0:4] & 0x7FFF, _halves(want, cl, "zero_cov")[0:4] & 0x7FFF)
    for nm in ("needle", "tiny_iso"):                                 # lambda2 on the 0.1 clamp: v2 = sqrt(0.2) in px, exactly
        h = _halves(fr, cl, nm)
        assert np.array_equal(h[2:4], _halves(want, cl, nm)[2:4]), nm
        assert abs(float(np.array(h[3]).view(np.float16)) * 480.0 + np.sqrt(2.0 * ke.C_0P1)) < 2.0 ** -11, nm
    fr, want, f = frames["mip"]
    assert _halves(fr, cl, "zero_cov")[9] == 0x0000                   # mip_cut: coef = 0
    fr, want, f = frames["k03"]
    assert _halves(fr, cl, "op_zero")[9] == 0x0000
    for nm, bits in (("op_one", 0x3C00), ("op_1p5", 0x3E00), ("op_subnormal", 0x0001)):
        assert _halves(fr, cl, nm)[9] == bits, nm
    assert not _halves(fr, cl, "col_exact_zero")[6:9].any() and not _halves(fr, cl, "col_negative")[6:9].any()
    assert (_halves(fr, cl, "col_overflow")[6:9] == 0x7C00).all()
    assert _halves(fr, cl, "nan_sh")[7] == 0
    for nm in ("nan_x", "nan_y", "nan_z"):
        slot = np.nonzero(fr["src_index"] == cl.index[nm])[0][0]
        assert (int(fr["keys"][slot]) & 0x7FFFFFFF) > 0x7F800000, (nm, hex(int(fr["keys"][slot])))       # a NaN key
    # the finite cases against float64, under the caps the oracle meets on the CPU
    for frame, (fr, want, f) in frames.items():
        names = _finite_names(frame)
        _deviation(cl, f, want, names, "oracle_vs_float64")
        dev = _deviation(cl, f, fr, names, "device_vs_float64")
        assert all(x <= 1.0 for x in dev.values()), (frame, dev)


def test_maths_cases_8256x80(ws, ctx, oracle):
    """The same frames through the tile-count footprint, against the oracle (at this width the axes of a small splat are f16
    subnormals, so the float64 caps do not apply)."""
    _maths_frames(ws, ctx, oracle, (8256, 80))


def test_maths_cases_compressed(ws, ctx, oracle):
    cl = ke.maths_cloud(ws, "compressed")
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, True)
    try:
        for kw in ({}, {"kernel_size": 0.0}):
            args = cl.with_args(ws, **kw)
            fr, want, f = _prepare(r, pc, args), cl.oracle_frame(oracle, args), cl.f64(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("maths", "compressed", "k0" if kw else "k03"))
            names = ke.COMPRESSED_FINITE if kw else ("iso_on_axis",)
            _deviation(cl, f, want, names, "oracle_vs_float64")
            dev = _deviation(cl, f, fr, names, "device_vs_float64")
            assert all(x <= 1.0 for x in dev.values()), (kw, dev)
        for nm in ("tiny_iso", "zero_cov"):                           # K1c's clamp: lambda2 = mid - 0.1 < 0, v2 is NaN
            h = _halves(fr, cl, nm)
            assert ((h[2:4] & 0x7FFF) > 0x7C00).any(), (nm, h)
    finally:
        r.close()
        pc.close()


def test_one_hot_sh_colours(ws, ctx, oracle):
    """One Gaussian per (coefficient, channel) with the value 1, seen along three directions: its colour is 0.5 plus the
    closed-form basis value in its own channel, and exactly 0.5 where the coefficient lies above max_sh_deg (a swapped SH plane
    or a wrong band limit moves a known Gaussian)."""
    cl = ke.one_hot_cloud(ws)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, False)
    try:
        for deg in range(4):
            args = cl.with_args(ws, max_sh_deg=deg)
            fr, want = _prepare(r, pc, args), cl.oracle_frame(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("one_hot", deg))
            exp = ke.one_hot_expected(deg)
            worst = 0.0
            for d in range(3):
                for k in range(16):
                    for ch in range(3):
                        got = _halves(fr, cl, f"onehot_d{d}_k{k}_c{ch}")[6:9].view(np.float16).astype(np.float64)
                        e = exp[d, k, ch]
                        worst = max(worst, float((np.abs(got - e) / (0.5 * ke.half_ulp(e) + ke.SLACK)).max()))
                        if k >= (deg + 1) ** 2:
                            assert np.array_equal(got, [0.5, 0.5, 0.5]), (deg, d, k, ch, got)
            REPORT["device_vs_float64"]["one_hot_colour"] = max(REPORT["device_vs_float64"].get("one_hot_colour", 0.0), worst)
            assert worst <= 1.0, (deg, worst)
    finally:
        r.close()
        pc.close()


# ---- (c) hostile Gaussians ---------------------------------------------------------------------------------------------------
def _drawn(r, pc, args):
    fr = _prepare(r, pc, args)
    r.render(pc, background=BG)
    fr["image"] = r.download_target().copy()
    fr["stats"] = r.frame_stats()
    fr["errors"] = r.errors()[0]
    fr["tile_lists"] = r.tile_lists()
    return fr


@pytest.mark.parametrize("which", ["hostile", "overflow"])
@pytest.mark.parametrize("vp", ke.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_hostile_gaussians_do_not_leak(ws, ctx, oracle, vp, which):
    cl = ke.hostile_cloud(ws, vp) if which == "hostile" else ke.overflow_cloud(ws, vp)
    assert all(ke.is_hostile(n) for n in cl.index)
    want = cl.oracle_frame(oracle)
    pc = ws.PointCloud(ctx, cl.gpc)
    sub = pc.subset(cl.ordinary.astype(np.uint32))
    r, r2 = _renderer(ws, ctx, False), _renderer(ws, ctx, False)
    try:
        assert bytes(sub.settings_uniform(cl.args)) == bytes(pc.settings_uniform(cl.args))
        fr = _drawn(r, pc, cl.args)
        _against_oracle(cl, oracle, fr, want, (which, f"{vp[0]}x{vp[1]}"))
        rows = np.array(sorted(cl.index.values()))
        slots = np.nonzero(np.isin(fr["src_index"], rows))[0]
        assert len(slots) == len(rows)                                 # every one of them IS a visible slot
        begin, end, entries = fr["tile_lists"]
        assert not np.isin(entries, slots).any(), "a hostile slot is in a tile list"
        assert fr["stats"]["overflow"] == 0 and fr["errors"] == 0, fr["stats"]
        assert np.isfinite(fr["image"]).all()
        alone = _drawn(r2, sub, cl.args)
        assert alone["stats"]["overflow"] == 0 and alone["errors"] == 0
        assert alone["num_visible"] == fr["num_visible"] - len(rows)
        assert alone["stats"]["num_tile_entries"] == fr["stats"]["num_tile_entries"] > 0
        assert np.array_equal(fr["image"].view(np.uint32), alone["image"].view(np.uint32))
        assert not np.array_equal(fr["image"], np.broadcast_to(np.array(BG, dtype=np.float32), fr["image"].shape))
    finally:
        r.close()
        r2.close()
        sub.close()
        pc.close()


# ---- (d) fade-in -------------------------------------------------------------------------------------------------------------
def test_fade_cases_equal_the_oracle(ws, ctx, oracle):
    cl = ke.fade_cloud(ws)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, False)
    try:
        for wt in ke.FADE_WALLTIMES:
            args = cl.with_args(ws, walltime=wt)
            assert bytes(pc.settings_uniform(args)) == bytes(cl.uniforms(oracle, args)[1])
            fr, want, f = _prepare(r, pc, args), cl.oracle_frame(oracle, args), cl.f64(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("fade", wt))
            _deviation(cl, f, want, list(ke.FADE_POINTS), "oracle_vs_float64")
            dev = _deviation(cl, f, fr, list(ke.FADE_POINTS), "device_vs_float64")
            assert all(x <= 1.0 for x in dev.values()), (wt, dev)
    finally:
        r.close()
        pc.close()


@pytest.mark.parametrize("user_box", [False, True], ids=["default_box", "user_box"])
def test_fade_shortcut_boundary(ws, ctx, oracle, user_box):
    """Gaussians on the corners of the bbox (dd = 5) at walltime 10.999 (full computation), 11.0 and 12.0 (shortcut, unless a
    user clip box turns it off): the same frame, bit for bit, and within the oracle's bounds."""
    cl = ke.corner_cloud(ws)
    box = ws.Aabb(list(ke.FADE_BBOX[0]), list(ke.FADE_BBOX[1])) if user_box else None
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, False)
    try:
        frames = []
        for wt in ke.CORNER_WALLTIMES:
            args = cl.with_args(ws, walltime=wt, clipping_box=box)
            fr, want = _prepare(r, pc, args), cl.oracle_frame(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("corners", wt, "user_box" if user_box else "default_box"))
            assert np.isin([cl.index[f"corner_{k}"] for k in range(8)], fr["src_index"]).all()
            frames.append(fr)
        for fr in frames[1:]:
            assert not kp.compare_frame(fr, frames[0], "bitwise")
    finally:
        r.close()
        pc.close()


def test_fade_with_the_centre_outside_the_bbox(ws, ctx, oracle):
    """ws_pointcloud_create takes the caller's centre as it is.  50 radii outside the bbox every dd is near 50: the reference
    still draws the Gaussians at scale 0 at walltime 11 and 12, so the shortcut "walltime >= 11" must not apply."""
    cl = ke.outside_cloud(ws)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = _renderer(ws, ctx, False)
    try:
        for wt in ke.OUTSIDE_WALLTIMES:
            args = cl.with_args(ws, walltime=wt)
            assert bytes(pc.settings_uniform(args)) == bytes(cl.uniforms(oracle, args)[1])
            fr, want = _prepare(r, pc, args), cl.oracle_frame(oracle, args)
            _against_oracle(cl, oracle, fr, want, ("centre_outside", wt))
    finally:
        r.close()
        pc.close()


# ---- the report (keep this test last) ------------------------------------------------------------------------------------------
def test_report(ws, ctx, oracle):
    """What was compared, and how far from bit-identical it was: not a gate of its own, the gates are above.  The figures are
    those of the tests of this module that ran before it in this process (a subset of them writes a partial report): their
    ids are in "tests_that_contributed".  Run alone, this test prepares the maths frames first."""
    if not REPORT["cases"]:
        test_maths_cases_640x480(ws, ctx, oracle)
    t = REPORT["tally"]
    rep = {"tests_that_contributed": sorted(REPORT["tests"]), "cases_run": len(REPORT["cases"]), "cases": REPORT["cases"], "slots_compared": REPORT["slots"],
           "halves_compared": t.get("halves", 0), "halves_not_bit_identical_to_the_oracle": t.get("halves_inexact", 0),
           "keys_compared": t.get("keys", 0), "keys_not_bit_identical_to_the_oracle": t.get("keys_inexact", 0),
           "largest_key_difference": t.get("key_max", 0),
           "nan_keys_with_another_sign_or_payload_than_the_oracle": t.get("nan_keys_of_other_bits", 0),
           "caps": {"sigma": "2^-9 of its largest entry", "centre / colour / opacity": "half an f16 ulp of the float64 value + 2e-6"},
           "largest_deviation_from_float64_as_a_fraction_of_the_cap": {"oracle": REPORT["oracle_vs_float64"],
                                                                       "device": REPORT["device_vs_float64"]}}
    print(json.dumps({k: v for k, v in rep.items() if k != "cases"}, indent=1))
    out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "k1_edges.json"), "w") as f:
        json.dump(rep, f, indent=1)
    assert rep["cases_run"] > 0 and rep["slots_compared"] > 0
