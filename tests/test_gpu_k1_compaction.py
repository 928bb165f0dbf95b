"""K1's ordered compaction (web-splat_amd/csrc/preprocess.hip k_preprocess) under visibility patterns the caller decides
(tests/k1_patterns.py; tests/test_k1_patterns.py shows on the CPU that every cloud used here has `visible set == mask` with
10 % to spare at every cull threshold, and that the frame checker reports what a wrong compactor leaves behind).

Random clouds give every wave a mix of survivors and culled lanes.  These frames hold what they never do: ballots of 0 and of
all 64 lanes, empty item rows, workgroups of aggregate 0, more than 64 of those in a row in front of a look-back, block counts
that are exact multiples of 64, a last block of 1 or 17 Gaussians, clouds smaller than a wave.  Per prepared frame, each
assertion against something other than the kernel under test:

  1. by construction: num_visible == mask.sum(), src_index == nonzero(mask), no overflow, no error bit
  2. the oracle's frame of the same cloud and uniforms, within the project's K1 bounds (compare_frame "oracle")
  3. the frame of the SURVIVORS ALONE (PointCloud.subset, same bbox / centre / uniforms) on a fresh renderer, bit for bit:
     splats, keys, sorted, z, the tile lists, the counters, the binning tile and the image.  K1's per-Gaussian maths does not
     depend on a Gaussian's neighbours, so these are identical, not merely close
  4. the z plane (depth form) against numpy's f32 view-space depth of xyz[src_index], within its 2-ulp bound, and > 0

in the forms {uncompressed, compressed} x {640 x 480: packed footprint rectangles, 8256 x 80: tile counts} x {capture,
contrib + depth: the DEPTH instantiation, binning tile decided on the device}; then many frames on ONE renderer (epoch tags,
ticket, counters, stale slots) and frames in flight.  The maths of k1_math, the SH degrees and the render settings stay with
tests/test_gpu_preprocess.py and tests/test_gpu_wgsl_golden.py."""
import json
import os

import numpy as np
import pytest

import k1_patterns as kp
from k1_patterns import N_BIG, N_EDGES
from test_gpu_aux import _numpy_z

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3, 0.4)
MODES = ("capture", "depth")
MAX_INEXACT = 0.02          # of the halves, and of the keys, not bit-identical to the oracle's (tests/test_gpu_preprocess.py)
POOL_MIN_SURVIVORS = 1000   # frames below this do not enter the pooled fractions (one half of a one-splat frame is 10 %)

POOL = {}                   # test name -> form -> tally of compare_frame(..., "oracle") over that test's frames
BINNING_TILES = {}          # form -> the binning tiles its frames used (the depth form lets the device decide, from K1's tile sums)


def _vp_id(v):
    return f"{v[0]}x{v[1]}"


def _renderer(ws, ctx, compressed, mode):
    r = ws.GaussianRenderer(ctx, "rgba32float", kp.SH_DEG, compressed)
    if mode == "capture":
        r.enable_capture(True)
    else:
        r.enable_contrib(True)
        r.enable_depth(True)
    return r


def _frame(r, pc, args, mode):
    """Prepare + render on r and read everything back."""
    r.prepare(pc, args)
    fr = r.download_frame(with_src_index=True)
    if mode == "depth":
        fr["z"] = r.download_depths()
    r.render(pc, background=BG)
    fr["image"] = r.download_target().copy()
    fr["stats"] = r.frame_stats()
    fr["errors"] = r.errors()[0]
    fr["tile_lists"] = r.tile_lists()
    fr["binning_tile"] = r.binning_tile()
    return fr


def _fresh_frame(ws, ctx, pc, args, compressed, mode):
    r = _renderer(ws, ctx, compressed, mode)
    try:
        return _frame(r, pc, args, mode)
    finally:
        r.close()


def _assert_identical(got, want, what):
    """Two device frames, bit for bit, in everything that was read back."""
    diffs = kp.compare_frame(got, want, "bitwise")
    assert not diffs, (what, diffs)
    for a, b, part in zip(got["tile_lists"], want["tile_lists"], ("begin", "end", "entries")):
        assert np.array_equal(a, b), (what, "tile lists", part)
    assert got["stats"]["num_visible"] == want["stats"]["num_visible"], what
    assert got["stats"]["num_tile_entries"] == want["stats"]["num_tile_entries"], what
    assert got["binning_tile"] == want["binning_tile"], what
    assert np.array_equal(got["image"].view(np.uint32), want["image"].view(np.uint32)), (what, "image")


def _form(cl, mode):
    return f"{cl.layout}/{_vp_id(cl.viewport)}/{mode}"


def _run_case(ws, ctx, oracle, cl, test):
    """Assertions 1-4 on cl in both renderer modes."""
    idx = np.nonzero(cl.mask)[0].astype(np.uint32)
    v = len(idx)
    want = cl.oracle_frame(oracle)
    cu, rs = cl.uniforms(oracle)
    znp, ztol = _numpy_z(list(cu.view), cl.xyz[idx])
    pc = ws.PointCloud(ctx, cl.gpc)
    sub = None
    try:
        assert bytes(pc.settings_uniform(cl.args)) == bytes(rs)       # the uniforms the CPU test checked the mask under
        try:
            sub = pc.subset(idx)
        except ws.WebSplatError:
            assert v == 0                                                # an empty subset is refused: compared with "nothing" below
        if sub is not None:
            assert sub.num_points() == v
            assert bytes(sub.settings_uniform(cl.args)) == bytes(pc.settings_uniform(cl.args))
        for mode in MODES:
            what = (cl.name, cl.n, cl.variant, _form(cl, mode))
            fr = _fresh_frame(ws, ctx, pc, cl.args, cl.compressed, mode)
            # 1. by construction
            assert fr["num_visible"] == v == fr["stats"]["num_visible"], what
            assert np.array_equal(fr["src_index"], idx), (what, "src_index is not nonzero(mask)")
            assert fr["stats"]["overflow"] == 0 and fr["errors"] == 0, (what, fr["stats"], fr["errors"])
            BINNING_TILES.setdefault(_form(cl, mode), set()).add(fr["binning_tile"])
            # 2. the oracle (and 4.: numpy's z with its bound rides in the wanted frame)
            w = dict(want)
            if mode == "depth":
                assert len(fr["z"]) == v, what
                w["z"], w["z_tol"] = znp, ztol
            tally = {}
            diffs = kp.compare_frame(fr, w, "oracle", key_ulp=1 if cl.compressed else 2, tally=tally)
            assert not diffs, (what, diffs)
            if v >= POOL_MIN_SURVIVORS:
                t = POOL.setdefault(test, {}).setdefault(_form(cl, mode), {})
                for k, x in tally.items():
                    t[k] = max(t.get(k, 0), x) if k == "key_max" else t.get(k, 0) + x
                t["frames"] = t.get("frames", 0) + 1
            # 3. the survivors alone, bit for bit
            if sub is not None:
                alone = _fresh_frame(ws, ctx, sub, cl.args, cl.compressed, mode)
                assert np.array_equal(alone["src_index"], np.arange(v, dtype=np.uint32)), what
                assert alone["stats"]["overflow"] == 0 and alone["errors"] == 0, what
                _assert_identical(fr, dict(alone, src_index=idx), what)
            else:
                assert fr["stats"]["num_tile_entries"] == 0 and len(fr["tile_lists"][2]) == 0, what
                assert np.array_equal(fr["image"], np.broadcast_to(np.array(BG, dtype=np.float32), fr["image"].shape)), what
    finally:
        if sub is not None:
            sub.close()
        pc.close()


# ---- the patterns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", kp.cases(kp.PATTERNS))
def test_patterns_uncompressed_640x480(ws, ctx, oracle, name, variant):
    _run_case(ws, ctx, oracle, kp.cloud(ws, name, N_BIG, "uncompressed", variant, (640, 480)), "patterns_full")


OTHER_FORMS = [("uncompressed", (8256, 80)), ("compressed", (640, 480)), ("compressed", (8256, 80))]


@pytest.mark.parametrize("name,variant", kp.cases(kp.REDUCED))
@pytest.mark.parametrize("layout,viewport", OTHER_FORMS, ids=[f"{lay}-{_vp_id(v)}" for lay, v in OTHER_FORMS])
def test_patterns_other_forms(ws, ctx, oracle, layout, viewport, name, variant):
    _run_case(ws, ctx, oracle, kp.cloud(ws, name, N_BIG, layout, variant, viewport), "patterns_other_forms")


@pytest.mark.parametrize("name,variant", kp.cases(kp.EDGE_PATTERNS))
@pytest.mark.parametrize("n", N_EDGES)
@pytest.mark.parametrize("layout", kp.LAYOUTS)
def test_patterns_edge_sizes(ws, ctx, oracle, layout, n, name, variant):
    _run_case(ws, ctx, oracle, kp.cloud(ws, name, n, layout, variant, (640, 480)), "patterns_edge_sizes")


# ---- one renderer, many frames ---------------------------------------------------------------------------------------------
SEQUENCE = [("all", N_BIG), ("none", N_BIG), ("last_only", N_BIG), ("all", 65), ("tail_after_66_empty", N_BIG), ("ramp", N_BIG),
            ("all", N_BIG)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", kp.LAYOUTS)
def test_many_frames_on_one_renderer(ws, ctx, layout, mode):
    """68 workgroups, then none visible, then one, then a cloud of ONE workgroup, then 66 empty workgroups in front of the
    survivors ...: the status words keep the tags of earlier frames (they are never re-zeroed), the ticket and the counters
    are reused, slots beyond the visible count keep stale splats.  Every frame equals a fresh renderer's, bit for bit."""
    r = _renderer(ws, ctx, layout == "compressed", mode)
    try:
        for step, (name, n) in enumerate(SEQUENCE):
            cl = kp.cloud(ws, name, n, layout, None, (640, 480))
            pc = ws.PointCloud(ctx, cl.gpc)
            try:
                got = _frame(r, pc, cl.args, mode)
                want = _fresh_frame(ws, ctx, pc, cl.args, layout == "compressed", mode)
                what = (step, name, n, layout, mode)
                assert got["num_visible"] == int(cl.mask.sum()), what
                assert np.array_equal(want["src_index"], np.nonzero(cl.mask)[0]), what
                assert got["errors"] == 0 and got["stats"]["overflow"] == 0, what
                _assert_identical(got, want, what)
            finally:
                pc.close()
    finally:
        r.close()


# ---- frames in flight ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ramp", "one_per_block"])
def test_frames_in_flight(ws, ctx, name):
    """Nine views over four slots (ws_view_batch_*): K1 launches of several frames run beside each other, each with its own
    ticket, status words and counters.  The clipping box decides visibility for every camera (tests/test_k1_patterns.py), so
    every frame compacts the same pattern; every image equals the lone renderer's."""
    w, h = 640, 480
    cl = kp.cloud(ws, name, N_BIG, "uncompressed", "clip", (w, h))
    views = kp.orbit_views(ws, cl, 9)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = ws.GaussianRenderer(ctx, "rgba32float", kp.SH_DEG, False)
    batch = ws.ViewBatch(ctx, "rgba32float", kp.SH_DEG, False, frames_in_flight=4)
    bufs = [ctx.malloc(w * h * 16) for _ in views]
    try:
        assert batch.frames_in_flight == 4
        alone = []
        for v in views:
            r.prepare(pc, v)
            r.render(pc, background=BG)
            alone.append(r.download_target().copy())
            assert r.frame_stats()["num_visible"] == int(cl.mask.sum()) and r.errors()[0] == 0
        assert len({a.tobytes() for a in alone}) == len(alone)          # nine different images
        for rep in range(2):
            batch.render(pc, views, bufs, w * 16, background=BG)
            batch.sync()
            for i in range(len(views)):
                got = ctx.download(bufs[i], (h, w, 4), np.float32)
                assert np.array_equal(got.view(np.uint32), alone[i].view(np.uint32)), (name, rep, i)
        assert batch.errors() == 0
    finally:
        for b in bufs:
            ctx.free(b)
        batch.close()
        r.close()
        pc.close()


# ---- the pooled fractions (keep this test last) ----------------------------------------------------------------------------
def _fractions(t):
    return {"frames": t["frames"], "survivors": t["keys"],
            "halves_not_identical": t["halves_inexact"] / t["halves"], "keys_not_identical": t["keys_inexact"] / t["keys"],
            "largest_key_difference": t["key_max"]}


def _merge(tallies):
    out = {}
    for t in tallies:
        for k, x in t.items():
            out[k] = max(out.get(k, 0), x) if k == "key_max" else out.get(k, 0) + x
    return out


def test_pooled_fractions_within_the_caps(ws, ctx, oracle):
    """"Within one ulp" must not hide a systematic error: at most 2 % of the halves and 2 % of the keys may differ from the
    oracle's at all -- over the pooled frames (of at least 1000 survivors) of each parametrised test above, and over the whole
    module.  (Per frame the cap would be meaningless: one half of a one-survivor frame is 10 %.)  Run alone, this test prepares
    random_50 in every form first.  The figures go to k1_compaction_report.json in
    WEBSPLAT_REPORT_DIR (default: test_reports/ under the repository root, as tests/test_gpu_blend_boundary.py)."""
    if not POOL:
        for layout in kp.LAYOUTS:
            for viewport in kp.VIEWPORTS:
                _run_case(ws, ctx, oracle, kp.cloud(ws, "random_50", N_BIG, layout, "clip", viewport), "random_50_only")
    report = {"caps": {"halves_not_identical": MAX_INEXACT, "keys_not_identical": MAX_INEXACT}, "tests": {}, "forms": {}}
    forms = {}
    for test, by_form in POOL.items():
        report["tests"][test] = _fractions(_merge(by_form.values()))
        for form, t in by_form.items():
            forms.setdefault(form, []).append(t)
    for form, ts in sorted(forms.items()):
        report["forms"][form] = dict(_fractions(_merge(ts)), binning_tiles=sorted(BINNING_TILES.get(form, ())))
    report["module"] = _fractions(_merge(t for by_form in POOL.values() for t in by_form.values()))
    report["bit_identical_to_the_oracle"] = (report["module"]["halves_not_identical"] == 0
                                             and report["module"]["keys_not_identical"] == 0)
    print(json.dumps(report, indent=1))
    out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "k1_compaction_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    for what, fr in list(report["tests"].items()) + [("module", report["module"])]:
        assert fr["halves_not_identical"] <= MAX_INEXACT, (what, fr)
        assert fr["keys_not_identical"] <= MAX_INEXACT, (what, fr)
