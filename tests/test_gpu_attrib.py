"""Weighted contribution sums and the error plane (include/websplat.h "Attributing a pixel plane to Gaussians"; contrib.hip
k_contrib<.., true>, metrics.hip k_image_error).

   1. E == 1 (three ways to say it) equals the plain sum, bitwise       7. reproducible; frames and accumulators merge exactly
   2. a 0/1 mask and its complement add up to the plain sum exactly      8. the error plane against its numpy restatement, bitwise
   3. against float64 (tests/attrib_ref.py) on c1 and a compressed cloud 9. ws_scene_accumulate_error equals the manual loop, bitwise
   4. tile lists at the staging boundaries, most quadrants idle         10. blame finds an appended floater
   5. clamp, NaN, a padded pitch                                        11. the error cases
   6. an all-zero plane                                                 12. a weighted add changes no pixel"""
import ctypes as C
import json

import numpy as np
import pytest

import attrib_ref
import metrics_ref as mr
import scenes
from attrib_frames import VIEW, F, _c1_frame, _compressed, _ctx, _Frame, _ramp_checker, _stack_frame, _u32
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu


# ---- 1. E == 1 ---------------------------------------------------------------------------------------------------------------
UNIT_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"bin_request": 2}]
_ids = lambda cfgs: ["-".join(f"{k}{v}" for k, v in c.items()) or "default" for c in cfgs]  # noqa: E731


@pytest.mark.parametrize("cfg", UNIT_CONFIGS, ids=_ids(UNIT_CONFIGS))
def test_unit_plane_equals_the_plain_sum_bitwise(ws, oracle, cfg):
    c = _ctx(ws, **cfg)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            q, m = f.plain()
            assert (q > 0).sum() > 1000
            w, h = VIEW
            anything = np.random.default_rng(1).uniform(-1e6, 1e6, size=(h, w)).astype(F)
            for name, plane, scale, bias in (("ones", np.ones((h, w), F), 1.0, 0.0), ("threes clamped", np.full((h, w), 3.0, F), 1.0, 0.0),
                                             ("anything, scale 0 bias 1", anything, 0.0, 1.0)):
                qw, mw = f.weighted(plane, scale, bias)
                assert np.array_equal(qw, q), name
                assert np.array_equal(_u32(mw), _u32(m)), name
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. partition of unity ---------------------------------------------------------------------------------------------------
def _mask(width, height, rect, dots):
    a = np.zeros((height, width), F)
    x0, x1, y0, y1 = rect
    a[y0:y1, x0:x1] = 1
    for x, y in dots:
        assert a[y, x] == 0
        a[y, x] = 1
    return a


def _check_partition(f, a):
    q, m = f.plain()
    qa, ma = f.weighted(a)
    qb, mb = f.weighted(F(1.0) - a)
    print(f"drawn {int((q > 0).sum())} in A {int((qa > 0).sum())} in B {int((qb > 0).sum())} in both {int(((qa > 0) & (qb > 0)).sum())} "
          f"zero {int((q == 0).sum())}")
    assert ((qa > 0) & (qb > 0)).any() and (qa > 0).any() and (qb > 0).any()
    assert np.array_equal(qa + qb, q)
    assert np.array_equal(np.maximum(_u32(ma), _u32(mb)), _u32(m))
    return q


def test_partition_of_unity_is_exact_c1(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:  # a rectangle with edges off the 8-px grid, and single pixels far from it
            _check_partition(f, _mask(*VIEW, (13, 211, 9, 150), [(300, 200), (250, 3), (5, 233), (317, 239), (0, 0)]))
        finally:
            f.close()
    finally:
        c.close()


def test_partition_of_unity_is_exact_on_a_saturating_stack(ws):
    """The opaque 32 x 32 stack with k = 513: every quadrant saturates after ~60 layers and the walk and the batch loop take their
    early exits.  Were the mask to steer termination, the two halves would stop at other layers than the plain walk."""
    c = _ctx(ws, bin_request=0)
    try:
        f = _stack_frame(ws, c, 513, 0.9)
        try:
            q = _check_partition(f, _mask(32, 32, (3, 21, 5, 14), [(30, 2), (1, 29), (25, 25)]))
            assert (q == 0).any() and (q > 0).any()
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. against float64 ------------------------------------------------------------------------------------------------------
def _compare(got_q, got_m, ref, min_drawn):
    tol_sum, tol_max = attrib_ref.bounds(ref)
    s = got_q.astype(np.float64) / L.WS_CONTRIB_SUM_SCALE
    d_sum, d_max = np.abs(s - ref["sum"]), np.abs(got_m.astype(np.float64) - ref["max"])
    drawn = int((got_q > 0).sum())
    ws_, wm = int(np.argmax(d_sum - tol_sum)), int(np.argmax(d_max - tol_max))
    print(f"gaussians {len(d_sum)} drawn {drawn} with P {int((ref['P'] > 0).sum())} with U {int((ref['U'] > 0).sum())}; sum: max |d| "
          f"{d_sum.max():.3e}, worst excess {(d_sum - tol_sum)[ws_]:.3e} at {ws_} (ref {ref['sum'][ws_]:.6e}, tol {tol_sum[ws_]:.3e}); "
          f"max: max |d| {d_max.max():.3e}, worst excess {(d_max - tol_max)[wm]:.3e} at {wm}")
    assert drawn > min_drawn
    assert np.array_equal(got_q == 0, got_m == 0)
    assert np.all(d_sum <= tol_sum), f"{int((d_sum > tol_sum).sum())} sums out of bound"
    assert np.all(d_max <= tol_max), f"{int((d_max > tol_max).sum())} maxima out of bound"


F64_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"blend_split": 1}]
_REF = {}  # K1 and the depth sort do not depend on the tile configuration: one float64 walk serves the three


@pytest.mark.parametrize("cfg", F64_CONFIGS, ids=_ids(F64_CONFIGS))
def test_against_f64_c1(ws, oracle, cfg):
    c = _ctx(ws, **cfg)
    try:
        f = _c1_frame(ws, oracle, c, seed=0)
        try:
            e = _ramp_checker(*VIEW)
            q, m = f.weighted(e)
            frame = f.frame()
            hit = _REF.get("c1")
            if hit is None or not all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
                hit = _REF["c1"] = (frame, attrib_ref.attrib_f64(frame, VIEW[0], VIEW[1], f.n, attrib_ref.clamp_plane(e)))
            _compare(q, m, hit[1], 1000)
        finally:
            f.close()
    finally:
        c.close()


def test_against_f64_compressed(ws):
    c = _ctx(ws)
    try:
        gpc, args = _compressed(ws)
        f = _Frame(ws, c, gpc, args, compressed=True)
        try:
            e = _ramp_checker(400, 300)
            q, m = f.weighted(e)
            _compare(q, m, attrib_ref.attrib_f64(f.frame(), 400, 300, f.n, attrib_ref.clamp_plane(e)), 1000)
        finally:
            f.close()
    finally:
        c.close()


# ---- 4. staging boundaries with idle quadrants --------------------------------------------------------------------------------
BOUNDARY_CASES = [({}, k) for k in (1, 512, 513)] + [({"tile_qw": 2, "tile_qh": 2}, k) for k in (256, 257)]
T_MIN = 2.0 ** -14


@pytest.mark.parametrize("opacity", [0.002, 0.9], ids=["faint", "opaque"])
@pytest.mark.parametrize("cfg,k", BOUNDARY_CASES, ids=[f"{'2x2' if c else '4x4'}-{k}" for c, k in BOUNDARY_CASES])
def test_list_lengths_at_staging_boundaries(ws, cfg, k, opacity):
    """Tile lists of exactly k entries (STAGE = 512 at the 4x4 tile, 256 at 2x2).  E = 1 on the quadrant [8, 16) x [8, 16) and on one
    pixel of the quadrant [16, 24) x [0, 8): two waves walk, every other quadrant is all-zero and only stages and votes.
    Faint: T stays above T_MIN, every batch is walked to its end and every Gaussian draws.  Opaque: the two walking quadrants
    saturate inside the first batch; a wave looks at its pixels' T after every fourth record, so at most three records behind the
    first one whose 64 pixels are all below T_MIN still add something -- one more for the gap between the device's f32 T and the
    reference's (T falls by more than 15 % per layer, the two differ by far less) -- and everything from the eighth on is exactly 0."""
    c = _ctx(ws, bin_request=0, **cfg)
    try:
        f = _stack_frame(ws, c, k, opacity)
        try:
            assert int(f.r.tile_stats()["list_len"].max()) == k
            e = np.zeros((32, 32), F)
            e[8:16, 8:16] = 1
            e[3, 20] = 1
            watch = np.zeros((32, 32), bool)
            watch[8:16, 8:16] = watch[0:8, 16:24] = True   # the 64 pixels of each wave that walks
            q, m = f.weighted(e)
            ref = attrib_ref.attrib_f64(f.frame(), 32, 32, k, e, watch=watch)
            _compare(q, m, ref, 0)
            print(f"k {k} opacity {opacity} drawn {int((q > 0).sum())} zero {int((q == 0).sum())}")
            if opacity < 0.5 or k == 1:
                assert np.all(q > 0)
            else:
                saturated = np.nonzero(ref["front"] < T_MIN)[0]   # (index = depth order: 0 is nearest)
                assert saturated.size and saturated[0] + 8 < k
                assert np.all(q[:saturated[0]] > 0)
                assert not q[saturated[0] + 8:].any() and not m[saturated[0] + 8:].any()
        finally:
            f.close()
    finally:
        c.close()


# ---- 5. / 6. clamp, NaN, pitch; the zero plane --------------------------------------------------------------------------------
def test_clamp_nan_and_padded_pitch(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            w, h = VIEW
            rng = np.random.default_rng(3)
            plane = rng.uniform(-0.5, 1.5, size=(h, w)).astype(F)
            special = np.array([-1.0, 2.0, np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0], F)
            plane[rng.integers(0, h, 4000), rng.integers(0, w, 4000)] = special[rng.integers(0, special.size, 4000)]
            clamped = attrib_ref.clamp_plane(plane)
            assert np.isnan(plane).sum() > 100 and np.isinf(plane).sum() > 100 and not np.isnan(clamped).any()
            padded = np.full((h, w + 13), np.nan, F)          # rows of 333 floats: the padding is never read
            padded[:, :w] = plane
            want_q, want_m = f.weighted(clamped)
            assert (want_q > 0).sum() > 1000
            for name, p in (("raw", plane), ("padded", padded)):
                q, m = f.weighted(p)
                assert np.array_equal(q, want_q) and np.array_equal(_u32(m), _u32(want_m)), name
        finally:
            f.close()
    finally:
        c.close()


def test_all_zero_plane(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        acc = ws.Contrib(c, f.n)
        try:
            f.r.accumulate_weighted(f.pc, acc, np.zeros((VIEW[1], VIEW[0]), F))
            f.r.accumulate_weighted(f.pc, acc, np.ones((VIEW[1], VIEW[0]), F), scale=-1.0, bias=0.0)
            _, q, m = acc.download()
            assert acc.frames == 2 and not q.any() and not _u32(m).any()
            assert f.r.frame_stats()["overflow"] == 0
        finally:
            acc.close()
            f.close()
    finally:
        c.close()


# ---- 7. reproducible and mergeable --------------------------------------------------------------------------------------------
def _orbit_args(ws, gpc, index):
    cj = synth.orbit_cameras(5, VIEW[0], VIEW[1], float(VIEW[0]), float(VIEW[0]))[index]
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, cj.width, cj.height)
    cam.fit_near_far(gpc.aabb)
    return ws.SplattingArgs(camera=cam, viewport=VIEW, max_sh_deg=3)


def test_reproducible_and_mergeable(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=VIEW)
        pc = ws.PointCloud(c, sc.gpc)
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        a1, a2, ab, b_only = (ws.Contrib(c, n) for _ in range(4))
        try:
            r.enable_contrib(True)
            e = _ramp_checker(*VIEW)
            r.prepare(pc, _orbit_args(ws, sc.gpc, 0))
            for acc in (a1, a2, ab):
                r.accumulate_weighted(pc, acc, e)
            r.prepare(pc, _orbit_args(ws, sc.gpc, 2))
            for acc in (ab, b_only):
                r.accumulate_weighted(pc, acc, e)
            _, q1, m1 = a1.download()
            _, q2, m2 = a2.download()
            assert (q1 > 0).sum() > 1000
            assert np.array_equal(q1, q2) and np.array_equal(_u32(m1), _u32(m2))
            _, qab, mab = ab.download()
            _, qb, mb = b_only.download()
            assert ab.frames == 2 and not np.array_equal(qb, q1)
            a1.add(qb, mb)
            _, qsum, msum = a1.download()
            assert np.array_equal(qsum, qab) and np.array_equal(_u32(msum), _u32(mab))
            assert np.array_equal(qab, q1 + qb) and np.array_equal(mab, np.maximum(m1, mb))
        finally:
            for a in (a1, a2, ab, b_only):
                a.close()
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 8. the error plane -------------------------------------------------------------------------------------------------------
def _random_image(rng, dtype, h=29, w=37):
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img = rng.uniform(-0.2, 1.2, size=(h, w, 4)).astype(dtype)
    img[..., 3] = rng.uniform(0, 1, size=(h, w)).astype(dtype)
    return img


def _error_plane_ref(a, b, bg_a, bg_b, quantize, kind):
    x, qx = mr.pixel_value(a, bg_a, quantize)
    y, qy = mr.pixel_value(b, bg_b, quantize)
    d = (x - y).astype(F)
    e = (d * d).astype(F) if kind == "sq" else np.abs(d)
    return (((e[..., 0] + e[..., 1]).astype(F) + e[..., 2]).astype(F) / F(3.0)).astype(F), qx, qy


@pytest.mark.parametrize("quantize", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("over_bg", [False, True], ids=["stored", "over-bg"])
@pytest.mark.parametrize("formats", [(np.uint8, np.float32), (np.float16, np.float16)], ids=["rgba8-rgba32f", "rgba16f-rgba16f"])
def test_error_plane(ws, formats, over_bg, quantize):
    c = _ctx(ws)
    try:
        rng = np.random.default_rng(11)
        a, b = _random_image(rng, formats[0]), _random_image(rng, formats[1])
        bg_a, bg_b = ((0.25, 0.5, 0.75), (0.1, 0.0, 0.9)) if over_bg else (None, None)
        rec = ws.image_metrics(c, a, b, background_a=bg_a, background_b=bg_b, quantize_u8=quantize)
        rel = 2.0 ** -21  # three f32 roundings per pixel (two adds, one division) against the f64 sum of the f32 squares
        for kind in ("sq", "abs"):
            got = ws.image_error_plane(c, a, b, kind=kind, quantize_u8=quantize, background_a=bg_a, background_b=bg_b)
            want, qx, qy = _error_plane_ref(a, b, bg_a, bg_b, quantize, kind)
            assert got.shape == (29, 37) and got.dtype == F and got.max() > 0
            assert np.array_equal(_u32(got), _u32(want)), kind
            if kind == "sq":
                mean = float(got.astype(np.float64).mean())
                if quantize:
                    sse = round(float(got.astype(np.float64).sum()) * 3 * 255.0 ** 2)
                    print(f"sse_u8 {rec['sse_u8']} from the plane {sse}")
                    assert rec["sse_u8"] == mr.sse_u8(qx, qy) and abs(sse - rec["sse_u8"]) <= rel * rec["sse_u8"]
                else:
                    print(f"mse {rec['mse']:.9e} plane mean {mean:.9e} rel {abs(mean - rec['mse']) / rec['mse']:.2e}")
                    assert abs(mean - rec["mse"]) <= rel * rec["mse"]
    finally:
        c.close()


# ---- 9. / 10. the scene driver ------------------------------------------------------------------------------------------------
SMALL = (160, 120)


def _eval_renderer(ws, c, cloud, contrib):
    r = ws.GaussianRenderer(c, "rgba16float", cloud.sh_deg(), False)
    r.set_blend_mode("target")
    if contrib:
        r.enable_contrib(True)
    return r


def _eval_frame(ws, r, cloud, cam, size):
    """One frame as ws_render_views sets it up (ws_scene_evaluate's frames)."""
    pcam = cam.to_perspective().fit_near_far(cloud.bbox())
    r.prepare(cloud, ws.SplattingArgs(camera=pcam, viewport=size, max_sh_deg=cloud.sh_deg(), walltime=100.0))
    r.render(cloud)
    assert r.errors()[0] == 0
    return r.download_target()


def _manual(ws, c, pc, cams, kind, image_b, bg):
    """The loop of ws_scene_accumulate_error over the public Python calls; image_b(cam) is image b and its background."""
    n = pc.num_points()
    err, weight = ws.Contrib(c, n), ws.Contrib(c, n)
    r = _eval_renderer(ws, c, pc, True)
    try:
        for cam in cams:
            a = _eval_frame(ws, r, pc, cam, SMALL)
            b, bg_b = image_b(cam)
            if kind == "dssim":
                _, ssim = ws.image_metrics(c, a, b, background_a=bg, background_b=bg_b, ssim_map=True)
                r.accumulate_weighted(pc, err, ssim, scale=-0.5, bias=0.5)
            else:
                r.accumulate_weighted(pc, err, ws.image_error_plane(c, a, b, kind=kind, background_a=bg, background_b=bg_b))
            r.accumulate_contrib(pc, weight)
        return err.download()[1:], weight.download()[1:]
    finally:
        r.close()
        err.close()
        weight.close()


@pytest.fixture(scope="module")
def world(ws, oracle):
    c = _ctx(ws)
    sc = scenes.c1(ws, oracle, n=10_000, viewport=SMALL)
    parent = ws.PointCloud(c, sc.gpc)
    keep = np.nonzero(np.arange(parent.num_points()) % 3 != 2)[0].astype(np.uint32)   # every third Gaussian dropped
    sub = parent.subset(keep)
    cams = synth.orbit_cameras(3, SMALL[0], SMALL[1], 150.0, 150.0, radius=3.0, height_off=0.4)
    scene = ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams]))
    yield c, parent, sub, scene
    scene.close()
    sub.close()
    parent.close()
    c.close()


def _driver(ws, c, pc, scene, with_weight=True, **kw):
    n = pc.num_points()
    err, weight = ws.Contrib(c, n), ws.Contrib(c, n)
    try:
        frames = ws.accumulate_error_scene(c, pc, scene, None, err, weight if with_weight else None, **kw)
        assert frames == 3 and err.frames == 3 and weight.frames == (3 if with_weight else 0)
        return err.download()[1:], weight.download()[1:]
    finally:
        err.close()
        weight.close()


def _same(got, want):
    for (gq, gm), (wq, wm) in zip(got, want):
        assert np.array_equal(gq, wq) and np.array_equal(_u32(gm), _u32(wm))


@pytest.mark.parametrize("kind", ["sq", "dssim"])
def test_scene_driver_equals_the_manual_loop(ws, world, kind):
    c, parent, sub, scene = world
    bg = sub.background_color()
    bg = (0.0, 0.0, 0.0) if bg is None else bg
    cams = scene.cameras(None)
    rb = _eval_renderer(ws, c, parent, False)
    try:
        want = _manual(ws, c, sub, cams, kind, lambda cam: (_eval_frame(ws, rb, parent, cam, SMALL), bg), bg)
    finally:
        rb.close()
    got = _driver(ws, c, sub, scene, ref=parent, kind=kind)
    assert (got[0][0] > 0).sum() > 1000 and (got[1][0] > 0).sum() > 1000
    _same(got, want)
    # the error sums are the plain sums weighted by values in [0, 1]
    assert np.all(got[0][0] <= got[1][0]) and np.all(got[0][1] <= got[1][1])
    # without `weight` the error sums are the same
    assert np.array_equal(_driver(ws, c, sub, scene, with_weight=False, ref=parent, kind=kind)[0][0], got[0][0])


def test_scene_driver_against_ground_truth_pngs(ws, world, tmp_path):
    c, parent, sub, scene = world
    cams = scene.cameras(None)
    gt = tmp_path / "gt"
    gt.mkdir()
    truth = {}
    rb = _eval_renderer(ws, c, parent, False)
    try:
        for cam in cams:
            img = _eval_frame(ws, rb, parent, cam, SMALL)
            rgba8 = mr.pixel_value(np.concatenate([img[..., :3], np.ones_like(img[..., :1])], -1), quantize=True)[1]
            rgba8 = np.concatenate([rgba8, np.full(rgba8.shape[:2] + (1,), 255, np.uint8)], -1)
            ws.write_png(str(gt / (cam.img_name + ".png")), rgba8)
            truth[cam.img_name] = rgba8
    finally:
        rb.close()
    bg = sub.background_color()
    bg = (0.0, 0.0, 0.0) if bg is None else bg
    want = _manual(ws, c, sub, cams, "abs", lambda cam: (truth[cam.img_name], None), bg)
    got = _driver(ws, c, sub, scene, gt_dir=str(gt), kind="abs")
    assert (got[0][0] > 0).sum() > 1000
    _same(got, want)


def test_blame_finds_the_culprit(ws, oracle):
    """c1 seen from z = -6 fills the middle of a 160 x 120 frame (its silhouette ends near x = 109 px).  One large, opaque, white
    Gaussian is appended beside it and nearer to the cameras (centre near x = 116 px, sigma ~ 7 px): its core lies over the empty
    background, its fringe over the cube's edge.  Nothing is in front of it; what lies behind it sees only the fringe, where the
    frame is wrong by little."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=10_000, seed=0)
        floater = synth._rows(np.array([[0.9, 0.0, -3.0]], F), np.full((1, 3), 3.0, F), np.zeros((1, 45), F), np.array([8.0], F),
                              np.full((1, 3), np.log(0.18), F), np.array([[1.0, 0.0, 0.0, 0.0]], F))
        parent = ws.PointCloud(c, ws.GenericGaussianPointCloud.from_ply_rows(rows, 3))
        pc = ws.PointCloud(c, ws.GenericGaussianPointCloud.from_ply_rows(np.concatenate([rows, floater]), 3))
        cams = [synth.look_at_camera(i, [0.0, dy, -6.0], [0.0, 0.0, 0.0], SMALL[0], SMALL[1], 120.0, 120.0) for i, dy in enumerate((-0.5, 0.0, 0.5))]
        scene = ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams]))
        try:
            (eq, _), (wq, _) = _driver(ws, c, pc, scene, ref=parent, kind="sq")
            j = pc.num_points() - 1
            ratio = np.where(wq > 0, eq.astype(np.float64) / np.maximum(wq, 1).astype(np.float64), 0.0)
            others_e, others_r = np.delete(eq, j), np.delete(ratio, j)
            print(f"floater: err {eq[j] / 2.0 ** 32:.4f} weight {wq[j] / 2.0 ** 32:.4f} ratio {ratio[j]:.4f}; the others: largest err "
                  f"{others_e.max() / 2.0 ** 32:.4f}, largest ratio {others_r.max():.4f}, {int((others_e > 0).sum())} with a non-zero error sum")
            assert (others_e > 0).sum() > 10                       # it does cover something
            assert int(np.argmax(eq)) == j and eq[j] > others_e.max()
            assert int(np.argmax(ratio)) == j and ratio[j] > others_r.max()
        finally:
            scene.close()
            pc.close()
            parent.close()
    finally:
        c.close()


# ---- 11. errors ---------------------------------------------------------------------------------------------------------------
def test_error_cases(ws, world, tmp_path):
    c, parent, sub, scene = world
    n = sub.num_points()
    w, h = SMALL
    cam = scene.cameras(None)[0]
    args = ws.SplattingArgs(camera=cam.to_perspective().fit_near_far(sub.bbox()), viewport=SMALL, max_sh_deg=3)
    r = ws.GaussianRenderer(c, "rgba32float", 3, False)
    acc, small, of_parent = ws.Contrib(c, n), ws.Contrib(c, n - 1), ws.Contrib(c, parent.num_points())
    d_plane = c.malloc((w + 1) * h * 4 + 16)
    ones = np.ones((h, w), F)

    def code_of(fn):
        with pytest.raises(ws.WebSplatError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip()
        return e.value.code

    def raw(ptr, pitch, scale=1.0, bias=0.0):
        v = L.ws_plane_view()
        v.d_values, v.row_pitch_bytes, v.scale, v.bias = ptr, pitch, scale, bias
        return ws.lib.ws_renderer_accumulate_weighted(r.handle, sub.handle, acc.handle, C.byref(v), None)

    try:
        # not prepared; prepared without contributions
        r.enable_contrib(True)
        assert code_of(lambda: r.accumulate_weighted(sub, acc, ones)) == L.WS_ERR_STATE
        r.enable_contrib(False)
        r.prepare(sub, args)
        assert code_of(lambda: r.accumulate_weighted(sub, acc, ones)) == L.WS_ERR_STATE
        r.enable_contrib(True)
        r.prepare(sub, args)
        # prepared for another cloud; an accumulator of another size
        assert code_of(lambda: r.accumulate_weighted(parent, of_parent, ones)) == L.WS_ERR_STATE
        assert code_of(lambda: r.accumulate_weighted(sub, small, ones)) == L.WS_ERR_INVALID
        # pitch, alignment, scale and bias, null pointers
        assert raw(d_plane, w * 4) == L.WS_OK
        assert raw(d_plane, w * 4 + 4) == L.WS_OK
        assert raw(d_plane, w * 4 - 4) == L.WS_ERR_INVALID and b"pitch" in ws.lib.ws_last_error()
        assert raw(d_plane, w * 4 + 2) == L.WS_ERR_INVALID
        assert raw(d_plane + 2, w * 4) == L.WS_ERR_INVALID
        assert raw(None, w * 4) == L.WS_ERR_INVALID
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert raw(d_plane, w * 4, scale=bad) == L.WS_ERR_INVALID and raw(d_plane, w * 4, bias=bad) == L.WS_ERR_INVALID
        assert ws.lib.ws_renderer_accumulate_weighted(r.handle, sub.handle, acc.handle, None, None) == L.WS_ERR_INVALID
        assert acc.frames == 2
        # the error plane: kinds, flags, pitch
        img = np.zeros((4, 4, 4), F)
        assert code_of(lambda: ws.image_error_plane(c, img, img, kind="dssim")) == L.WS_ERR_INVALID
        va = ws.ImageView(d_plane, "rgba8unorm", 16).to_c()
        assert ws.lib.ws_image_error_plane(c.handle, C.byref(va), C.byref(va), 4, 4, 0, 0, C.c_void_p(d_plane), 12, None) == L.WS_ERR_INVALID
        assert ws.lib.ws_image_error_plane(c.handle, C.byref(va), C.byref(va), 4, 4, 0, 2, C.c_void_p(d_plane), 16, None) == L.WS_ERR_INVALID
        assert ws.lib.ws_image_error_plane(c.handle, C.byref(va), C.byref(va), 4, 4, 0, 0, None, 16, None) == L.WS_ERR_INVALID
        # the scene driver: both or neither of ref / gt_dir, an accumulator of another size, a missing PNG
        for kw in (dict(), dict(ref=parent, gt_dir=str(tmp_path))):
            assert code_of(lambda: ws.accumulate_error_scene(c, sub, scene, None, acc, **kw)) == L.WS_ERR_INVALID
        assert code_of(lambda: ws.accumulate_error_scene(c, sub, scene, None, small, ref=parent)) == L.WS_ERR_INVALID
        assert code_of(lambda: ws.accumulate_error_scene(c, sub, scene, None, acc, small, ref=parent)) == L.WS_ERR_INVALID
        with pytest.raises(ws.WebSplatError) as e:
            ws.accumulate_error_scene(c, sub, scene, None, acc, gt_dir=str(tmp_path))
        assert e.value.code == L.WS_ERR_IO and cam.img_name in str(e.value)
        assert acc.frames == 2
    finally:
        c.sync()
        c.free(d_plane)
        for a in (acc, small, of_parent):
            a.close()
        r.close()


# ---- 12. no pixel changes -----------------------------------------------------------------------------------------------------
def test_weighted_add_changes_no_pixel(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=VIEW)
        pc = ws.PointCloud(c, sc.gpc)
        plain, r = ws.GaussianRenderer(c, "rgba32float", 3, False), ws.GaussianRenderer(c, "rgba32float", 3, False)
        acc = ws.Contrib(c, pc.num_points())
        try:
            plain.prepare(pc, sc.args)
            plain.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            want = plain.download_target().copy()
            r.enable_contrib(True)
            r.prepare(pc, sc.args)
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            before = r.download_target().copy()
            r.accumulate_weighted(pc, acc, _ramp_checker(*VIEW))
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            after = r.download_target().copy()
            assert (want[..., 3] > 0.5).mean() > 0.05
            assert np.array_equal(_u32(want), _u32(before)) and np.array_equal(_u32(before), _u32(after))
            assert acc.frames == 1 and (acc.download()[1] > 0).sum() > 1000
        finally:
            acc.close()
            plain.close()
            r.close()
            pc.close()
    finally:
        c.close()
