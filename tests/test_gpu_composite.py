"""Compositing over an existing target behind an opaque depth buffer (include/websplat.h ws_renderer_render_composite).

  1. load over the clear colour is render(), bit for bit, over the FAST launch forms and the strict blend
  2. pixels no splat reaches keep their bytes (three formats)
  3. load against a float64 composite of the device's own frame over a random premultiplied target
  4. a constant-depth occluder equals the sub-cloud of Gaussians in front of it (FAST and strict)
  5. a spatially varying occluder (tilted plane + step edge) against the float64 reference
  6. trivial occluders: +inf / NDC 1.0 = no occluder; 0 leaves the target untouched and the planes 0
  7. the NDC kind equals the view-z kind for a plane converted by the header's expression
  8. the Dmax drop is exact
  9. the captured frame graph with depth and the occluder toggled between frames
 10. the error cases of the C ABI"""
import ctypes as C

import numpy as np
import pytest

import composite_ref
import scenes
from websplat import synth

pytestmark = pytest.mark.gpu

F32_BG = (0.125, 0.25, 0.375, 0.5)  # exact in f16; for unorm8 the backgrounds are k / 255 (the format's decode)
U8_K = (32, 64, 96, 128)


def _ctx(ws, **cfg):
    return ws.Context(0, ws.config_from_env({}, **cfg))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _background(fmt):
    if fmt == "rgba8unorm":
        return tuple(float(np.float32(k) / np.float32(255.0)) for k in U8_K)
    return F32_BG


def _fill(fmt, w, h, bg):
    """An image of the target's dtype whose decode is `bg` everywhere."""
    if fmt == "rgba8unorm":
        return np.broadcast_to(np.array(U8_K, dtype=np.uint8), (h, w, 4)).copy()
    dt = np.float16 if fmt == "rgba16float" else np.float32
    return np.broadcast_to(np.array(bg, dtype=dt), (h, w, 4)).copy()


def _random_target(fmt, w, h, seed):
    """A random premultiplied target (colour <= alpha) of the target's dtype, and its f32 decode."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (h, w, 1))
    img = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)) * a, a], axis=2)
    if fmt == "rgba8unorm":
        enc = np.rint(img * 255.0).astype(np.uint8)
        return enc, enc.astype(np.float32) / np.float32(255.0)
    dt = np.float16 if fmt == "rgba16float" else np.float32
    enc = img.astype(dt)
    return enc, enc.astype(np.float32)


def _c1(ws, oracle, n=10_000, viewport=(320, 240), seed=0):
    return scenes.c1(ws, oracle, n=n, viewport=viewport, seed=seed)


# ---- 1. load over the clear colour is render() ------------------------------------------------------------------------------
LOAD_CASES = [
    ("rgba32float", {}),
    ("rgba16float", {}),
    ("rgba8unorm", {}),
    ("rgba32float", {"tile_qw": 2, "tile_qh": 2}),
    ("rgba8unorm", {"tile_qw": 4, "tile_qh": 2}),
    ("rgba32float", {"blend_split": 1}),
    ("rgba16float", {"blend_split": 0}),
    ("rgba32float", {"bin_request": 2}),
    ("rgba32float", {"blend_order": 1, "blend_split": 0}),
]


def _load_equals_render(ws, c, pc, args, fmt, compressed=False, sh_deg=3, mode="fast", occluder=None):
    w, h = args.viewport
    bg = _background(fmt)
    r = ws.GaussianRenderer(c, fmt, sh_deg, compressed)
    try:
        r.set_blend_mode(mode)
        if occluder is not None:
            r.enable_depth(True)
        r.prepare(pc, args)
        r.render(pc, background=bg)
        want = r.download_target().copy()
        r.upload_target(_fill(fmt, w, h, bg))
        r.render_composite(pc, load=True, occluder=occluder, background=(0.9, 0.9, 0.9, 0.9))  # (ignored under load)
        got = r.download_target().copy()
        assert r.frame_stats()["overflow"] == 0
    finally:
        r.close()
    assert np.array_equal(_bits(want), _bits(got))
    assert not np.array_equal(_bits(want), _bits(_fill(fmt, w, h, bg)))  # the frame draws something


@pytest.mark.parametrize("fmt,cfg", LOAD_CASES, ids=[f"{f}-{'-'.join(f'{k}{v}' for k, v in c.items()) or 'default'}" for f, c in LOAD_CASES])
def test_load_over_clear_is_render(ws, oracle, fmt, cfg):
    c = _ctx(ws, **cfg)
    try:
        sc = _c1(ws, oracle, n=20_000, viewport=(480, 352))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _load_equals_render(ws, c, pc, sc.args, fmt)
        finally:
            pc.close()
    finally:
        c.close()


@pytest.mark.parametrize("fmt", ["rgba32float", "rgba16float", "rgba8unorm"])
def test_load_over_clear_is_render_strict(ws, oracle, fmt):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=8_000, viewport=(256, 192))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _load_equals_render(ws, c, pc, sc.args, fmt, mode="target")
        finally:
            pc.close()
    finally:
        c.close()


def test_load_over_clear_is_render_at_4k(ws, oracle):
    """3840x2160: several tiles per workgroup (the MULTI forms); also with a +inf occluder (the OCCLUDE | LOAD form)."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c2(n=200_000, seed=1)
        cj = synth.orbit_cameras(4, 3840, 2160, 3840.0, 3840.0)[0]
        sc = scenes.Scene(ws, oracle, rows, 3, cj, (3840, 2160))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _load_equals_render(ws, c, pc, sc.args, "rgba16float")
            _load_equals_render(ws, c, pc, sc.args, "rgba32float", occluder=np.full((2160, 3840), np.inf, dtype=np.float32))
        finally:
            pc.close()
    finally:
        c.close()


def test_load_over_clear_is_render_compressed(ws):
    from test_gpu_aux import _compressed  # (the compressed scene builder; the f64 reference is composite_ref)
    c = _ctx(ws)
    try:
        gpc, _, args = _compressed(ws)
        pc = ws.PointCloud(c, gpc)
        try:
            _load_equals_render(ws, c, pc, args, "rgba32float", compressed=True)
        finally:
            pc.close()
    finally:
        c.close()


# ---- 2. untouched pixels keep their bytes ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba32float", "rgba16float", "rgba8unorm"])
def test_untouched_pixels_keep_their_bytes(ws, oracle, fmt):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=3_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, fmt, 3, False)
        try:
            r.prepare(pc, sc.args)
            enc, _ = _random_target(fmt, 320, 240, seed=5)
            r.upload_target(enc)
            r.render_composite(pc, load=True, alpha=True)
            got = r.download_target().copy()
            alpha = r.download_aux()["alpha"]
        finally:
            r.close()
            pc.close()
        clear = alpha == 0
        assert 0.05 < clear.mean() < 0.95
        assert np.array_equal(_bits(got[clear]), _bits(enc[clear]))
        assert not np.array_equal(_bits(got[~clear]), _bits(enc[~clear]))
    finally:
        c.close()


# ---- 3. load against float64 -------------------------------------------------------------------------------------------
def _device_frame(ws, c, pc, args, fmt="rgba32float"):
    """(renderer, frame, z) of a prepared frame with its z plane; the caller closes the renderer."""
    r = ws.GaussianRenderer(c, fmt, 3, False)
    r.enable_depth(True)
    r.prepare(pc, args)
    return r, r.download_frame(), r.download_depths()


def _check_f64(got, alpha, ref, T, undecided, w, h):
    bad = (np.abs(got.astype(np.float64) - ref) > 2e-4).any(axis=2)
    bad |= np.abs(alpha.astype(np.float64) - (1.0 - T)) > 2e-4
    allowed = max(4, int(scenes.BOUNDARY_PIXEL_FRACTION * w * h))
    n_bad = int(bad.sum())
    assert n_bad <= allowed, f"{n_bad} pixels outside the tolerances (allowed cut-off boundary pixels: {allowed})"
    assert undecided[bad].all(), "a pixel outside the tolerances is not a cut-off boundary pixel"


@pytest.mark.parametrize("seed", [0, 7])
def test_load_against_f64(ws, oracle, seed):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(320, 240), seed=seed)
        pc = ws.PointCloud(c, sc.gpc)
        r, frame, z = _device_frame(ws, c, pc, sc.args)
        try:
            enc, dst = _random_target("rgba32float", 320, 240, seed=seed + 100)
            r.upload_target(enc)
            r.render_composite(pc, load=True, alpha=True)
            got = r.download_target().copy()
            alpha = r.download_aux()["alpha"]
        finally:
            r.close()
            pc.close()
        ref, T, undecided = composite_ref.composite_f64(frame, z, 320, 240, dst=dst)
        _check_f64(got, alpha, ref, T, undecided, 320, 240)
        assert ((1.0 - T) > 0.5).mean() > 0.02
    finally:
        c.close()


# ---- 4. a constant-depth occluder equals the sub-cloud in front of it ------------------------------------------------------
def _z_per_gaussian(ws, c, pc, args, n):
    r = ws.GaussianRenderer(c, "rgba32float", 3, False)
    try:
        r.enable_capture(True)
        r.prepare(pc, args)
        src = r.download_frame(with_src_index=True)["src_index"]
        r.enable_capture(False)
        r.enable_depth(True)
        r.prepare(pc, args)
        z = r.download_depths()
    finally:
        r.close()
    zg = np.full(n, np.nan, dtype=np.float32)
    zg[src] = z
    return zg


def _subcloud_case(ws, oracle, c, rows, sh_deg, args, mode, quantile, min_unsaturated):
    """d0 at `quantile` of the frame's splat depths; FAST: bit-identical in the 8x8 blocks that did not saturate (at least
    `min_unsaturated` of the image), within the early-out bound in the others."""
    w, h = args.viewport
    full = ws.GenericGaussianPointCloud.from_ply_rows(rows, sh_deg)
    pc = ws.PointCloud(c, full)
    try:
        zg = _z_per_gaussian(ws, c, pc, args, len(rows))
        zs = np.unique(zg[np.isfinite(zg)])
        i = int(len(zs) * quantile)
        d0 = np.float32((np.float64(zs[i]) + np.float64(zs[i + 1])) / 2)
        assert zs[i] < d0 < zs[i + 1]
        r = ws.GaussianRenderer(c, "rgba32float", sh_deg, False)
        try:
            r.set_blend_mode(mode)
            r.enable_depth(True)
            r.prepare(pc, args)
            planes = mode == "fast"
            r.render_composite(pc, load=False, occluder=np.full((h, w), d0, dtype=np.float32), depth=planes,
                               median_depth=planes, alpha=planes, background=(0.1, 0.2, 0.3, 0.4))
            got, got_planes = r.download_target().copy(), r.download_aux()
        finally:
            r.close()
    finally:
        pc.close()
    sub = ws.GenericGaussianPointCloud.from_ply_rows(np.ascontiguousarray(rows[np.isfinite(zg) & (zg < d0)]), sh_deg)
    spc = ws.PointCloud(c, sub)
    r = ws.GaussianRenderer(c, "rgba32float", sh_deg, False)
    try:
        r.set_blend_mode(mode)
        r.enable_depth(True)
        r.prepare(spc, args)
        if mode == "fast":
            r.render_aux(spc, depth=True, median_depth=True, alpha=True, background=(0.1, 0.2, 0.3, 0.4))
        else:
            r.render(spc, background=(0.1, 0.2, 0.3, 0.4))
        want, want_planes = r.download_target().copy(), (r.download_aux() if mode == "fast" else {})
    finally:
        r.close()
        spc.close()
    if mode != "fast":
        assert np.array_equal(_bits(got), _bits(want))
        return
    # (an 8x8 block whose every pixel saturated may end its walk at a different point of a list of different make-up: there
    # the two may differ by contributions below the early-out bound)
    sat = composite_ref.saturated_quadrants(want_planes["alpha"]) | composite_ref.saturated_quadrants(got_planes["alpha"])
    assert 1.0 - sat.mean() >= min_unsaturated
    assert np.array_equal(_bits(got[~sat]), _bits(want[~sat]))
    for k in ("depth", "median_depth", "alpha"):
        assert np.array_equal(got_planes[k][~sat].view(np.uint32), want_planes[k][~sat].view(np.uint32)), k
    assert np.abs(got[sat] - want[sat]).max(initial=0.0) <= 4 * 2.0 ** -14
    assert (want_planes["alpha"] > 0).mean() > 0.05


@pytest.mark.parametrize("mode", ["fast", "target"])
def test_constant_occluder_is_the_subcloud_c1(ws, oracle, mode):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(320, 240))
        rows = synth.scene_c1(n=10_000, seed=0, sh_deg=3)
        _subcloud_case(ws, oracle, c, rows, 3, sc.args, mode, 0.3, 0.5)
    finally:
        c.close()


@pytest.mark.parametrize("mode", ["fast", "target"])
def test_constant_occluder_is_the_subcloud_hd1m_crop(ws, oracle, mode):
    c = _ctx(ws)
    try:
        rows = synth.scene_c2(n=1_000_000, seed=1)
        cj = synth.orbit_cameras(64, 256, 192, 1920.0, 1920.0)[0]
        sc = scenes.Scene(ws, oracle, rows, 3, cj, (256, 192))
        _subcloud_case(ws, oracle, c, rows, 3, sc.args, mode, 0.02, 0.0)
    finally:
        c.close()


# ---- 5. a spatially varying occluder against float64 ------------------------------------------------------------------------
def test_varying_occluder_against_f64(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        r, frame, z = _device_frame(ws, c, pc, sc.args)
        try:
            lo, hi = np.percentile(z, [10, 90])
            yy, xx = np.mgrid[0:240, 0:320]
            occ = (lo + (hi - lo) * (xx / 319.0) * 0.7 + (hi - lo) * 0.3 * (yy / 239.0)).astype(np.float32)  # tilted plane
            occ[:, 200:] = np.float32(np.percentile(z, 50))  # a step edge
            enc, dst = _random_target("rgba32float", 320, 240, seed=3)
            r.upload_target(enc)
            r.render_composite(pc, load=True, occluder=occ, alpha=True)
            got = r.download_target().copy()
            alpha = r.download_aux()["alpha"]
            r.upload_target(enc)
            r.render_composite(pc, load=True, alpha=True)
            no_occ = r.download_aux()["alpha"]
        finally:
            r.close()
            pc.close()
        ref, T, undecided = composite_ref.composite_f64(frame, z, 320, 240, dst=dst, occluder=occ)
        _check_f64(got, alpha, ref, T, undecided, 320, 240)
        assert (alpha < no_occ - 0.05).mean() > 0.05  # the occluder removes something
        assert (alpha > 0.2).mean() > 0.02  # and leaves something
    finally:
        c.close()


# ---- 6. trivial occluders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba32float", "rgba8unorm"])
def test_trivial_occluders(ws, oracle, fmt):
    c = _ctx(ws)
    w, h = 320, 240
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(w, h))
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, fmt, 3, False)
        try:
            r.enable_depth(True)
            r.prepare(pc, sc.args)
            enc, _ = _random_target(fmt, w, h, seed=9)

            def run(**kw):
                r.upload_target(enc)
                r.render_composite(pc, load=True, depth=True, median_depth=True, alpha=True, **kw)
                return r.download_target().copy(), r.download_aux()

            base, base_planes = run()
            for kw in ({"occluder": np.full((h, w), np.inf, dtype=np.float32)},
                       {"occluder": np.ones((h, w), dtype=np.float32), "occluder_kind": "ndc"}):
                img, planes = run(**kw)
                assert np.array_equal(_bits(img), _bits(base)), kw
                for k in planes:
                    assert np.array_equal(planes[k].view(np.uint32), base_planes[k].view(np.uint32)), (kw, k)
            img, planes = run(occluder=np.zeros((h, w), dtype=np.float32))
            assert np.array_equal(_bits(img), _bits(enc))
            for k in planes:
                assert np.array_equal(planes[k], np.zeros((h, w), dtype=np.float32)), k
            assert (base_planes["alpha"] > 0).mean() > 0.05
        finally:
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 7. NDC = view z ------------------------------------------------------------------------------------------------------
def _near_far(args):
    proj = np.asarray(args.camera.uniform(args.viewport).proj, dtype=np.float32)
    n = np.float32(-proj[3 * 4 + 2] / proj[2 * 4 + 2])
    f = np.float32(-proj[3 * 4 + 2] / (proj[2 * 4 + 2] - np.float32(1.0)))
    return n, f


def test_ndc_equals_view_z(ws, oracle):
    c = _ctx(ws)
    w, h = 320, 240
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(w, h))
        pc = ws.PointCloud(c, sc.gpc)
        r, frame, z = _device_frame(ws, c, pc, sc.args)
        try:
            n, f = _near_far(sc.args)
            assert 0 < n < f
            # D: midpoints of the gaps between consecutive splat depths that are at least 2e-4 relative wide (so every D lies
            # 1e-4 relative away from every splat z), laid out in blocks of 20 x 20 pixels
            zs = np.unique(z.astype(np.float64))
            mid = (zs[1:] + zs[:-1]) / 2
            cand = mid[(zs[1:] - zs[:-1]) / mid >= 2e-4]
            cand = cand[(cand > np.percentile(zs, 3)) & (cand < np.percentile(zs, 97))]
            assert len(cand) >= 8
            cand = cand[np.linspace(0, len(cand) - 1, 24).astype(int)]
            yy, xx = np.mgrid[0:h, 0:w]
            D = cand[(xx // 20 + 7 * (yy // 20)) % len(cand)]
            k = np.clip(np.searchsorted(zs, D), 1, len(zs) - 1)
            assert (np.minimum(np.abs(D - zs[k - 1]), np.abs(zs[k] - D)) / D >= 1e-4 * 0.999).all()
            D32 = D.astype(np.float32)
            # the NDC plane from the header's expression, inverted: d = (f - n f / D) / (f - n)
            nf, fmn = np.float64(n) * np.float64(f), np.float64(f) - np.float64(n)
            d = ((np.float64(f) - nf / D) / fmn).astype(np.float32)
            assert ((d > 0) & (d < 1)).all()
            out = []
            for occ, kind in ((D32, "view_z"), (d, "ndc")):
                r.render_composite(pc, load=False, occluder=occ, occluder_kind=kind, depth=True, alpha=True)
                out.append((r.download_target().copy(), r.download_aux()))
        finally:
            r.close()
            pc.close()
        (a, ap), (b, bp) = out
        assert np.array_equal(_bits(a), _bits(b))
        for k in ap:
            assert np.array_equal(ap[k].view(np.uint32), bp[k].view(np.uint32)), k
        assert (ap["alpha"] > 0).mean() > 0.05
    finally:
        c.close()


# ---- 8. the Dmax drop is exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [32, 16])
def test_dmax_drop_is_exact(ws, oracle, tile):
    """Whole tiles behind a near occluder (every record dropped at staging) against the same tiles with one pixel per tile at
    +inf (nothing dropped: every pair fails the per-pair test instead).  tile = 16 runs the 2x2 shape."""
    cfg = {} if tile == 32 else {"tile_qw": 2, "tile_qh": 2}
    c = _ctx(ws, blend_split=0, **cfg)
    w, h = 320, 256
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(w, h))
        pc = ws.PointCloud(c, sc.gpc)
        r, frame, z = _device_frame(ws, c, pc, sc.args)
        try:
            zmin, zmed = float(z.min()), float(np.median(z))
            ty, tx = np.mgrid[0:h, 0:w] // tile
            occ = np.where((tx + ty) % 2 == 0, np.float32(0.5 * zmin), np.float32(zmed)).astype(np.float32)  # hidden / half
            occ[:, : 2 * tile] = np.inf
            alt = occ.copy()
            altered = np.zeros((h, w), dtype=bool)
            altered[tile // 2::tile, tile // 2::tile] = True
            alt[altered] = np.inf
            enc, _ = _random_target("rgba32float", w, h, seed=4)
            out = []
            for o in (occ, alt):
                r.upload_target(enc)
                r.render_composite(pc, load=True, occluder=o, depth=True, median_depth=True, alpha=True)
                out.append((r.download_target().copy(), r.download_aux()))
        finally:
            r.close()
            pc.close()
        (a, ap), (b, bp) = out
        hidden = ((tx + ty) % 2 == 0) & (tx >= 2)
        keep = ~altered & hidden
        assert np.array_equal(_bits(a[keep]), _bits(b[keep]))
        assert np.array_equal(_bits(a[keep]), _bits(enc[keep]))  # nothing in front of the near occluder
        for k in ap:
            assert np.array_equal(ap[k][keep].view(np.uint32), bp[k][keep].view(np.uint32)), k
        # the altered pixels did change where splats reach them
        assert not np.array_equal(_bits(a[altered & hidden]), _bits(b[altered & hidden]))
    finally:
        c.close()


# ---- 9. the captured frame graph ------------------------------------------------------------------------------------------
def test_frame_graph_with_depth_and_occluder_toggled(ws, oracle):
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    cg, cn = _ctx(ws, use_graph=1), _ctx(ws, use_graph=0)
    w, h = 320, 240
    try:
        sc = _c1(ws, oracle, n=20_000, viewport=(w, h))
        cams = synth.orbit_cameras(6, w, h, 320.0, 320.0, radius=3.0, height_off=0.4)
        views = []
        for cj in cams:
            cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
            cam.fit_near_far(sc.gpc.aabb)
            views.append(ws.SplattingArgs(camera=cam, viewport=(w, h), max_sh_deg=3))
        enc, _ = _random_target("rgba32float", w, h, seed=2)
        yy, xx = np.mgrid[0:h, 0:w]
        occ = (0.96 + 0.5 * xx / w).astype(np.float32) * np.float32(3.0)
        pg, pn = ws.PointCloud(cg, sc.gpc), ws.PointCloud(cn, sc.gpc)
        rg, rn = ws.GaussianRenderer(cg, "rgba32float", 3, False), ws.GaussianRenderer(cn, "rgba32float", 3, False)
        try:
            for i, args in enumerate(views):
                on = i % 3 != 1  # depth (and the occluder) on, off, on, on, off, on
                out = []
                for r, pc, s in ((rg, pg, stream.value), (rn, pn, None)):
                    r.enable_depth(on)
                    r.prepare(pc, args, stream=s)
                    r.upload_target(enc, stream=s)
                    r.render_composite(pc, load=True, occluder=occ if on else None, alpha=True, stream=s)
                    (cg if r is rg else cn).sync(s)
                    out.append((r.download_target().copy(), r.download_aux()))
                (ig, ag), (i_n, an) = out
                assert np.array_equal(_bits(ig), _bits(i_n)), i
                assert np.array_equal(ag["alpha"], an["alpha"]), i
        finally:
            rg.close()
            rn.close()
            pg.close()
            pn.close()
    finally:
        cg.close()
        cn.close()
        hip.hipStreamDestroy(stream)


# ---- 10. errors -------------------------------------------------------------------------------------------------------------
def test_errors(ws, oracle):
    from websplat import _lib as L
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=5000, viewport=(160, 120))
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        w, h = 160, 120
        out = c.malloc(w * h * 16)
        occ = c.malloc(w * h * 4 + 64)
        pl = c.malloc(w * h * 4 + 64)
        try:
            def call(aux=None, **fields):
                d = L.ws_composite_desc()
                for k, v in fields.items():
                    if k == "reserved":
                        d.reserved[1] = v
                    else:
                        setattr(d, k, v)
                return ws.lib.ws_renderer_render_composite(r.handle, pc.handle, None, C.c_void_p(out), w * 16,
                                                           C.byref(aux) if aux is not None else None, C.byref(d), None)

            r.prepare(pc, sc.args)  # depth off
            assert call(occluder=occ, occluder_pitch=w * 4) == L.WS_ERR_STATE
            assert call(load=1, occluder=occ, occluder_pitch=w * 4) == L.WS_ERR_STATE
            assert call(load=1) == L.WS_OK  # load needs no z plane
            assert call() == L.WS_OK  # nothing asked for: render_aux
            assert ws.lib.ws_renderer_render_composite(r.handle, pc.handle, None, C.c_void_p(out), w * 16, None, None, None) == L.WS_OK
            r.enable_depth(True)
            r.prepare(pc, sc.args)
            assert call(occluder=occ, occluder_pitch=w * 4) == L.WS_OK
            # pitch / alignment / reserved / kind / load
            assert call(occluder=occ, occluder_pitch=w * 4 - 4) == L.WS_ERR_INVALID
            assert call(occluder=occ, occluder_pitch=w * 4 + 2) == L.WS_ERR_INVALID
            assert call(occluder=occ + 2, occluder_pitch=w * 4) == L.WS_ERR_INVALID
            assert call(load=1, reserved=1) == L.WS_ERR_INVALID
            assert call(reserved=1) == L.WS_ERR_INVALID
            assert call(load=1, occluder_kind=2) == L.WS_ERR_INVALID
            assert call(load=2) == L.WS_ERR_INVALID
            # the planes keep render_aux's checks
            t = L.ws_aux_targets()
            t.depth, t.depth_pitch = pl, w * 4 - 4
            assert call(aux=t, load=1) == L.WS_ERR_INVALID
            t.depth_pitch = w * 4
            assert call(aux=t, load=1, occluder=occ, occluder_pitch=w * 4) == L.WS_OK
            # the blend modes
            r.set_blend_mode("fast_exact_cut")
            assert call(load=1) == L.WS_ERR_UNSUPPORTED
            assert call(occluder=occ, occluder_pitch=w * 4) == L.WS_ERR_UNSUPPORTED
            assert call() == L.WS_OK  # nothing asked for: render() in that mode
            r.set_blend_mode("target")
            assert call(load=1, occluder=occ, occluder_pitch=w * 4) == L.WS_OK
            assert call(aux=t, load=1) == L.WS_ERR_UNSUPPORTED  # planes need WS_BLEND_FAST
            r.set_blend_mode("fast")
            r.enable_blend_timing(True)
            assert call(load=1) == L.WS_ERR_UNSUPPORTED
            r.enable_blend_timing(False)
            r.enable_capture(True)
            r.prepare(pc, sc.args)
            assert call(load=1) == L.WS_ERR_UNSUPPORTED
            assert call(occluder=occ, occluder_pitch=w * 4) == L.WS_ERR_UNSUPPORTED
            r.enable_capture(False)
            c.sync()
        finally:
            c.free(out)
            c.free(occ)
            c.free(pl)
            r.close()
            pc.close()
    finally:
        c.close()
