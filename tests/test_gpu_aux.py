"""Auxiliary planes (include/websplat.h ws_renderer_render_aux): per-pixel expected depth, median depth and coverage beside the
colour image, from K1's per-splat z plane (ws_renderer_enable_depth) and k_blend's AUX forms.

  1. the colour image is bit-identical to render()'s over every FAST launch form (formats, tile shapes, split halves, binning
     shift, longest-first order, several tiles per workgroup at 4K, compressed scenes); depth off again = a renderer that never had it
  2. the z plane equals numpy's f32 (view @ [x, y, z, 1]).z of the source Gaussians (store slot -> Gaussian by capture's src_index)
  3. the planes against a float64 front-to-back composite of the device's own frame (its splats, draw order and z plane)
  4. oracle-free properties: one fronto-parallel plane of centres, an opaque near layer over a far one, alpha = A on a clear background
  5. the captured frame graph with depth toggled between frames
  6. the error cases of the C ABI"""
import ctypes as C

import numpy as np
import pytest

import scenes
from websplat import synth

pytestmark = pytest.mark.gpu

PLANES = ("depth", "median_depth", "alpha")


def _ctx(ws, **cfg):
    return ws.Context(0, ws.config_from_env({}, **cfg))


def _render_pair(ws, c, pc, args, fmt="rgba32float", compressed=False, sh_deg=3, background=(0.1, 0.2, 0.3, 0.4)):
    """(colour of render(), colour of render_aux() with all planes, the planes) on one renderer and one prepared frame."""
    r = ws.GaussianRenderer(c, fmt, sh_deg, compressed)
    try:
        r.enable_depth(True)
        r.prepare(pc, args)
        r.render(pc, background=background)
        plain = r.download_target().copy()
        r.render_aux(pc, depth=True, median_depth=True, alpha=True, background=background)
        with_aux = r.download_target().copy()
        planes = r.download_aux()
        assert r.frame_stats()["overflow"] == 0
        return plain, with_aux, planes
    finally:
        r.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _c1(ws, oracle, n=10_000, viewport=(320, 240), seed=0):
    return scenes.c1(ws, oracle, n=n, viewport=viewport, seed=seed)


# ---- 1. the colour image is untouched ------------------------------------------------------------------------------------
COLOUR_CASES = [
    # (format, config overrides)
    ("rgba32float", {}),
    ("rgba16float", {}),
    ("rgba8unorm", {}),
    ("rgba32float", {"tile_qw": 2, "tile_qh": 2}),
    ("rgba32float", {"tile_qw": 4, "tile_qh": 2}),
    ("rgba16float", {"tile_qw": 2, "tile_qh": 2}),
    ("rgba32float", {"blend_split": 1}),
    ("rgba32float", {"blend_split": 0}),
    ("rgba32float", {"bin_request": 0}),
    ("rgba32float", {"bin_request": 2}),
    ("rgba32float", {"bin_request": 1}),
    ("rgba32float", {"blend_order": 1, "blend_split": 0}),
    ("rgba32float", {"blend_order": 0, "blend_split": 0}),
]


@pytest.mark.parametrize("fmt,cfg", COLOUR_CASES, ids=[f"{f}-{'-'.join(f'{k}{v}' for k, v in c.items()) or 'default'}" for f, c in COLOUR_CASES])
def test_colour_is_bit_identical(ws, oracle, fmt, cfg):
    c = _ctx(ws, **cfg)
    try:
        sc = _c1(ws, oracle, n=20_000, viewport=(480, 352))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            plain, with_aux, planes = _render_pair(ws, c, pc, sc.args, fmt)
            assert np.array_equal(_bits(plain), _bits(with_aux))
            assert set(planes) == set(PLANES)
            assert (planes["alpha"] > 0).mean() > 0.05
            for p in planes.values():
                assert np.isfinite(p).all()
        finally:
            pc.close()
    finally:
        c.close()


def test_colour_is_bit_identical_at_4k(ws, oracle):
    """3840x2160: several tiles per workgroup (the MULTI form)."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c2(n=200_000, seed=1)
        cj = synth.orbit_cameras(4, 3840, 2160, 3840.0, 3840.0)[0]
        sc = scenes.Scene(ws, oracle, rows, 3, cj, (3840, 2160))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            plain, with_aux, planes = _render_pair(ws, c, pc, sc.args)
            assert np.array_equal(_bits(plain), _bits(with_aux))
            assert (planes["alpha"] > 0).mean() > 0.05
        finally:
            pc.close()
    finally:
        c.close()


def _compressed(ws, n=50_000, seed=41):
    blobs = synth.compressed_blobs(n=n, n_geometry=1024, n_sh=777, seed=seed, sh_deg=3)
    q = ws.ws_gaussian_quantization()
    for name in ("color_dc", "color_rest", "opacity", "scaling_factor"):
        zp, s = blobs["quant"][name]
        getattr(q, name).zero_point = int(zp)
        getattr(q, name).scale = float(s)
    g = blobs["gaussians"]
    aabb, center, up = ws.pointcloud_stats(g, 24, ws.Aabb([-1, -1, -1], [1, 1, 1]))
    gpc = ws.GenericGaussianPointCloud(g, blobs["sh"], blobs["sh_deg"], blobs["num_points"], aabb, center,
                                       compressed=True, covars=blobs["covars"], quantization=q, up=up)
    cj = synth.look_at_camera(0, [0.0, 0.0, -3.0], [0, 0, 0], 400, 300, 400.0, 400.0)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 400, 300)
    cam.fit_near_far(gpc.aabb)
    return gpc, blobs, ws.SplattingArgs(camera=cam, viewport=(400, 300), max_sh_deg=3)


def test_colour_is_bit_identical_compressed(ws):
    c = _ctx(ws)
    try:
        gpc, _, args = _compressed(ws)
        pc = ws.PointCloud(c, gpc)
        try:
            plain, with_aux, planes = _render_pair(ws, c, pc, args, compressed=True)
            assert np.array_equal(_bits(plain), _bits(with_aux))
            assert (planes["alpha"] > 0).mean() > 0.05
        finally:
            pc.close()
    finally:
        c.close()


def test_depth_off_again_is_a_plain_renderer(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle)
        pc = ws.PointCloud(c, sc.gpc)
        ra, rb = ws.GaussianRenderer(c, "rgba32float", 3, False), ws.GaussianRenderer(c, "rgba32float", 3, False)
        try:
            ra.enable_depth(True)
            ra.prepare(pc, sc.args)
            ra.render_aux(pc, depth=True, median_depth=True, alpha=True)
            ra.enable_depth(False)
            ra.prepare(pc, sc.args)
            ra.render(pc, background=(0.2, 0.1, 0.0, 1.0))
            a = ra.download_target().copy()
            rb.prepare(pc, sc.args)
            rb.render(pc, background=(0.2, 0.1, 0.0, 1.0))
            b = rb.download_target().copy()
            assert np.array_equal(_bits(a), _bits(b))
            with pytest.raises(ws.WebSplatError):
                ra.download_depths()
        finally:
            ra.close()
            rb.close()
            pc.close()
    finally:
        c.close()


# ---- 2. the z plane ----------------------------------------------------------------------------------------------------
def _numpy_z(view16, xyz):
    """f32 (view @ [x, y, z, 1]).z, view[c * 4 + r] column-major as the uniform holds it; and 2 ulp of the largest product."""
    v = np.asarray(view16, dtype=np.float32)
    xyz = np.asarray(xyz, dtype=np.float32)
    terms = np.stack([v[0 * 4 + 2] * xyz[:, 0], v[1 * 4 + 2] * xyz[:, 1], v[2 * 4 + 2] * xyz[:, 2],
                      np.full(len(xyz), v[3 * 4 + 2], dtype=np.float32)], 1)
    z = ((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]
    big = np.abs(terms).max(axis=1)
    return z, 2.0 * np.spacing(big)


def _z_check(ws, c, pc, args, xyz, compressed):
    r = ws.GaussianRenderer(c, "rgba32float", 3, compressed)
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
    assert len(z) == len(src) > 1000
    want, tol = _numpy_z(list(args.camera.uniform(args.viewport).view), xyz[src])
    assert np.all(np.abs(z.astype(np.float64) - want.astype(np.float64)) <= tol), np.abs(z - want).max()
    assert (z > 0).all()  # in front of the camera


def test_z_plane_uncompressed(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=30_000)
        pc = ws.PointCloud(c, sc.gpc)
        try:
            g = np.ascontiguousarray(np.asarray(sc.gpc.gaussians, dtype=np.uint8).reshape(sc.gpc.num_points, 28)[:, :12])
            xyz = g.view(np.float32).reshape(-1, 3)  # the 28-B Gaussian record starts with xyz (f32 x 3)
            _z_check(ws, c, pc, sc.args, xyz, False)
        finally:
            pc.close()
    finally:
        c.close()


def test_z_plane_compressed(ws):
    c = _ctx(ws)
    try:
        gpc, blobs, args = _compressed(ws)
        pc = ws.PointCloud(c, gpc)
        try:
            g = np.ascontiguousarray(blobs["gaussians"]).view(np.uint8).reshape(gpc.num_points, 24)[:, :12]
            _z_check(ws, c, pc, args, np.ascontiguousarray(g).view(np.float32).reshape(-1, 3), True)  # GaussianCompressed: xyz f32 x 3 first
        finally:
            pc.close()
    finally:
        c.close()


# ---- 3. against a float64 composite of the device's own frame ----------------------------------------------------------
T_MIN = 1.0 / 16384.0


def _f64_reference(frame, z, width, height):
    """Front-to-back composite in float64 over the device's splats (gaussian.wgsl:40-66 decode and cut-off, as
    scenes.BoundaryProof), no early termination.  Returns alpha, depth, median, the T at the median's crossing, and
    a mask of pixels that have a fragment within f32 rounding of the cut-off."""
    order = frame["sorted"].astype(np.int64)[::-1]  # near -> far
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
    T = np.ones((height, width))
    wz = np.zeros((height, width))
    ws_ = np.zeros((height, width))
    med = np.zeros((height, width))
    tcross = np.full((height, width), np.inf)
    undecided = np.zeros((height, width), dtype=bool)
    e = 2.0 ** -24
    rad = np.sqrt(scenes.CUT_A) * 1.001
    for s in order:
        m00, m01, m10, m11 = h[s, 0] * W, h[s, 2] * W, -h[s, 1] * H, -h[s, 3] * H
        det = m00 * m11 - m01 * m10
        if not np.isfinite(det) or det == 0:
            continue
        i00, i01, i10, i11 = m11 / det, -m01 / det, -m10 / det, m00 / det
        cx, cy = (h[s, 4] * 0.5 + 0.5) * W, (0.5 - h[s, 5] * 0.5) * H
        ex, ey = rad * np.hypot(m00, m01) + 2, rad * np.hypot(m10, m11) + 2
        x0, x1 = max(int(np.floor(cx - ex)), 0), min(int(np.ceil(cx + ex)), width - 1)
        y0, y1 = max(int(np.floor(cy - ey)), 0), min(int(np.ceil(cy + ey)), height - 1)
        if x0 > x1 or y0 > y1:
            continue
        xs = np.arange(x0, x1 + 1) + 0.5 - cx
        ys = np.arange(y0, y1 + 1)[:, None] + 0.5 - cy
        t00, t01, t10, t11 = i00 * xs, i01 * ys, i10 * xs, i11 * ys
        p0, p1 = t00 + t01, t10 + t11
        a = p0 * p0 + p1 * p1
        e0 = 6 * e * (np.abs(t00) + np.abs(t01)) + 4 * e * 64.0 * (abs(i00) + abs(i01))
        e1 = 6 * e * (np.abs(t10) + np.abs(t11)) + 4 * e * 64.0 * (abs(i10) + abs(i11))
        tol = 4.0 * (2 * np.abs(p0) * e0 + 2 * np.abs(p1) * e1 + 2 * e * a) + 1e-7
        undecided[y0:y1 + 1, x0:x1 + 1] |= np.abs(a - scenes.CUT_A) <= tol
        keep = a <= scenes.CUT_A
        b = np.where(keep, np.minimum(0.99, np.exp(-a) * h[s, 9]), 0.0)
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        w = b * Tb
        Ta = Tb - w
        cross = keep & (Tb > 0.5) & (Ta <= 0.5)
        med[y0:y1 + 1, x0:x1 + 1] = np.where(cross, z[s], med[y0:y1 + 1, x0:x1 + 1])
        tcross[y0:y1 + 1, x0:x1 + 1] = np.where(cross, np.minimum(np.abs(Tb - 0.5), np.abs(Ta - 0.5)), tcross[y0:y1 + 1, x0:x1 + 1])
        wz[y0:y1 + 1, x0:x1 + 1] += w * float(z[s])
        ws_[y0:y1 + 1, x0:x1 + 1] += w
        T[y0:y1 + 1, x0:x1 + 1] = Ta
    depth = np.where(ws_ > 0, wz / np.where(ws_ > 0, ws_, 1.0), 0.0)
    return 1.0 - T, depth, med, tcross, undecided


def _check_against_f64(ws, c, pc, args):
    w, h = args.viewport
    r = ws.GaussianRenderer(c, "rgba32float", 3, False)
    try:
        r.enable_depth(True)
        r.prepare(pc, args)
        r.render_aux(pc, depth=True, median_depth=True, alpha=True)
        got = r.download_aux()
        frame = r.download_frame()
        z = r.download_depths()
    finally:
        r.close()
    alpha, depth, med, tcross, undecided = _f64_reference(frame, z, w, h)
    zfar = float(np.abs(z).max())
    bad = np.abs(got["alpha"] - alpha) > 2e-4
    bad |= np.abs(got["depth"] - depth) > 1e-4 * zfar
    # the median is exact (the same f32 z), except where T at the crossing lies within 1e-4 of 0.5
    near_half = tcross < 1e-4
    bad |= (got["median_depth"] != med.astype(np.float32)) & ~near_half
    allowed = max(4, int(scenes.BOUNDARY_PIXEL_FRACTION * w * h))
    n_bad = int(bad.sum())
    assert n_bad <= allowed, f"{n_bad} pixels outside the tolerances (allowed cut-off boundary pixels: {allowed})"
    assert undecided[bad].all(), "a pixel outside the tolerances is not a cut-off boundary pixel"
    assert (alpha > 0.5).mean() > 0.02  # the frame draws something


@pytest.mark.parametrize("seed", [0, 7])
def test_planes_against_f64_c1(ws, oracle, seed):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=10_000, viewport=(320, 240), seed=seed)
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _check_against_f64(ws, c, pc, sc.args)
        finally:
            pc.close()
    finally:
        c.close()


def test_planes_against_f64_hd1m_crop(ws, oracle):
    """The hd1m scene (1 M Gaussians) through the hd1m camera's focal length, a 256x192 crop of its centre."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c2(n=1_000_000, seed=1)
        cj = synth.orbit_cameras(64, 256, 192, 1920.0, 1920.0)[0]
        sc = scenes.Scene(ws, oracle, rows, 3, cj, (256, 192))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _check_against_f64(ws, c, pc, sc.args)
        finally:
            pc.close()
    finally:
        c.close()


# ---- 4. oracle-free properties ----------------------------------------------------------------------------------------
def _rows_at(xyz, scale, opacity_logit, sh_deg=0, colour=0.5):
    """PLY rows (synth layout: xyz, normal, f_dc, f_rest, opacity, scale, rot) for isotropic Gaussians."""
    n = len(xyz)
    ncoef = (sh_deg + 1) ** 2
    rows = np.zeros((n, 3 + 3 + 3 * ncoef + 1 + 3 + 4), dtype=np.float32)
    rows[:, 0:3] = xyz
    rows[:, 6:9] = colour
    o = 6 + 3 * ncoef
    rows[:, o] = opacity_logit
    rows[:, o + 1:o + 4] = np.log(scale)[:, None] if np.ndim(scale) else np.log(scale)
    rows[:, o + 4] = 1.0
    return rows


def _plane_scene(ws, rows, viewport=(256, 192)):
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 0)
    cj = synth.look_at_camera(0, [0.0, 0.0, -4.0], [0, 0, 0], viewport[0], viewport[1], 300.0, 300.0)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, viewport[0], viewport[1])
    cam.fit_near_far(gpc.aabb)
    return gpc, ws.SplattingArgs(camera=cam, viewport=viewport, max_sh_deg=0)


def _aux_of(ws, c, gpc, args, background=(0.0, 0.0, 0.0, 0.0), fmt="rgba32float"):
    pc = ws.PointCloud(c, gpc)
    r = ws.GaussianRenderer(c, fmt, 0, False)
    try:
        r.enable_depth(True)
        r.prepare(pc, args)
        r.render_aux(pc, depth=True, median_depth=True, alpha=True, background=background)
        return r.download_aux(), r.download_target().copy(), r.download_depths()
    finally:
        r.close()
        pc.close()


def test_one_fronto_parallel_plane(ws):
    rng = np.random.default_rng(3)
    n = 4000
    xyz = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.1, 1.1, n), np.zeros(n)], 1).astype(np.float32)
    rows = _rows_at(xyz, np.full(n, 0.03, dtype=np.float32), 0.5)
    c = _ctx(ws)
    try:
        gpc, args = _plane_scene(ws, rows)
        planes, _, z = _aux_of(ws, c, gpc, args)
        z0 = float(np.median(z))
        assert np.abs(z - z0).max() <= 1e-6 * z0  # every centre at the same view depth
        cov = planes["alpha"] > 0
        assert cov.mean() > 0.3
        assert np.all(np.abs(planes["depth"][cov] - z0) <= 1e-5 * z0)
        opaque = planes["alpha"] >= 0.5 + 1e-3
        assert opaque.mean() > 0.1
        assert np.all(np.abs(planes["median_depth"][opaque] - z0) <= 1e-5 * z0)
        assert np.all(planes["depth"][~cov] == 0) and np.all(planes["median_depth"][planes["alpha"] < 0.5] == 0)
    finally:
        c.close()


def test_opaque_near_layer_over_far_layer(ws):
    """Near layer: dense opaque splats over the left half of the view at z = -1; far layer over the whole view at z = +1."""
    rng = np.random.default_rng(5)
    nn, nf = 6000, 6000
    near = np.stack([rng.uniform(-1.6, -0.1, nn), rng.uniform(-1.2, 1.2, nn), np.full(nn, -1.0)], 1)
    far = np.stack([rng.uniform(-2.4, 2.4, nf), rng.uniform(-1.8, 1.8, nf), np.full(nf, 1.0)], 1)
    rows = np.concatenate([_rows_at(near.astype(np.float32), np.full(nn, 0.05, dtype=np.float32), 8.0),
                           _rows_at(far.astype(np.float32), np.full(nf, 0.06, dtype=np.float32), 8.0)])
    c = _ctx(ws)
    try:
        gpc, args = _plane_scene(ws, rows)
        planes, _, z = _aux_of(ws, c, gpc, args)
        zn, zf = float(z.min()), float(z.max())
        assert zf - zn > 1.5
        # the near layer covers where its median is the near z
        near_px = np.abs(planes["median_depth"] - zn) <= 1e-5 * zf
        assert near_px.mean() > 0.2
        # where the near layer covers opaquely (its own coverage alone is ~1), the median is the near layer's depth ...
        w = args.viewport[0]
        left = np.zeros_like(near_px)
        left[:, : int(w * 0.3)] = True
        solid = left & (planes["alpha"] > 0.999)
        assert solid.mean() > 0.1
        assert np.all(np.abs(planes["median_depth"][solid] - zn) <= 1e-5 * zf)
        # ... and where only the far layer reaches (right side), depth is the far layer's z
        right = np.zeros_like(near_px)
        right[:, int(w * 0.75):] = True
        only_far = right & (planes["alpha"] > 0)
        assert only_far.mean() > 0.1
        assert np.all(np.abs(planes["depth"][only_far] - zf) <= 1e-5 * zf)
    finally:
        c.close()


def test_alpha_equals_a_channel_on_a_clear_background(ws, oracle):
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle)
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        try:
            r.prepare(pc, sc.args)  # (depth off: alpha needs no z plane)
            r.render_aux(pc, depth=False, alpha=True, background=(0.0, 0.0, 0.0, 0.0))
            a = r.download_aux()["alpha"]
            img = r.download_target()
            assert np.abs(a - img[..., 3]).max() <= 1e-6
            assert (a > 0).mean() > 0.05
            # with another clear colour the coverage stays what it is
            r.render_aux(pc, depth=False, alpha=True, background=(0.3, 0.3, 0.3, 1.0))
            assert np.array_equal(r.download_aux()["alpha"], a)
        finally:
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 5. the captured frame graph -------------------------------------------------------------------------------------
def test_frame_graph_with_depth_toggled(ws, oracle):
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    cg, cn = _ctx(ws, use_graph=1), _ctx(ws, use_graph=0)
    try:
        sc = _c1(ws, oracle, n=20_000, viewport=(320, 240))
        cams = synth.orbit_cameras(6, 320, 240, 320.0, 320.0, radius=3.0, height_off=0.4)
        views = []
        for cj in cams:
            cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 320, 240)
            cam.fit_near_far(sc.gpc.aabb)
            views.append(ws.SplattingArgs(camera=cam, viewport=(320, 240), max_sh_deg=3))
        pg, pn = ws.PointCloud(cg, sc.gpc), ws.PointCloud(cn, sc.gpc)
        rg, rn = ws.GaussianRenderer(cg, "rgba32float", 3, False), ws.GaussianRenderer(cn, "rgba32float", 3, False)
        try:
            for i, args in enumerate(views):
                on = i % 3 != 1  # on, off, on, on, off, on
                out = []
                for r, pc, s in ((rg, pg, stream.value), (rn, pn, None)):
                    r.enable_depth(on)
                    r.prepare(pc, args, stream=s)
                    r.render_aux(pc, depth=on, median_depth=on, alpha=True, stream=s)
                    (cg if r is rg else cn).sync(s)
                    out.append((r.download_target().copy(), r.download_aux()))
                (ig, ag), (i_n, an) = out
                assert np.array_equal(_bits(ig), _bits(i_n)), i
                assert set(ag) == set(an)
                for k in ag:
                    assert np.array_equal(ag[k], an[k]), (i, k)
        finally:
            rg.close()
            rn.close()
            pg.close()
            pn.close()
    finally:
        cg.close()
        cn.close()
        hip.hipStreamDestroy(stream)


# ---- 6. errors -------------------------------------------------------------------------------------------------------
def test_errors(ws, oracle):
    from websplat import _lib as L
    c = _ctx(ws)
    try:
        sc = _c1(ws, oracle, n=5000, viewport=(160, 120))
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        w, h = 160, 120
        out = c.malloc(w * h * 16)
        pl = c.malloc(w * h * 4 + 64)
        try:
            def call(background=None, **fields):
                t = L.ws_aux_targets()
                for k, v in fields.items():
                    if k == "reserved":
                        t.reserved[0] = v
                    else:
                        setattr(t, k, v)
                return ws.lib.ws_renderer_render_aux(r.handle, pc.handle, None, C.c_void_p(out), w * 16, C.byref(t), None)

            r.prepare(pc, sc.args)  # depth off
            # depth / median without a z plane
            assert call(depth=pl, depth_pitch=w * 4) == L.WS_ERR_STATE
            assert call(median_depth=pl, median_depth_pitch=w * 4) == L.WS_ERR_STATE
            nv = C.c_uint32()
            assert ws.lib.ws_renderer_download_depths(r.handle, 0, None, C.byref(nv)) == L.WS_ERR_STATE
            # alpha alone needs none
            assert call(alpha=pl, alpha_pitch=w * 4) == L.WS_OK
            # aux == NULL and all-NULL targets are render()
            assert ws.lib.ws_renderer_render_aux(r.handle, pc.handle, None, C.c_void_p(out), w * 16, None, None) == L.WS_OK
            assert call() == L.WS_OK
            r.enable_depth(True)
            r.prepare(pc, sc.args)
            assert call(depth=pl, depth_pitch=w * 4) == L.WS_OK
            # pitch / alignment / reserved
            assert call(depth=pl, depth_pitch=w * 4 - 4) == L.WS_ERR_INVALID
            assert call(median_depth=pl, median_depth_pitch=w * 4 + 2) == L.WS_ERR_INVALID
            assert call(alpha=pl + 2, alpha_pitch=w * 4) == L.WS_ERR_INVALID
            assert call(alpha=pl, alpha_pitch=w * 4, reserved=1) == L.WS_ERR_INVALID
            # the other blend modes
            for mode in ("target", "fast_exact_cut"):
                r.set_blend_mode(mode)
                assert call(alpha=pl, alpha_pitch=w * 4) == L.WS_ERR_UNSUPPORTED
                assert call(depth=pl, depth_pitch=w * 4) == L.WS_ERR_UNSUPPORTED
                assert call() == L.WS_OK  # no plane: render() in that mode
            r.set_blend_mode("fast")
            assert call(depth=pl, depth_pitch=w * 4, median_depth=pl, median_depth_pitch=w * 4, alpha=pl, alpha_pitch=w * 4) == L.WS_OK
            c.sync()
        finally:
            c.free(out)
            c.free(pl)
            r.close()
            pc.close()
    finally:
        c.close()
