"""Pruned point clouds (include/websplat.h ws_pointcloud_create_subset, contrib.hip k_pc_gather): the subset is the parent's
records gathered in order with the parent's metadata; dropping the Gaussians that never drew (max_weight == 0) leaves an
unsaturated frame bit-identical and a saturated one within the early-termination remainder."""
import ctypes as C

import numpy as np
import pytest

import scenes
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu


def _ctx(ws, **cfg):
    return ws.Context(0, ws.config_from_env({}, **cfg))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _random_ascending(n, keep, seed):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(np.arange(1, n - 1), size=keep - 2, replace=False))
    return np.concatenate([[0], idx, [n - 1]]).astype(np.uint32)


def _meta(pc):
    b = pc.bbox()
    return (pc.sh_deg(), pc.compressed(), list(b.min), list(b.max), pc.center(), pc.up(), pc.mip_splatting(),
            pc.dilation_kernel_size(), pc.background_color())


def _compressed_gpc(ws, n, seed=41):
    blobs = synth.compressed_blobs(n=n, n_geometry=1024, n_sh=777, seed=seed, sh_deg=3)
    q = ws.ws_gaussian_quantization()
    for name in ("color_dc", "color_rest", "opacity", "scaling_factor"):
        zp, s = blobs["quant"][name]
        getattr(q, name).zero_point = int(zp)
        getattr(q, name).scale = float(s)
    g = blobs["gaussians"]
    aabb, center, up = ws.pointcloud_stats(g, 24, ws.Aabb([-1, -1, -1], [1, 1, 1]))
    return ws.GenericGaussianPointCloud(g, blobs["sh"], blobs["sh_deg"], blobs["num_points"], aabb, center, compressed=True,
                                        covars=blobs["covars"], quantization=q, up=up, kernel_size=0.25, mip_splatting=True,
                                        background_color=[0.25, 0.5, 0.75])


@pytest.mark.parametrize("compressed", [False, True], ids=["uncompressed", "compressed"])
def test_subset_is_the_parent_indexed(ws, compressed):
    n = 5000
    c = _ctx(ws)
    try:
        if compressed:
            gpc = _compressed_gpc(ws, n)
            cj = synth.look_at_camera(0, [0.0, 0.0, -3.0], [0, 0, 0], 256, 192, 256.0, 256.0)
        else:
            gpc = ws.GenericGaussianPointCloud.from_ply_rows(synth.scene_c1(n=n, seed=5), 3, kernel_size=0.2, mip_splatting=False,
                                                             background_color=[0.1, 0.2, 0.3])
            cj = synth.camera_c1(256, 192)
        parent = ws.PointCloud(c, gpc)
        idx = _random_ascending(n, 1777, seed=9)
        g_par, s_par = parent.download()
        meta = _meta(parent)
        sub = parent.subset(idx)
        parent.close()  # the subset owns its memory
        try:
            assert sub.num_points() == len(idx)
            assert _meta(sub) == meta
            g_sub, s_sub = sub.download()
            assert np.array_equal(g_sub, g_par[idx])
            if compressed:
                assert s_sub is None
            else:
                assert np.array_equal(s_sub, s_par[idx])
            # and it renders: the same view of a cloud made of the same records from scratch gives the same bytes
            # (compressed: the codebooks and the quantisation block were copied whole)
            cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 256, 192)
            cam.fit_near_far(gpc.aabb)
            args = ws.SplattingArgs(camera=cam, viewport=(256, 192), max_sh_deg=3)
            if compressed:
                fresh_gpc = ws.GenericGaussianPointCloud(gpc.gaussians[idx], gpc.sh_coefs, gpc.sh_deg, len(idx), gpc.aabb, gpc.center,
                                                         compressed=True, covars=gpc.covars, quantization=gpc.quantization, up=gpc.up,
                                                         kernel_size=0.25, mip_splatting=True, background_color=[0.25, 0.5, 0.75])
            else:
                fresh_gpc = ws.GenericGaussianPointCloud(gpc.gaussians[idx], gpc.sh_coefs[idx], gpc.sh_deg, len(idx), gpc.aabb, gpc.center,
                                                         up=gpc.up, kernel_size=0.2, mip_splatting=False, background_color=[0.1, 0.2, 0.3])
            fresh = ws.PointCloud(c, fresh_gpc)
            r = ws.GaussianRenderer(c, "rgba32float", 3, compressed)
            try:
                r.prepare(sub, args)
                r.render(sub)
                a = r.download_target().copy()
                r.prepare(fresh, args)
                r.render(fresh)
                b = r.download_target().copy()
                assert (a[..., 3] > 0).mean() > 0.05
                assert np.array_equal(_bits(a), _bits(b))
            finally:
                r.close()
                fresh.close()
        finally:
            sub.close()
    finally:
        c.close()


def _rows_at(xyz, scale, opacity_logit, colour=0.5):
    """PLY rows (synth layout, sh_deg 0: xyz, normal, f_dc, opacity, scale, rot) for isotropic Gaussians."""
    n = len(xyz)
    rows = np.zeros((n, 3 + 3 + 3 + 1 + 3 + 4), dtype=np.float32)
    rows[:, 0:3] = xyz
    rows[:, 6:9] = colour
    rows[:, 9] = opacity_logit
    rows[:, 10:13] = np.log(scale)[:, None]
    rows[:, 13] = 1.0
    return rows


def _unsaturated_scene(ws):
    """Three sparse layers of faint isotropic Gaussians in front of a camera at z = -4, a block behind the camera and a block
    of sub-pixel ones."""
    rng = np.random.default_rng(11)
    parts = []
    for z, colour in ((-0.5, 0.3), (0.0, 0.6), (0.5, 0.9)):
        m = 1500
        xyz = np.stack([rng.uniform(-1.7, 1.7, m), rng.uniform(-1.3, 1.3, m), np.full(m, z)], 1).astype(np.float32)
        parts.append(_rows_at(xyz, np.full(m, 0.04, dtype=np.float32), -2.0, colour))
    m = 700
    behind = np.stack([rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, m), rng.uniform(-7.0, -5.0, m)], 1).astype(np.float32)
    parts.append(_rows_at(behind, np.full(m, 0.05, dtype=np.float32), 2.0, 0.8))
    tiny = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1.0, 1.0, m), rng.uniform(-0.2, 0.2, m)], 1).astype(np.float32)
    parts.append(_rows_at(tiny, np.full(m, 1e-5, dtype=np.float32), -2.0, 0.4))
    rows = np.concatenate(parts)
    rows = rows[rng.permutation(len(rows))]
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 0)
    cj = synth.look_at_camera(0, [0.0, 0.0, -4.0], [0, 0, 0], 256, 192, 300.0, 300.0)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 256, 192)
    cam.fit_near_far(gpc.aabb)
    return gpc, ws.SplattingArgs(camera=cam, viewport=(256, 192), max_sh_deg=0), rows


def _image(ws, c, pc, args, fmt, sh_deg, background=(0.1, 0.2, 0.3, 0.4)):
    r = ws.GaussianRenderer(c, fmt, sh_deg, False)
    try:
        r.prepare(pc, args)
        r.render(pc, background=background)
        return r.download_target().copy()
    finally:
        r.close()


def _score(ws, c, pc, args, sh_deg):
    """(max_weight per Gaussian, the frame's coverage plane, largest colour channel of the frame's Splat records)."""
    r = ws.GaussianRenderer(c, "rgba32float", sh_deg, False)
    acc = ws.Contrib(c, pc.num_points())
    try:
        r.enable_contrib(True)
        r.prepare(pc, args)
        r.accumulate_contrib(pc, acc)
        r.render_aux(pc, depth=False, median_depth=False, alpha=True)
        alpha = r.download_aux()["alpha"]
        rec = np.ascontiguousarray(r.download_frame()["splats"]).view(np.float16).reshape(-1, 10)
        return acc.download()[2], alpha, float(rec[:, 6:9].astype(np.float32).max())
    finally:
        acc.close()
        r.close()


def test_pruning_an_unsaturated_frame_is_bit_identical(ws):
    c = _ctx(ws)
    try:
        gpc, args, rows = _unsaturated_scene(ws)
        pc = ws.PointCloud(c, gpc)
        try:
            mw, alpha, _ = _score(ws, c, pc, args, 0)
            assert float(alpha.max()) < 1.0 - 2.0 ** -13  # the precondition: no pixel saturates, no quadrant stops early
            assert (alpha > 0).mean() > 0.5
            keep = np.nonzero(mw > 0)[0].astype(np.uint32)
            assert 3000 < len(keep) < pc.num_points()
            assert not mw[rows[:, 2] < -4.5].any()  # the block behind the camera never drew
            sub = pc.subset(keep)
            try:
                for fmt in ("rgba32float", "rgba8unorm"):
                    a = _image(ws, c, pc, args, fmt, 0)
                    b = _image(ws, c, sub, args, fmt, 0)
                    assert np.array_equal(_bits(a), _bits(b)), fmt
            finally:
                sub.close()
        finally:
            pc.close()
    finally:
        c.close()


def test_pruning_a_saturated_frame_stays_within_the_termination_remainder(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            mw, alpha, max_colour = _score(ws, c, pc, sc.args, 3)
            keep = np.nonzero(mw > 0)[0].astype(np.uint32)
            assert 1000 < len(keep) < pc.num_points()
            sub = pc.subset(keep)
            try:
                a = _image(ws, c, pc, sc.args, "rgba32float", 3, background=(0, 0, 0, 0))
                b = _image(ws, c, sub, sc.args, "rgba32float", 3, background=(0, 0, 0, 0))
                d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
                bound = 2.0 ** -13 * max(1.0, max_colour)
                print(f"kept {len(keep)} of {pc.num_points()}; max |d| {d:.3e} bound {bound:.3e} saturated pixels "
                      f"{int((alpha >= 1 - 2.0 ** -14).sum())}")
                assert d <= bound
            finally:
                sub.close()
        finally:
            pc.close()
    finally:
        c.close()


def test_subset_index_validation(ws):
    c = _ctx(ws)
    try:
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(synth.scene_c1(n=1000, seed=2), 3)
        pc = ws.PointCloud(c, gpc)
        try:
            def code_of(indices):
                with pytest.raises(ws.WebSplatError) as e:
                    pc.subset(np.asarray(indices, dtype=np.uint32)).close()
                assert "ws_pointcloud_create_subset" in str(e.value)
                return e.value.code

            assert code_of([]) == L.WS_ERR_INVALID                 # n = 0
            assert code_of([3, 2]) == L.WS_ERR_INVALID             # descending
            assert code_of([2, 2]) == L.WS_ERR_INVALID             # not strictly ascending
            assert code_of([0, 999, 1000]) == L.WS_ERR_INVALID     # not below num_points
            h = C.c_void_p()
            assert ws.lib.ws_pointcloud_create_subset(c.handle, pc.handle, None, 1, C.byref(h)) == L.WS_ERR_INVALID
            whole = pc.subset(np.arange(1000, dtype=np.uint32))
            try:
                assert whole.num_points() == 1000
                assert np.array_equal(whole.download()[0], pc.download()[0])
            finally:
                whole.close()
        finally:
            pc.close()
    finally:
        c.close()
