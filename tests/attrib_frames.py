"""The frames of test_gpu_contrib, test_gpu_attrib, test_gpu_values and test_gpu_removal: a context, one prepared frame with contributions on, and
the scenes the three files share (the stack of the staging boundaries, c1, the compressed cloud, the ramp-checker plane)."""
import numpy as np

import blend_ref
import scenes
from websplat import synth

F = np.float32
VIEW = (320, 240)  # 7.5 tile rows of 32 px: the last row's lower lanes are outside the viewport
BG = (0.25, 0.5, 0.75)  # the background of the removal effect


def _ctx(ws, **cfg):
    return ws.Context(0, ws.config_from_env({}, **cfg))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Frame:
    """One prepared frame with contributions on; accumulators come and go."""

    def __init__(self, ws, c, gpc, args, compressed=False, fmt="rgba32float"):
        self.ws, self.c = ws, c
        self.pc = ws.PointCloud(c, gpc)
        self.r = ws.GaussianRenderer(c, fmt, 3, compressed)
        self.r.enable_contrib(True)
        self.r.prepare(self.pc, args)
        self.n = self.pc.num_points()
        self.view = (int(args.viewport[0]), int(args.viewport[1]))

    def _download(self, accumulate):
        acc = self.ws.Contrib(self.c, self.n)
        try:
            accumulate(acc)
            assert acc.frames == 1
            _, q, m = acc.download()
            return q, m
        finally:
            acc.close()

    def plain(self):
        return self._download(lambda acc: self.r.accumulate_contrib(self.pc, acc))

    def weighted(self, plane, scale=1.0, bias=0.0):
        return self._download(lambda acc: self.r.accumulate_weighted(self.pc, acc, plane, scale=scale, bias=bias))

    def removal(self, background=BG, kind="sq", scale=1.0, weight=None, base=False, **kw):
        got = self._download(lambda acc: self.r.accumulate_removal(self.pc, acc, background=background, kind=kind, scale=scale,
                                                                    weight=weight, base=base, **kw))
        return got + (self.r.download_removal_base(),) if base else got

    def values(self, f, winner=False):
        """H x W x C float32 (None without values) and, with winner, H x W uint32."""
        self.r.render_values(self.pc, f, winner=winner)
        got = self.r.download_values()
        assert ("values" in got) == (f is not None) and ("winner" in got) == bool(winner)
        return (got.get("values"), got["winner"]) if winner else got["values"]

    def frame(self):
        assert self.r.frame_stats()["overflow"] == 0
        return self.r.download_frame(with_src_index=True)

    def close(self):
        self.r.close()
        self.pc.close()


def _stack(k, opacity):
    """k isotropic Gaussians on the optical axis at distinct depths, index 0 nearest, each covering the whole 32 x 32 viewport
    (sigma ~ 12 px: the cut-off ellipse reaches 26 px from the centre, the corners are 22.6 px away), so every tile lists all k and
    every quadrant's wave walks all of them -- until it saturates.  `opacity`: one value or one per Gaussian."""
    z = np.linspace(-0.25, 0.25, k, dtype=np.float32) if k > 1 else np.zeros(1, dtype=np.float32)
    xyz = np.stack([np.zeros(k, np.float32), np.zeros(k, np.float32), z], axis=1)
    rng = np.random.default_rng(k)
    f_dc = rng.uniform(-1.0, 1.0, size=(k, 3)).astype(np.float32)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (k, 1))
    log_scale = np.full((k, 3), np.log(12.0 * 3.0 / 320.0), np.float32)
    op = np.broadcast_to(np.asarray(opacity, np.float64), (k,))
    logit = np.log(op / (1.0 - op)).astype(np.float32)
    return synth._rows(xyz, f_dc, np.zeros((k, 45), np.float32), logit, log_scale, rot)


def _stack_frame(ws, c, k, opacity, viewport=(32, 32)):
    return _Frame(ws, c, *blend_ref.device_scene(ws, _stack(k, opacity), viewport))


def _cloud_rows(n=3000, seed=17):
    """The general cloud of test_gpu_removal, test_gpu_gradient and the geometry tests: anisotropic Gaussians of random rotation
    and random colours in the unit cube, scales 0.01 - 0.08, opacities 0.02 - 0.3."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(F)
    log_scale = rng.uniform(np.log(0.01), np.log(0.08), size=(n, 3)).astype(F)
    rot = rng.standard_normal(size=(n, 4)).astype(F)
    op = rng.uniform(0.02, 0.3, size=n)
    f_dc = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(F)
    return synth._rows(xyz, f_dc, np.zeros((n, 45), F), np.log(op / (1.0 - op)).astype(F), log_scale, rot)


def _c1_frame(ws, oracle, c, seed=0, viewport=VIEW):
    sc = scenes.c1(ws, oracle, n=10_000, viewport=viewport, seed=seed)
    return _Frame(ws, c, sc.gpc, sc.args)


def _compressed(ws, n=50_000, seed=41):
    """The compressed cloud and view of test_gpu_aux._compressed."""
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
    return gpc, ws.SplattingArgs(camera=cam, viewport=(400, 300), max_sh_deg=3)


def _ramp_checker(width, height, cell=5):
    """A smooth ramp (exact zeros at the left, exact ones at the right) times a checker of 5-px cells."""
    x = np.arange(width, dtype=np.float64)[None, :] / (width - 1)
    y = np.arange(height, dtype=np.float64)[:, None] / (height - 1)
    ramp = np.clip(1.5 * x + 0.2 * np.sin(6.0 * y) - 0.2, 0.0, 1.0)
    checker = ((np.arange(width)[None, :] // cell + np.arange(height)[:, None] // cell) % 2).astype(np.float64)
    e = (ramp * checker).astype(F)
    assert (e == 0).any() and (e == 1).any() and ((e > 0) & (e < 1)).any()
    return e
