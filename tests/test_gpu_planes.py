"""The renderer-owned planes of the Python binding (target, aux, value, base and occluder planes) across viewport changes:
each must be the new viewport's, in shape and in content, whatever the renderer held before."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

N = 2000
VIEWPORTS = [(64, 48), (48, 64), (96, 48)]  # the same byte count under another shape, then another pitch at the same height


def _frame(ws, ctx, r, pc, sc, values):
    """Every call that makes or reuses a renderer-owned plane, once, on sc's viewport; what the downloads give."""
    w, h = sc.viewport
    out = {}
    r.prepare(pc, sc.args)
    r.render(pc)
    out["target"] = r.download_target()
    r.render_aux(pc, depth=True, median_depth=True, alpha=True)
    out.update({"aux_" + k: v for k, v in r.download_aux().items()})
    r.render_values(pc, values=values, winner=True)
    out.update(r.download_values())
    contrib = ws.Contrib(ctx, N)
    try:
        r.accumulate_removal(pc, contrib, base=True)
        out["base"] = r.download_removal_base()
        _, out["contrib_q32"], out["contrib_max"] = contrib.download()
    finally:
        contrib.close()
    r.render_composite(pc, occluder=np.full((h, w), np.inf, dtype=np.float32))
    out["composite"] = r.download_target()
    return out


def _renderer(ws, ctx):
    r = ws.GaussianRenderer(ctx, "rgba32float", 3, False)
    r.enable_depth()
    r.enable_contrib()
    return r


def test_planes_follow_the_viewport(ws, ctx, oracle):
    scs = [scenes.c1(ws, oracle, n=N, viewport=vp, seed=5) for vp in VIEWPORTS]
    pc = ws.PointCloud(ctx, scs[0].gpc)
    values = np.linspace(0.0, 1.0, N, dtype=np.float32)
    r = _renderer(ws, ctx)
    try:
        for sc in scs:
            w, h = sc.viewport
            got = _frame(ws, ctx, r, pc, sc, values)
            fresh = _renderer(ws, ctx)
            try:
                want = _frame(ws, ctx, fresh, pc, sc, values)
            finally:
                fresh.close()
            assert sorted(got) == sorted(want) == sorted(["target", "aux_depth", "aux_median_depth", "aux_alpha", "values", "winner",
                                                          "base", "contrib_q32", "contrib_max", "composite"])
            for key in ("target", "base", "composite"):
                assert got[key].shape == (h, w, 4), key
            for key in ("aux_depth", "aux_median_depth", "aux_alpha", "winner"):
                assert got[key].shape == (h, w), key
            assert got["values"].shape == (h, w, 1)
            for key in got:
                assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (sc.viewport, key)
            assert got["target"][..., 3].max() > 0 and got["contrib_q32"].any()  # (the frames are not empty)
    finally:
        r.close()
        r.close()
        pc.close()


def test_plane_calls_before_prepare_end_in_the_librarys_error(ws, ctx, oracle):
    """No prepare(): the viewport is (0, 0), the planes are one element each, and the library refuses the call before any launch."""
    sc = scenes.c1(ws, oracle, n=N, viewport=(64, 48), seed=5)
    pc = ws.PointCloud(ctx, sc.gpc)
    r = _renderer(ws, ctx)
    contrib = ws.Contrib(ctx, N)
    try:
        with pytest.raises(ws.WebSplatError) as e:
            r.render(pc)
        assert e.value.code == -5
        for call in (lambda: r.render_aux(pc), lambda: r.render_values(pc, winner=True),
                     lambda: r.accumulate_removal(pc, contrib, base=True)):
            with pytest.raises(ws.WebSplatError):
                call()
        with pytest.raises(ValueError):
            r.upload_target(np.zeros((48, 64, 4), np.float32))
        r.prepare(pc, sc.args)  # and the renderer still works: the one-element planes are let go for the viewport's
        r.render(pc)
        assert r.download_target().shape == (48, 64, 4)
    finally:
        contrib.close()
        r.close()
        pc.close()


def test_view_batch_renderer_view(ws, ctx, oracle):
    """ViewBatch.renderer(slot) is a whole GaussianRenderer on the slot's handle: it answers, its plane methods end in the
    library's own error (the view was never prepared through this object), never in an AttributeError, and its close() leaves
    the slot alone."""
    sc = scenes.c1(ws, oracle, n=N, viewport=(64, 48), seed=5)
    w, h = sc.viewport
    pc = ws.PointCloud(ctx, sc.gpc)
    batch = ws.ViewBatch(ctx, "rgba32float", 3, False, frames_in_flight=2)
    targets = [ctx.malloc(w * h * 16) for _ in range(2)]
    try:
        batch.render(pc, [sc.args] * 2, targets, w * 16)
        batch.sync()
        first = ctx.download(targets[0], (h, w, 4), np.float32)
        view = batch.renderer(0)
        assert view.frame_stats()["num_visible"] > 0
        with pytest.raises(ws.WebSplatError):
            view.render_aux(pc)
        view.close()
        view.close()
        batch.render(pc, [sc.args] * 2, targets, w * 16)
        batch.sync()
        assert batch.errors() == 0
        assert np.array_equal(ctx.download(targets[0], (h, w, 4), np.float32), first)
        assert np.array_equal(ctx.download(targets[1], (h, w, 4), np.float32), first)
    finally:
        batch.close()
        for t in targets:
            ctx.free(t)
        pc.close()
