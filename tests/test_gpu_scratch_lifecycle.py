"""One renderer through every call that makes it let device memory go or take new memory (api_renderer.cpp renderer_ensure_scratch and
the arrays allocated on first use: frame_scratch.h), in turn.  After each step the frame it draws is error-free and byte-equal to
what a fresh renderer draws for that cloud and viewport: a frame is a pure function of scene and camera
(test_gpu_render.py test_determinism_and_reuse), so an array that a reallocation left too short, stale or uninitialised shows here.
Nothing is provoked: every step is a call the suite makes elsewhere."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu


def test_one_renderer_through_every_reallocation(ws, ctx, oracle):
    sc_a = scenes.c1(ws, oracle, n=4000, viewport=(320, 240))
    sc_b = scenes.c1(ws, oracle, n=4000, viewport=(96, 64))      # the same cloud (same seed), a smaller target
    # ... and one of 24 x 22 tiles: the time-stamped blend instruments whole 32x32 tiles only, and below 2 x 256 tiles a frame is
    # composited in half tiles (frame_plan.h split_wanted), where render() refuses it
    sc_t = scenes.c1(ws, oracle, n=4000, viewport=(768, 704))
    sc_2 = scenes.c1(ws, oracle, n=1500, viewport=(320, 240), seed=3)
    pc, pc2 = ws.PointCloud(ctx, sc_a.gpc), ws.PointCloud(ctx, sc_2.gpc)
    contrib = ws.Contrib(ctx, 4000)
    r = ws.GaussianRenderer(ctx, "rgba32float", 3, False)
    made = [pc, pc2, contrib, r]

    def fresh(cloud, sc, capacity=0):
        f = ws.GaussianRenderer(ctx, "rgba32float", 3, False)
        try:
            f.set_tile_entry_capacity(capacity)
            f.prepare(cloud, sc.args)
            f.render(cloud)
            return f.download_target().copy(), f.frame_stats()
        finally:
            f.close()

    try:
        want_a, stats_a = fresh(pc, sc_a)
        want_b, _ = fresh(pc, sc_b)
        want_t, _ = fresh(pc, sc_t)
        want_2, _ = fresh(pc2, sc_2)
        want_a_1000, _ = fresh(pc, sc_a, capacity=1000)
        assert stats_a["overflow"] == 0 and not np.array_equal(want_a, want_a_1000)
        print("tile entries of the 4000-point frame at 320x240:", stats_a["num_tile_entries"])

        def frame(step, cloud, sc, want, bits=0, between=None):
            r.prepare(cloud, sc.args)
            if between:
                between()
            r.render(cloud)
            got = r.download_target()
            assert r.errors()[0] == bits, step
            assert got.shape == want.shape and np.array_equal(got, want), step

        frame("first frame", pc, sc_a, want_a)
        frame("viewport A -> B", pc, sc_b, want_b)
        frame("viewport B -> A", pc, sc_a, want_a)
        # 1000 entries are far too few for this frame (test_gpu_render.py: entries are dropped and flagged, bit 0, nothing else):
        # the same bytes as a fresh renderer with that capacity; the flag is sticky, so it is reset before the next step
        assert stats_a["num_tile_entries"] > 1000
        r.set_tile_entry_capacity(1000)
        frame("entry capacity 1000", pc, sc_a, want_a_1000, bits=1)
        assert r.errors(reset=True)[0] == 1
        r.set_tile_entry_capacity(0)
        frame("entry capacity 1000 -> automatic", pc, sc_a, want_a)
        r.enable_depth(True)
        frame("depth on", pc, sc_a, want_a)
        r.enable_depth(False)
        frame("depth off", pc, sc_a, want_a)
        frame("viewport A -> T", pc, sc_t, want_t)
        r.enable_blend_timing(True)
        frame("blend timing on", pc, sc_t, want_t)
        stamps = r.blend_timing()
        assert stamps.shape == (24 * 22, 16, 16) and stamps.any()
        r.enable_blend_timing(False)
        frame("blend timing off", pc, sc_t, want_t)
        frame("viewport T -> A", pc, sc_a, want_a)
        r.enable_frame_trace(2)
        frame("frame trace 2", pc, sc_a, want_a)
        r.enable_frame_trace(0)
        frame("frame trace 0", pc, sc_a, want_a)
        r.enable_contrib(True)
        frame("removal effect into the renderer's own base plane", pc, sc_a, want_a, between=lambda: r.accumulate_removal(pc, contrib))
        r.enable_contrib(False)
        frame("a second cloud of 1500 points", pc2, sc_2, want_2)
        frame("back to the first cloud", pc, sc_a, want_a)
    finally:
        for h in reversed(made):
            h.close()
