"""One captured frame graph through every event that must drop it (web-splat_amd/csrc/frame_graph.h, api_renderer.cpp
renderer_free_graph): the frame-graph sibling of test_gpu_scratch_lifecycle.py, which runs with the graph off.  One renderer of a
use_graph=1 context draws on a real non-blocking stream; after each step its frame is error-free and byte-equal to what a fresh
renderer of a use_graph=0 context draws for that cloud and viewport (a frame is a pure function of scene and camera,
test_gpu_render.py test_determinism_and_reuse), so a graph that was replayed where it had to be captured anew, a ring slot patched
while its last launch was pending, or a handle let go too early shows here.  Nothing is provoked: every call is one the suite makes
at larger shapes (test_gpu_fullsize.py test_frame_graph_replay_equals_launch_by_launch).

The expected images and both point clouds are made first, and everything between the graph's launches -- clearing the targets,
the downloads, the error words -- is ordered on the renderer's own stream: legacy-NULL-stream work between two launches of a used
executable graph is what made the graph opt-in."""
import ctypes as C

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu


def _ctx(ws, **cfg):
    return ws.Context(0, ws.config_from_env({}, **cfg))


def test_one_graph_through_every_event_that_drops_it(ws, oracle):
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking
    cg, cn = _ctx(ws, use_graph=1), _ctx(ws, use_graph=0)
    made, bufs = [], []
    try:
        s = stream.value
        sc_a = scenes.c1(ws, oracle, n=4000, viewport=(320, 240))
        sc_b = scenes.c1(ws, oracle, n=4000, viewport=(96, 64))      # the same cloud (same seed), a smaller target
        sc_2 = scenes.c1(ws, oracle, n=1500, viewport=(320, 240), seed=3)
        pn, pn2 = ws.PointCloud(cn, sc_a.gpc), ws.PointCloud(cn, sc_2.gpc)
        pc, pc2 = ws.PointCloud(cg, sc_a.gpc), ws.PointCloud(cg, sc_2.gpc)
        made += [pn, pn2, pc, pc2]

        def fresh(cloud, sc, capacity=0):
            f = ws.GaussianRenderer(cn, "rgba32float", 3, False)
            try:
                f.set_tile_entry_capacity(capacity)
                f.prepare(cloud, sc.args)
                f.render(cloud)
                return f.download_target().copy(), f.frame_stats()
            finally:
                f.close()

        want_a, stats_a = fresh(pn, sc_a)
        want_b, _ = fresh(pn, sc_b)
        want_2, _ = fresh(pn2, sc_2)
        want_a_1000, _ = fresh(pn, sc_a, capacity=1000)
        assert stats_a["overflow"] == 0 and stats_a["num_tile_entries"] > 1000 and not np.array_equal(want_a, want_a_1000)
        assert not np.array_equal(want_a, want_2)

        bufs += [cg.malloc(320 * 240 * 16) for _ in range(6)]
        r = ws.GaussianRenderer(cg, "rgba32float", 3, False)
        made.append(r)

        def frame(step, cloud, sc, want, bits=0, count=1):
            w, h = sc.viewport
            blank = np.zeros((h, w, 4), np.float32)
            for b in bufs[:count]:                     # (a frame that drew nothing must not pass on an earlier step's image)
                cg.upload(b, blank, stream=s)
            for b in bufs[:count]:                     # enqueued back to back: no sync, no read-back in between
                r.prepare(cloud, sc.args, stream=s)
                r.render(cloud, target_ptr=b, pitch=w * 16, stream=s)
            cg.sync(s)
            assert r.errors()[0] == bits, step
            for i, b in enumerate(bufs[:count]):
                got = np.empty((h, w, 4), np.float32)
                ws.check(ws.lib.ws_memcpy_d2h(cg.handle, got.ctypes.data_as(C.c_void_p), C.c_void_p(b), got.nbytes, C.c_void_p(s)))
                assert np.array_equal(got, want), (step, i)

        frame("first frame", pc, sc_a, want_a)
        frame("six frames past the ring of four", pc, sc_a, want_a, count=6)
        frame("viewport A -> B", pc, sc_b, want_b)
        frame("viewport B -> A", pc, sc_a, want_a)
        # 1000 entries are far too few for this frame (test_gpu_render.py: entries are dropped and flagged, bit 0, nothing else):
        # the same bytes as a fresh renderer with that capacity; the flag is sticky, so it is reset before the next step
        r.set_tile_entry_capacity(1000)
        frame("entry capacity 1000", pc, sc_a, want_a_1000, bits=1)
        assert r.errors(reset=True)[0] == 1
        r.set_tile_entry_capacity(0)
        frame("entry capacity 1000 -> automatic", pc, sc_a, want_a)
        r.enable_depth(True)
        frame("depth on", pc, sc_a, want_a)
        r.enable_depth(False)
        frame("depth off", pc, sc_a, want_a)
        frame("a second cloud of 1500 points", pc2, sc_2, want_2)
        frame("back to the first cloud", pc, sc_a, want_a)
    finally:
        for h in reversed(made):
            h.close()
        for b in bufs:
            cg.free(b)
        cg.close()
        cn.close()
        hip.hipStreamDestroy(stream)
