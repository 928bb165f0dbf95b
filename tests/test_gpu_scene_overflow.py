"""GPU tests of the scene drivers' overflow paths (web-splat_amd/csrc/drivers.cpp): frames whose (tile, splat) demand exceeds the
automatic entry capacity, through the three policies the drivers have --

   ws_render_views                      per frame: look at the bits, grow the entry list, draw the frame again
   ws_scene_evaluate against a cloud    per pass: grow both renderers and run the whole split again, on the same renderers
   the accumulators                     no retry: WS_ERR_OVERFLOW, "... incomplete"

and of the camera with an empty image, which every driver refuses before its first frame.

The scene is the heavy cloud of test_gpu_drivers.test_measure_survives_a_scene_heavier_than_the_automatic_capacity under two orbit
cameras declared at 2000 x 2000 (drawn at 1600 x 1600, the width cap).  ws_render_views takes one split at a time and the first
camera of a file is its test view, so a small camera that nothing here draws stands at file position 0 and the two heavy ones
are the train split."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

SIZE = (1600, 1600)


def _args(ws, cloud, cam):
    """The frame of ws_render_views (offline_args): the camera as declared, near / far fitted to the cloud, the capped viewport."""
    pcam = cam.to_perspective().fit_near_far(cloud.bbox())
    return ws.SplattingArgs(camera=pcam, viewport=SIZE, max_sh_deg=cloud.sh_deg(), walltime=100.0)


@pytest.fixture(scope="module")
def world(ws):
    c = ws.Context(0, ws.config_from_env({}))
    rows = synth.scene_c1(n=25_000, seed=5)
    rows[:, 55:58] = np.log(0.45)
    rows[:, 54] = -3.0
    pc = ws.PointCloud.from_ply_rows(c, rows, 3)
    cams = synth.orbit_cameras(3, 2000, 2000, 1800.0, 1800.0, radius=3.0, height_off=0.3)
    cams[0].width, cams[0].height, cams[0].fx, cams[0].fy = 200, 150, 180.0, 180.0   # (file position 0: the test view)
    scene = ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams]))
    heavy = scene.cameras("train")
    assert len(heavy) == 2 and all((cam.width, cam.height) == (2000, 2000) for cam in heavy)
    # not vacuous: a fresh renderer overflows its automatic capacity on every heavy camera, and says how much it needed
    demand = []
    for cam in heavy:
        r = ws.GaussianRenderer(c, "rgba16float", pc.sh_deg(), False)
        try:
            r.set_blend_mode("target")
            r.prepare(pc, _args(ws, pc, cam))
            r.render(pc)
            bits, need = r.errors()
            cap = r.frame_stats()["tile_entries_capacity"]
            print(f"camera {cam.id}: error bits {bits}, tile-entry demand {need}, automatic capacity {cap}")
            assert bits == 1 and need > cap
            demand.append(need)
        finally:
            r.close()
    yield c, pc, scene, heavy, max(demand)
    scene.close()
    pc.close()
    c.close()


def test_render_views_draws_an_overflowed_frame_again(ws, world, tmp_path):
    c, pc, scene, heavy, demand = world
    out = tmp_path / "out"
    assert ws.render_views(c, pc, scene, "train", str(out)) == 2
    r = ws.GaussianRenderer(c, "rgba16float", pc.sh_deg(), False)
    try:
        r.set_blend_mode("target")
        r.set_tile_entry_capacity(2 * demand)   # (room for every entry beforehand: this frame dropped nothing)
        for i, cam in enumerate(heavy):
            r.prepare(pc, _args(ws, pc, cam))
            r.render(pc)
            assert r.errors()[0] == 0
            rgba8 = r.download_target_rgba8()
            assert rgba8.shape == (1600, 1600, 4) and (rgba8[..., 3] > 0).mean() > 0.5
            by_hand = tmp_path / f"by_hand_{i}.png"
            ws.write_png(str(by_hand), rgba8)
            assert (out / "train" / f"{i:05d}.png").read_bytes() == by_hand.read_bytes()
    finally:
        r.close()


def test_evaluate_against_a_cloud_runs_an_overflowed_pass_again(ws, world):
    c, pc, scene, _, _ = world
    m = ws.Metrics(c, 4)
    try:
        assert ws.evaluate_scene(c, pc, scene, "train", m, ref=pc) == 2 and m.count == 2
        assert [r["mse"] for r in m.download()] == [0.0, 0.0]
        assert ws.evaluate_scene(c, pc, scene, "train", m, ref=pc) == 2 and m.count == 4   # (fresh renderers: two passes again)
        recs = m.download()
        assert len(recs) == 4 and all(r["mse"] == 0.0 and (r["width"], r["height"]) == SIZE for r in recs)
    finally:
        m.close()


def test_accumulators_report_an_overflow_and_do_not_retry(ws, world):
    c, pc, scene, _, _ = world
    contrib, grad = ws.Contrib(c, pc.num_points()), ws.Grad(c, pc.num_points())
    try:
        for call in (lambda: ws.accumulate_contrib_scene(c, pc, scene, "train", contrib),
                     lambda: ws.accumulate_gradient_scene(c, pc, scene, "train", grad, ref=pc)):
            with pytest.raises(ws.WebSplatError) as e:
                call()
            assert e.value.code == L.WS_ERR_OVERFLOW and "incomplete" in str(e.value)
    finally:
        contrib.close()
        grad.close()


def test_camera_with_an_empty_image_is_refused_before_the_first_frame(ws, world):
    """cameras.json may carry width 0.  Every driver refuses such a split with WS_ERR_INVALID and 0 frames."""
    c, pc, _, _, _ = world
    cams = synth.orbit_cameras(3, 160, 120, 150.0, 150.0, radius=3.0, height_off=0.4)
    contrib, grad = ws.Contrib(c, pc.num_points()), ws.Grad(c, pc.num_points())
    scenes = []
    try:
        cams[2].width = 0                 # all: two good cameras, then the empty one
        scenes.append(ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams])))
        cams[2].width, cams[0].width = 160, 0   # test: the empty one alone
        scenes.append(ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams])))
        n = C.c_uint32(7)
        rc = ws.lib.ws_scene_accumulate_gradient(c.handle, pc.handle, scenes[0].handle, L.WS_SPLIT_ALL, pc.handle, None, L.WS_ERROR_SQ,
                                                 1.0, 1.0, grad.handle, C.byref(n))
        assert rc == L.WS_ERR_INVALID and n.value == 0 and b"camera with an empty image" in ws.lib.ws_last_error()
        n = C.c_uint32(7)
        rc = ws.lib.ws_scene_accumulate_contrib(c.handle, pc.handle, scenes[1].handle, L.WS_SPLIT_TEST, contrib.handle, C.byref(n))
        assert rc == L.WS_ERR_INVALID and n.value == 0 and b"ws_scene_accumulate_contrib: camera with an empty image" in ws.lib.ws_last_error()
        assert grad.frames == 0 and contrib.frames == 0
    finally:
        for s in scenes:
            s.close()
        contrib.close()
        grad.close()
