"""GPU tests of ws_scene_evaluate (include/websplat.h "Image metrics"): a cloud against itself, a pruned subset against its
parent, and renders against ground-truth PNGs of another size -- every record checked against tests/metrics_ref.py on the two
images rendered separately through the Python API with the same setup (frames are reproducible bit for bit)."""
import json

import numpy as np
import pytest

import metrics_ref as mr
import scenes
from websplat import synth

pytestmark = pytest.mark.gpu

N = 2_000
VIEW = (160, 120)


def _png_name(cam):
    return cam.img_name if cam.img_name.lower().endswith(".png") else cam.img_name + ".png"


@pytest.fixture(scope="module")
def world(ws, oracle):
    c = ws.Context(0, ws.config_from_env({}))
    sc = scenes.c1(ws, oracle, n=N, viewport=VIEW)
    pc = ws.PointCloud(c, sc.gpc)
    cams = synth.orbit_cameras(3, VIEW[0], VIEW[1], 150.0, 150.0, radius=3.0, height_off=0.4)
    cams[1].img_name = "view_b.PNG"   # (a name that already carries the extension, in capitals)
    scene = ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams]))
    yield c, pc, scene
    scene.close()
    pc.close()
    c.close()


def _render(ws, c, cloud, cam, size):
    """One frame as ws_render_views sets it up, at `size`: Rgba16Float, cleared to transparent, the target-precision blend."""
    r = ws.GaussianRenderer(c, "rgba16float", cloud.sh_deg(), False)
    try:
        r.set_blend_mode("target")
        pcam = cam.to_perspective().fit_near_far(cloud.bbox())
        r.prepare(cloud, ws.SplattingArgs(camera=pcam, viewport=size, max_sh_deg=cloud.sh_deg(), walltime=100.0))
        r.render(cloud)
        assert r.errors()[0] == 0
        return r.download_target()
    finally:
        r.close()


def _check(rec, ref, quantize):
    assert (rec["width"], rec["height"]) == (ref["width"], ref["height"])
    if quantize:
        assert rec["sse_u8"] == ref["sse_u8"] and abs(rec["mse"] - ref["mse"]) <= 1e-12 * ref["mse"]
    else:
        assert abs(rec["mse"] - ref["mse"]) <= 1e-5 * ref["mse"]
    assert abs(rec["ssim"] - ref["ssim"]) <= mr.tolerances(ref)[0]
    assert rec["psnr"] == pytest.approx(ref["psnr"], abs=1e-4)


def test_cloud_against_itself(ws, world):
    c, pc, scene = world
    m = ws.Metrics(c, 3)
    try:
        assert ws.evaluate_scene(c, pc, scene, None, m, ref=pc) == 3 and m.count == 3
        recs = m.download()
        assert len(recs) == 3
        for r in recs:
            assert r["mse"] == 0.0 and r["psnr"] == float("inf") and (r["width"], r["height"]) == VIEW and abs(r["ssim"] - 1) <= 1e-6
    finally:
        m.close()


def test_pruned_subset_against_parent(ws, world):
    c, pc, scene = world
    contrib = ws.Contrib(c, pc.num_points())
    try:
        for split in ("train", "test"):
            ws.accumulate_contrib_scene(c, pc, scene, split, contrib)
        _, _, mw = contrib.download()
    finally:
        contrib.close()
    t = float(np.median(mw[mw > 0]))
    idx = np.nonzero(mw > t)[0].astype(np.uint32)
    assert 0.3 * pc.num_points() <= idx.size <= 0.7 * pc.num_points(), idx.size    # (the case is not vacuous)
    sub = pc.subset(idx)
    m = ws.Metrics(c, 6)
    try:
        assert ws.evaluate_scene(c, sub, scene, None, m, ref=pc) == 3
        assert ws.evaluate_scene(c, sub, scene, None, m, ref=pc, quantize_u8=True) == 3
        recs = m.download()
        assert len(recs) == 6 and [r["flags"] for r in recs] == [0, 0, 0, 1, 1, 1]
        bg = pc.background_color()
        bg = (0.0, 0.0, 0.0) if bg is None else bg
        for i, cam in enumerate(scene.cameras(None)):
            a, b = _render(ws, c, sub, cam, VIEW), _render(ws, c, pc, cam, VIEW)
            for quantize in (False, True):
                ref = mr.reference(a, b, bg_a=bg, bg_b=bg, quantize=quantize)
                assert ref["mse"] > 0                                             # pruning cost something
                _check(recs[i + 3 * quantize], ref, quantize)
    finally:
        m.close()
        sub.close()


def test_ground_truth_pngs(ws, world, tmp_path):
    from websplat import _lib as L
    c, pc, scene = world
    cams = scene.cameras(None)
    small = (96, 72)                                                              # the aspect of 160 x 120 at another size
    gt = tmp_path / "gt"
    gt.mkdir()
    truth = []
    for cam in cams:
        img = _render(ws, c, pc, cam, small)
        rgba8 = mr.pixel_value(np.concatenate([img[..., :3], np.ones_like(img[..., :1])], -1), quantize=True)[1]
        rgba8 = np.concatenate([rgba8, np.full(rgba8.shape[:2] + (1,), 255, np.uint8)], -1)
        rgba8[::7, ::5, :3] ^= 0x10                                               # (a ground truth that is not the render)
        ws.write_png(str(gt / _png_name(cam)), rgba8)
        truth.append((img, rgba8))
    m = ws.Metrics(c, 8)
    try:
        for quantize in (False, True):
            m.reset()
            assert ws.evaluate_scene(c, pc, scene, None, m, gt_dir=str(gt), quantize_u8=quantize) == 3
            recs = m.download()
            assert [(r["width"], r["height"]) for r in recs] == [small] * 3
            for r, (img, rgba8) in zip(recs, truth):
                ref = mr.reference(img, rgba8, bg_a=(0.0, 0.0, 0.0), quantize=quantize)
                assert ref["mse"] > 0
                _check(r, ref, quantize)
        # splits: the first camera of the file is the test view
        m.reset()
        assert ws.evaluate_scene(c, pc, scene, "test", m, gt_dir=str(gt)) == 1 and ws.evaluate_scene(c, pc, scene, "train", m, gt_dir=str(gt)) == 2
        assert m.count == 3
        # another aspect: refused, naming the file; the accumulator keeps what it had
        ws.write_png(str(gt / _png_name(cams[1])), np.zeros((64, 96, 4), np.uint8))
        with pytest.raises(ws.WebSplatError) as e:
            ws.evaluate_scene(c, pc, scene, None, m, gt_dir=str(gt))
        assert e.value.code == L.WS_ERR_INVALID and _png_name(cams[1]) in str(e.value) and m.count == 3
        # a missing file
        (gt / _png_name(cams[1])).unlink()
        with pytest.raises(ws.WebSplatError) as e:
            ws.evaluate_scene(c, pc, scene, None, m, gt_dir=str(gt))
        assert e.value.code == L.WS_ERR_IO and _png_name(cams[1]) in str(e.value)
        assert cams[1].img_name.encode() in ws.lib.ws_last_error() and m.count == 3
        # exactly one of ref / gt_dir
        for kw in (dict(), dict(ref=pc, gt_dir=str(gt))):
            with pytest.raises(ws.WebSplatError) as e:
                ws.evaluate_scene(c, pc, scene, None, m, **kw)
            assert e.value.code == L.WS_ERR_INVALID
    finally:
        m.close()
