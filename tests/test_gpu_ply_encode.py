"""GPU tests of saving a point cloud (include/websplat.h "Saving a point cloud"; ply_encode.hip k_ply_encode):

   1. the kernel against its host twin at block edges: bit for bit outside the four log columns, within 1 f32 ulp inside them
   2. load -> save_ply -> load_ply -> download on the device alone, the four checks of tests/ply_encode_ref.py, both decoders
   3. the header comments, bbox and centre through save and load
   4. prune -> refit -> save -> load: the refitted halves bit for bit, the render of the loaded cloud bit for bit
   5. websplat_evaluate --save
   6. the refusals
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ply_encode_ref as per
import ply_rows
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

F = np.float32
EDGE_NS = (1, 63, 64, 65, 127, 128, 129, 257, 1000)   # k_ply_encode: 128 rows per block


@pytest.fixture(scope="module")
def contexts(ws):
    cs = {"device": ws.Context(0, ws.config_from_env({})), "host": ws.Context(0, ws.config_from_env({"WS_PLY_DECODE": "host"}))}
    yield cs
    for c in cs.values():
        c.close()


def _resident(ws, c, name, sh_deg, n=per.N_CLOUD):
    """the named cloud on the device: decoded from its rows by the load kernel; `edges` uploaded as the blobs it is built as"""
    if name == "edges":
        g, s = per.blobs(name, sh_deg)
        aabb, center, up = ws.pointcloud_stats(g, 28, ws.Aabb([0, 0, 0], [0, 0, 0]))
        return ws.PointCloud(c, ws.GenericGaussianPointCloud(g, s, sh_deg, g.shape[0], aabb, center, up=up))
    return ws.PointCloud.from_ply_rows(c, per.cloud_rows(name, sh_deg, n), sh_deg)


# ---- 1. device against host twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_deg", (0, 3))
def test_kernel_against_host_twin_at_block_edges(ws, contexts, sh_deg):
    c = contexts["device"]
    t = ply_rows.tail_col(sh_deg)
    log_cols = [t, t + 1, t + 2, t + 3]
    other = [k for k in range(ply_rows.row_len(sh_deg)) if k not in log_cols]
    full = per.cloud_rows("aniso", sh_deg)
    worst = 0.0
    for n in EDGE_NS:
        pc = ws.PointCloud.from_ply_rows(c, full[:n], sh_deg)
        try:
            dev = pc.to_ply_rows()
            g, s = pc.download()
        finally:
            pc.close()
        host = ws.encode_ply_rows(g, s, sh_deg)
        assert dev.shape == host.shape == (n, ply_rows.row_len(sh_deg))
        differ = int((dev[:, other].view(np.uint32) != host[:, other].view(np.uint32)).sum())
        u = per.ulps_f32(dev[:, log_cols], host[:, log_cols])
        worst = max(worst, float(u.max()))
        print(f"deg {sh_deg} n {n}: words outside the log columns that differ {differ}, log columns at most {u.max():.2f} ulp apart "
              f"({int((u > 0).sum())} of {u.size} differ)")
        assert differ == 0
        assert u.max() <= 1.0
        per.tail_is_sound(dev, g, s, sh_deg)


def test_rows_that_stay_on_the_device(ws, contexts):
    """ws_pointcloud_encode_ply_rows_device writes what ws_pointcloud_encode_ply_rows copies back; ws_pointcloud_decode_ply_rows_device
    of those rows into another cloud of the size gives what loading them gives."""
    c = contexts["device"]
    sh_deg, n = 2, 300
    pc = ws.PointCloud.from_ply_rows(c, per.cloud_rows("aniso", sh_deg)[:n], sh_deg)
    other = ws.PointCloud.from_ply_rows(c, per.cloud_rows("flat", sh_deg)[:n], sh_deg)
    nbytes = n * 4 * ply_rows.row_len(sh_deg)
    d = c.malloc(nbytes)
    try:
        rows = pc.to_ply_rows()
        pc.encode_ply_rows_device(d, nbytes)
        c.sync()
        assert np.array_equal(c.download(d, rows.shape, F).view(np.uint32), rows.view(np.uint32))
        other.decode_ply_rows_device(d, nbytes)
        c.sync()
        loaded = ws.PointCloud.from_ply_rows(c, rows, sh_deg)
        try:
            (g1, s1), (g2, s2) = other.download(), loaded.download()
        finally:
            loaded.close()
        assert np.array_equal(g1, g2) and np.array_equal(s1, s2)
        for call in (pc.encode_ply_rows_device, other.decode_ply_rows_device):
            with pytest.raises(ws.WebSplatError) as e:
                call(d, nbytes - 4)
            assert e.value.code == L.WS_ERR_INVALID and "too small" in str(e.value)
    finally:
        c.sync()
        c.free(d)
        other.close()
        pc.close()


# ---- 2. round trip on the device alone ----------------------------------------------------------------------------------------------
CASES = [(name, 3) for name in per.CLOUDS] + [("edges", d) for d in (0, 1, 2, 3)]


@pytest.mark.parametrize("decode", ("device", "host"))
@pytest.mark.parametrize("name,sh_deg", CASES)
def test_save_then_load_gives_the_cloud_back(ws, contexts, tmp_path, name, sh_deg, decode):
    c = contexts[decode]
    pc = _resident(ws, c, name, sh_deg)
    try:
        g0, s0 = pc.download()
        path = tmp_path / "saved.ply"
        pc.save_ply(str(path))
        back = ws.PointCloud.load_ply(c, str(path))
        try:
            assert back.num_points() == pc.num_points() and back.sh_deg() == sh_deg
            g1, s1 = back.download()
        finally:
            back.close()
    finally:
        pc.close()
    assert path.stat().st_size == path.read_bytes().index(b"end_header\n") + 11 + g0.shape[0] * 4 * ply_rows.row_len(sh_deg)
    out = per.round_trip(g0, s0, g1, s1, label=f"{name} deg {sh_deg} decode {decode}")
    assert name in ("flat", "edges") or out["margin_rows"] > 1000


# ---- 3. metadata --------------------------------------------------------------------------------------------------------------------
def test_metadata_bbox_and_centre_survive(ws, contexts, tmp_path):
    c = contexts["device"]
    rows = per.cloud_rows("ordinary", 2, 500)
    meta = dict(kernel_size=0.1, mip_splatting=True, background_color=(0.1, 0.2, 1.0 / 3.0))
    pc = ws.PointCloud.from_ply_rows(c, rows, 2, **meta)
    bare = ws.PointCloud.from_ply_rows(c, rows, 2)
    try:
        a, b = tmp_path / "meta.ply", tmp_path / "bare.ply"
        pc.save_ply(str(a))
        bare.save_ply(str(b))
        assert a.read_bytes().count(b"comment ") == 3 and b.read_bytes().count(b"comment ") == 0
        back, back_bare = ws.PointCloud.load_ply(c, str(a)), ws.PointCloud.load_ply(c, str(b))
        try:
            assert back.mip_splatting() is True and F(back.dilation_kernel_size()) == F(0.1)
            assert np.array_equal(np.array(back.background_color(), F), np.array(meta["background_color"], F))
            assert back_bare.mip_splatting() is None and back_bare.dilation_kernel_size() is None and back_bare.background_color() is None
            for x in (back, back_bare):
                assert x.bbox().min == pc.bbox().min and x.bbox().max == pc.bbox().max and x.center() == pc.center() and x.up() == pc.up()
        finally:
            back.close()
            back_bare.close()
    finally:
        pc.close()
        bare.close()


# ---- 4. the pipeline the feature exists for -------------------------------------------------------------------------------------------
VIEW = (64, 64)


def _render(ws, c, cloud, cam, box):
    r = ws.GaussianRenderer(c, "rgba32float", cloud.sh_deg(), False)
    try:
        pcam = cam.to_perspective().fit_near_far(box)
        r.prepare(cloud, ws.SplattingArgs(camera=pcam, viewport=VIEW, max_sh_deg=cloud.sh_deg(), walltime=100.0, clipping_box=box))
        r.render(cloud, background=(0.1, 0.2, 0.3, 1.0))
        assert r.errors()[0] == 0
        return r.download_target().copy()
    finally:
        r.close()


def test_prune_refit_save_load(ws, contexts, tmp_path):
    c = contexts["device"]
    rows = ply_rows.ordinary(1000, 3, 1)
    cams = synth.orbit_cameras(3, VIEW[0], VIEW[1], 60.0, 60.0, radius=3.0, height_off=0.4)
    scene = ws.Scene.from_json_text(json.dumps([cam.to_json() for cam in cams]))
    parent = ws.PointCloud.from_ply_rows(c, rows, 3)
    sub = parent.subset(np.arange(0, 1000, 2, dtype=np.uint32))
    fit = ws.Refit(c, sub)
    try:
        g_before, s_before = sub.download()
        assert ws.refit_scene(c, sub, scene, "train", fit, ref=parent, epochs=2, views_per_step=0, lr_colour=0.005, lr_opacity=0.01) == 2
        g0, s0 = sub.download()
        moved = (per.split(g0, s0)[1] != per.split(g_before, s_before)[1]).sum()
        assert moved > 100, moved                                                   # (the refit did something to save)
        path = tmp_path / "refitted.ply"
        sub.save_ply(str(path))
        back = ws.PointCloud.load_ply(c, str(path))
        try:
            g1, s1 = back.download()
            (pos0, op0, cov0, sh0), (pos1, op1, cov1, sh1) = per.split(g0, s0), per.split(g1, s1)
            assert np.array_equal(op0, op1) and np.array_equal(sh0[:, :3], sh1[:, :3])   # the refitted halves, bit for bit
            assert np.array_equal(sh0, sh1) and np.array_equal(pos0.view(np.uint32), pos1.view(np.uint32))
            assert np.array_equal(cov0, cov1)                                       # every covariance came back identical: the image check is bitwise
            box = sub.bbox()                                                        # (a subset keeps its parent's box; the file's own is tighter)
            for cam in scene.cameras(None):
                a, b = _render(ws, c, sub, cam, box), _render(ws, c, back, cam, box)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.ptp(a[..., :3]) > 0.01
        finally:
            back.close()
    finally:
        fit.close()
        sub.close()
        parent.close()
        scene.close()


# ---- 5. the tool ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_tool_saves(ws, tmp_path):
    rows = synth.scene_c1(n=2_000, seed=0, sh_deg=3)                                # the small scene of tests/test_gpu_evaluate.py
    ply, out_ply, cj = tmp_path / "scene.ply", tmp_path / "out.ply", tmp_path / "cameras.json"
    synth.write_ply(str(ply), rows)
    cams = synth.orbit_cameras(3, 160, 120, 150.0, 150.0, radius=3.0, height_off=0.4)
    cj.write_text(json.dumps([cam.to_json() for cam in cams]))
    exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
    out = subprocess.run([exe, str(ply), str(cj), "--ref", str(ply), "--refit", "1", "--save", str(out_ply)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    last = out.stdout.splitlines()[-1]
    m = re.fullmatch(r"saved (.+): (\d+) Gaussians, (\d+) bytes", last)
    assert m and m.group(1) == str(out_ply) and int(m.group(2)) == 2000 and int(m.group(3)) == out_ply.stat().st_size
    assert "after refit: 1 epochs" in out.stdout
    back = ws.read_ply(str(out_ply))
    assert back.num_points == 2000 and back.sh_deg == 3
    again = subprocess.run([exe, str(out_ply), str(cj), "--ref", str(out_ply)], capture_output=True, text=True, timeout=120)
    assert again.returncode == 0, again.stderr
    lines = again.stdout.splitlines()
    assert lines[-1].startswith("mean over 1 images: PSNR inf") and all(re.search(r"PSNR\s+inf", ln) for ln in lines[:-1]), again.stdout
    # --save alone converts; a compressed scene is refused with the library's message
    alone = subprocess.run([exe, str(ply), str(cj), "--save", str(tmp_path / "copy.ply")], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 0 and alone.stdout.startswith("saved ") and "PSNR" not in alone.stdout, alone.stderr
    npz = tmp_path / "packed.npz"
    synth.write_npz(str(npz), synth.c3dgs_arrays(n=2000, n_geometry=256, n_sh=256))
    bad = subprocess.run([exe, str(npz), str(cj), "--save", str(tmp_path / "packed.ply")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "ws_pointcloud_save_ply" in bad.stderr and "compressed" in bad.stderr and not (tmp_path / "packed.ply").exists()


# ---- 6. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(ws, contexts, tmp_path):
    c = contexts["device"]
    npz = tmp_path / "packed.npz"
    synth.write_npz(str(npz), synth.c3dgs_arrays(n=500, n_geometry=64, n_sh=64))
    packed = ws.PointCloud.load_npz(c, str(npz))
    pc = ws.PointCloud.from_ply_rows(c, per.cloud_rows("ordinary", 1, 130), 1)
    try:
        with pytest.raises(ws.WebSplatError) as e:
            packed.to_ply_rows()
        assert e.value.code == L.WS_ERR_UNSUPPORTED and "compressed" in str(e.value)
        with pytest.raises(ws.WebSplatError) as e:
            packed.save_ply(str(tmp_path / "packed.ply"))
        assert e.value.code == L.WS_ERR_UNSUPPORTED and "compressed" in str(e.value) and not (tmp_path / "packed.ply").exists()
        rows = np.full((130, ply_rows.row_len(1)), 7.0, F)
        rc = ws.lib.ws_pointcloud_encode_ply_rows(pc.handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes - 4)
        assert rc == L.WS_ERR_INVALID and b"too small" in ws.lib.ws_last_error() and (rows == 7.0).all()
        assert ws.lib.ws_pointcloud_encode_ply_rows(pc.handle, None, rows.nbytes) == L.WS_ERR_INVALID
        assert ws.lib.ws_pointcloud_save_ply(pc.handle, None) == L.WS_ERR_INVALID
        for call in (packed.encode_ply_rows_device, packed.decode_ply_rows_device):
            with pytest.raises(ws.WebSplatError) as e:
                call(0, 0)
            assert e.value.code == L.WS_ERR_UNSUPPORTED
        with pytest.raises(ws.WebSplatError) as e:
            pc.save_ply(str(tmp_path / "no_such_directory" / "x.ply"))
        assert e.value.code == L.WS_ERR_IO
        assert ws.lib.ws_pointcloud_encode_ply_rows(pc.handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes) == L.WS_OK and not (rows == 7.0).any()
    finally:
        pc.close()
        packed.close()
