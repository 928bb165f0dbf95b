"""Per-Gaussian contribution sums over frames (include/websplat.h "Per-Gaussian contributions", contrib.hip k_contrib).

  1. against a float64 front-to-back walk of the device's own frame (tests/contrib_ref.py), every Gaussian compared, over the
     tile shapes, binning shifts and split setting, and on a compressed cloud; tile lists of exactly the lengths at which
     the staging changes batch or sub-round
  2. oracle-free: the sums add up to the coverage plane; bitwise reproducible, additive over frames and accumulators; the
     sum / max invariants; culled Gaussians are exactly 0
  3. enable_contrib changes no pixel; the error cases of the C ABI
  4. ws_scene_accumulate_contrib equals the manual prepare / accumulate loop"""
import ctypes as C
import json

import numpy as np
import pytest

import contrib_ref
import scenes
from attrib_frames import _compressed, _ctx, _stack
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _accumulate(ws, c, pc, args, compressed=False, sh_deg=3, with_frame=False, with_alpha=False):
    """One frame into a fresh accumulator: dict(sum, q, max [, frame] [, alpha, longest])."""
    r = ws.GaussianRenderer(c, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(c, pc.num_points())
    try:
        r.enable_contrib(True)
        r.prepare(pc, args)
        r.accumulate_contrib(pc, acc)
        s, q, m = acc.download()
        assert acc.frames == 1
        assert r.frame_stats()["overflow"] == 0
        out = {"sum": s, "q": q, "max": m}
        if with_frame:
            out["frame"] = r.download_frame(with_src_index=True)
        if with_alpha:
            r.render_aux(pc, depth=False, median_depth=False, alpha=True)
            out["alpha"] = r.download_aux()["alpha"]
            out["longest"] = int(r.tile_stats()["list_len"].max())
        return out
    finally:
        acc.close()
        r.close()


def _compare(got, ref, min_drawn=1000):
    tol_sum, tol_max = contrib_ref.bounds(ref)
    d_sum = np.abs(got["sum"] - ref["sum"])
    d_max = np.abs(got["max"].astype(np.float64) - ref["max"])
    drawn = int((got["sum"] > 0).sum())
    worst_s, worst_m = int(np.argmax(d_sum - tol_sum)), int(np.argmax(d_max - tol_max))
    print(f"gaussians {len(d_sum)} drawn {drawn} with P {int((ref['P'] > 0).sum())} with U {int((ref['U'] > 0).sum())}; "
          f"sum: max |d| {d_sum.max():.3e}, worst excess {(d_sum - tol_sum)[worst_s]:.3e} at {worst_s} "
          f"(ref {ref['sum'][worst_s]:.6e}, tol {tol_sum[worst_s]:.3e}); max rel err without P/U "
          f"{np.max(np.where((ref['P'] == 0) & (ref['U'] == 0) & (ref['sum'] > 0), d_sum / np.maximum(ref['sum'], 1e-300), 0)):.3e}; "
          f"max: max |d| {d_max.max():.3e}, worst excess {(d_max - tol_max)[worst_m]:.3e} at {worst_m}")
    assert drawn > min_drawn
    assert np.all(d_sum <= tol_sum), f"{int((d_sum > tol_sum).sum())} sums out of bound"
    assert np.all(d_max <= tol_max), f"{int((d_max > tol_max).sum())} maxima out of bound"


# ---- 1. against float64 ------------------------------------------------------------------------------------------------
F64_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"tile_qw": 4, "tile_qh": 2}, {"bin_request": 0}, {"bin_request": 2}, {"blend_split": 1}]
_REF_CACHE = {}  # seed -> (frame, reference): K1 and the depth sort do not depend on the tile configuration


def _reference(key, frame, width, height, n):
    hit = _REF_CACHE.get(key)
    if hit is not None and all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
        return hit[1]
    ref = contrib_ref.contrib_f64(frame, width, height, n)
    _REF_CACHE[key] = (frame, ref)
    return ref


@pytest.mark.parametrize("cfg", F64_CONFIGS, ids=["-".join(f"{k}{v}" for k, v in c.items()) or "default" for c in F64_CONFIGS])
@pytest.mark.parametrize("seed", [0, 7])
def test_against_f64_c1(ws, oracle, seed, cfg):
    c = _ctx(ws, **cfg)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=(320, 240), seed=seed)
        pc = ws.PointCloud(c, sc.gpc)
        try:
            got = _accumulate(ws, c, pc, sc.args, with_frame=True)
            _compare(got, _reference(("c1", seed), got["frame"], 320, 240, pc.num_points()))
        finally:
            pc.close()
    finally:
        c.close()


# list lengths around the batch size (STAGE = 512 at the 4x4 tile, 256 at 2x2) and the sub-round size (LCAP), one and two batches
BOUNDARY_CASES = [({}, k) for k in (1, 511, 512, 513, 1024, 1025)] + [({"tile_qw": 2, "tile_qh": 2}, k) for k in (255, 256, 257, 513)]


@pytest.mark.parametrize("opacity", [0.002, 0.9], ids=["faint", "opaque"])
@pytest.mark.parametrize("cfg,k", BOUNDARY_CASES, ids=[f"{'2x2' if c else '4x4'}-{k}" for c, k in BOUNDARY_CASES])
def test_list_lengths_at_staging_boundaries(ws, cfg, k, opacity):
    """Tile lists of exactly k entries.  Faint: T stays above T_MIN (0.998^1025 = 0.13), every batch is walked to its end and
    every Gaussian draws.  Opaque: every pixel is below T_MIN after ~60 layers (b >= 0.15 at the corners), the tile saturates
    inside its first batch, the walk and the batch loop take their early exits and the Gaussians behind get exactly 0 (a single
    Gaussian, k = 1, saturates nothing: it has to draw)."""
    c = _ctx(ws, bin_request=0, **cfg)
    try:
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(_stack(k, opacity), 3)
        cj = synth.look_at_camera(0, [0.0, 0.0, -3.0], [0.0, 0.0, 0.0], 32, 32, 320.0, 320.0)
        cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 32, 32)
        # (the cloud's own box is a segment of the optical axis, for k = 1 a point: near / far fitted to it touch the Gaussians)
        cam.fit_near_far(ws.Aabb([-1, -1, -1], [1, 1, 1]))
        args = ws.SplattingArgs(camera=cam, viewport=(32, 32), max_sh_deg=3)
        pc = ws.PointCloud(c, gpc)
        try:
            got = _accumulate(ws, c, pc, args, with_frame=True, with_alpha=True)  # (asserts overflow == 0)
        finally:
            pc.close()
        q = got["q"]
        print(f"k {k} opacity {opacity} longest list {got['longest']} drawn {int((q > 0).sum())} zero {int((q == 0).sum())}")
        assert got["longest"] == k
        if opacity < 0.5 or k == 1:
            assert np.all(q > 0)
        else:
            assert (q == 0).any() and (q > 0).any()
        _compare(got, contrib_ref.contrib_f64(got["frame"], 32, 32, k), min_drawn=0)
    finally:
        c.close()


def test_against_f64_compressed(ws):
    c = _ctx(ws)
    try:
        gpc, args = _compressed(ws)
        pc = ws.PointCloud(c, gpc)
        try:
            got = _accumulate(ws, c, pc, args, compressed=True, with_frame=True)
            _compare(got, contrib_ref.contrib_f64(got["frame"], 400, 300, pc.num_points()))
        finally:
            pc.close()
    finally:
        c.close()


# ---- 2. oracle-free ----------------------------------------------------------------------------------------------------
def _sums_match_coverage(got, width, height):
    total = float(got["sum"].sum())
    cover = float(got["alpha"].astype(np.float64).sum())
    bound = width * height * 2.0 ** -14 + got["longest"] * 2.0 ** -23 * width * height
    print(f"sum of sums {total:.6f} coverage {cover:.6f} |d| {abs(total - cover):.3e} bound {bound:.3e} longest list {got['longest']}")
    assert cover > 0.01 * width * height
    assert abs(total - cover) <= bound


def test_sums_add_up_to_the_coverage_plane(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=20_000, viewport=(480, 352))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _sums_match_coverage(_accumulate(ws, c, pc, sc.args, with_alpha=True), 480, 352)
        finally:
            pc.close()
    finally:
        c.close()


def test_sums_add_up_to_the_coverage_plane_at_4k(ws, oracle):
    """3840x2160: 8160 tiles, the blend's several-tiles-per-workgroup regime."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c2(n=200_000, seed=1)
        cj = synth.orbit_cameras(4, 3840, 2160, 3840.0, 3840.0)[0]
        sc = scenes.Scene(ws, oracle, rows, 3, cj, (3840, 2160))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            _sums_match_coverage(_accumulate(ws, c, pc, sc.args, with_alpha=True), 3840, 2160)
        finally:
            pc.close()
    finally:
        c.close()


def _orbit_args(ws, gpc, index, viewport=(320, 240)):
    cj = synth.orbit_cameras(5, viewport[0], viewport[1], float(viewport[0]), float(viewport[0]))[index]
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, cj.width, cj.height)
    cam.fit_near_far(gpc.aabb)
    return ws.SplattingArgs(camera=cam, viewport=viewport, max_sh_deg=3)


def test_reproducible_and_additive(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        a1, a2, twice, ab, b_only = (ws.Contrib(c, n) for _ in range(5))
        try:
            r.enable_contrib(True)
            view_a, view_b = _orbit_args(ws, sc.gpc, 0), _orbit_args(ws, sc.gpc, 2)
            r.prepare(pc, view_a)
            r.accumulate_contrib(pc, a1)
            r.accumulate_contrib(pc, a2)
            r.accumulate_contrib(pc, twice)
            r.accumulate_contrib(pc, twice)
            r.accumulate_contrib(pc, ab)
            r.prepare(pc, view_b)
            r.accumulate_contrib(pc, ab)
            r.accumulate_contrib(pc, b_only)
            _, q1, m1 = a1.download()
            _, q2, m2 = a2.download()
            assert (q1 > 0).sum() > 1000
            # the same frame into two fresh accumulators: identical bits
            assert np.array_equal(q1, q2) and np.array_equal(m1.view(np.uint32), m2.view(np.uint32))
            # twice into one: twice the sums, the same maxima
            _, qt, mt = twice.download()
            assert twice.frames == 2
            assert np.array_equal(qt, 2 * q1) and np.array_equal(mt.view(np.uint32), m1.view(np.uint32))
            # frames A and B into one accumulator == add() of two separate ones
            _, qab, mab = ab.download()
            _, qb, mb = b_only.download()
            assert not np.array_equal(qb, q1)
            a1.add(qb, mb)
            _, qsum, msum = a1.download()
            assert np.array_equal(qsum, qab) and np.array_equal(msum.view(np.uint32), mab.view(np.uint32))
            assert np.array_equal(qab, q1 + qb) and np.array_equal(mab, np.maximum(m1, mb))
            # reset: zero again
            a1.reset()
            _, q0, m0 = a1.download()
            assert a1.frames == 0 and not q0.any() and not m0.any()
        finally:
            for a in (a1, a2, twice, ab, b_only):
                a.close()
            r.close()
            pc.close()
    finally:
        c.close()


def test_invariants_and_culled_gaussians_are_zero(ws, oracle):
    """Camera inside the cloud with a clipping box: Gaussians behind the camera or outside the box are exactly 0."""
    c = _ctx(ws)
    try:
        rows = synth.scene_c1(n=20_000, seed=3)
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 3)
        cj = synth.look_at_camera(0, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 320, 240, 200.0, 200.0)
        cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, 320, 240)
        cam.fit_near_far(gpc.aabb)
        box = ws.Aabb([-0.7, -0.7, -0.7], [0.7, 0.7, 0.7])
        args = ws.SplattingArgs(camera=cam, viewport=(320, 240), max_sh_deg=3, clipping_box=box)
        pc = ws.PointCloud(c, gpc)
        try:
            got = _accumulate(ws, c, pc, args)
        finally:
            pc.close()
        q, m = got["q"], got["max"]
        assert np.array_equal(q == 0, m == 0)
        assert float(m.max()) <= 0.99 and float(m.min()) >= 0.0
        assert np.all(q >= (m.astype(np.float64) * 2.0 ** 32).astype(np.uint64))  # (max * 2^32 is exact: the largest single term)
        xyz = rows[:, :3].astype(np.float32)
        behind = xyz[:, 2] < 0
        outside = np.any(xyz < np.float32(-0.7), axis=1) | np.any(xyz > np.float32(0.7), axis=1)
        assert behind.sum() > 5000 and outside.sum() > 5000
        assert not q[behind | outside].any() and not m[behind | outside].any()
        assert (q[~(behind | outside)] > 0).sum() > 500
    finally:
        c.close()


# ---- 3. the frame is untouched; errors -----------------------------------------------------------------------------------
def _frame_images(ws, c, pc, args, fmt, contrib):
    r = ws.GaussianRenderer(c, fmt, 3, False)
    try:
        r.enable_depth(True)
        if contrib is not None:
            r.enable_contrib(contrib)
        r.prepare(pc, args)
        r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
        plain = r.download_target().copy()
        r.render_aux(pc, depth=True, median_depth=True, alpha=True, background=(0.1, 0.2, 0.3, 0.4))
        return plain, r.download_target().copy(), r.download_aux()
    finally:
        r.close()


@pytest.mark.parametrize("fmt", ["rgba32float", "rgba8unorm"])
def test_enable_contrib_changes_no_pixel(ws, oracle, fmt):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=20_000, viewport=(480, 352))
        pc = ws.PointCloud(c, sc.gpc)
        try:
            off = _frame_images(ws, c, pc, sc.args, fmt, None)
            on = _frame_images(ws, c, pc, sc.args, fmt, True)
            assert (off[2]["alpha"] > 0).mean() > 0.05
            assert np.array_equal(_bits(off[0]), _bits(on[0])) and np.array_equal(_bits(off[1]), _bits(on[1]))
            for name in ("depth", "median_depth", "alpha"):
                assert np.array_equal(_bits(off[2][name]), _bits(on[2][name])), name
        finally:
            pc.close()
    finally:
        c.close()


def test_contrib_off_again_and_error_cases(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        n = pc.num_points()
        ra, rb = ws.GaussianRenderer(c, "rgba32float", 3, False), ws.GaussianRenderer(c, "rgba32float", 3, False)
        acc, small = ws.Contrib(c, n), ws.Contrib(c, n - 1)

        def code_of(fn):
            with pytest.raises(ws.WebSplatError) as e:
                fn()
            assert str(e.value).split(":", 1)[1].strip()  # a text in ws_last_error
            return e.value.code

        try:
            # not prepared at all
            ra.enable_contrib(True)
            assert code_of(lambda: ra.accumulate_contrib(pc, acc)) == L.WS_ERR_STATE
            ra.prepare(pc, sc.args)
            ra.accumulate_contrib(pc, acc)
            # another cloud size
            assert code_of(lambda: ra.accumulate_contrib(pc, small)) == L.WS_ERR_INVALID
            # off again: a renderer that never had it
            ra.enable_contrib(False)
            ra.prepare(pc, sc.args)
            ra.render(pc, background=(0.2, 0.1, 0.0, 1.0))
            a = ra.download_target().copy()
            rb.prepare(pc, sc.args)
            rb.render(pc, background=(0.2, 0.1, 0.0, 1.0))
            b = rb.download_target().copy()
            assert np.array_equal(_bits(a), _bits(b))
            assert code_of(lambda: ra.accumulate_contrib(pc, acc)) == L.WS_ERR_STATE
            assert code_of(lambda: rb.accumulate_contrib(pc, acc)) == L.WS_ERR_STATE
            with pytest.raises(ws.WebSplatError):
                ra.download_frame(with_src_index=True)
            assert acc.frames == 1
            # capacities
            q = np.zeros(n, dtype=np.uint64)
            m = np.zeros(n, dtype=np.float32)
            qp, mp = q.ctypes.data_as(C.POINTER(C.c_uint64)), m.ctypes.data_as(C.POINTER(C.c_float))
            assert ws.lib.ws_contrib_download(acc.handle, n - 1, qp, mp) == L.WS_ERR_INVALID
            assert ws.lib.ws_contrib_download(acc.handle, n, qp, None) == L.WS_OK
            assert ws.lib.ws_contrib_download(acc.handle, n, None, mp) == L.WS_OK
            assert (q > 0).sum() > 1000 and np.array_equal(q == 0, m == 0)
            assert ws.lib.ws_contrib_add(acc.handle, qp, mp, n - 1) == L.WS_ERR_INVALID
            assert ws.lib.ws_last_error()
        finally:
            acc.close()
            small.close()
            ra.close()
            rb.close()
        # a context that stops its frames early
        cut = _ctx(ws, debug_cut=2)
        try:
            pc2 = ws.PointCloud(cut, sc.gpc)
            r = ws.GaussianRenderer(cut, "rgba32float", 3, False)
            acc2 = ws.Contrib(cut, n)
            try:
                r.enable_contrib(True)
                r.prepare(pc2, sc.args)
                assert code_of(lambda: r.accumulate_contrib(pc2, acc2)) == L.WS_ERR_UNSUPPORTED
            finally:
                acc2.close()
                r.close()
                pc2.close()
        finally:
            cut.close()
        pc.close()
    finally:
        c.close()


# ---- 4. the scene driver -------------------------------------------------------------------------------------------------
def test_scene_driver_equals_the_manual_loop(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=(320, 240))
        pc = ws.PointCloud(c, sc.gpc)
        n = pc.num_points()
        cams = synth.orbit_cameras(3, 1800, 1200, 1800.0, 1800.0)  # (wider than the 1600-px cap: 1600 x 1066)
        scene = ws.Scene.from_json_text(json.dumps([cj.to_json() for cj in cams]))
        try:
            for split, count in (("train", 2), ("test", 1)):
                driver, manual = ws.Contrib(c, n), ws.Contrib(c, n)
                r = ws.GaussianRenderer(c, "rgba16float", 3, False)
                try:
                    assert ws.accumulate_contrib_scene(c, pc, scene, split, driver) == count
                    assert driver.frames == count
                    r.enable_contrib(True)
                    listed = scene.cameras(split)
                    assert len(listed) == count
                    for cam in listed:
                        w, h = cam.width, cam.height
                        if w > 1600:
                            s = np.float32(w) / np.float32(1600.0)
                            w, h = 1600, int(np.float32(h) / s)
                        pcam = cam.to_perspective().fit_near_far(pc.bbox())
                        r.prepare(pc, ws.SplattingArgs(camera=pcam, viewport=(w, h), max_sh_deg=pc.sh_deg(), walltime=100.0))
                        r.accumulate_contrib(pc, manual)
                    _, qd, md = driver.download()
                    _, qm, mm = manual.download()
                    assert (qd > 0).sum() > 1000
                    assert np.array_equal(qd, qm) and np.array_equal(md.view(np.uint32), mm.view(np.uint32))
                finally:
                    driver.close()
                    manual.close()
                    r.close()
        finally:
            scene.close()
            pc.close()
    finally:
        c.close()
