"""The removal effect (include/websplat.h "Removal effect"; removal.hip k_removal_base, k_removal): what deleting each Gaussian
alone would do to a prepared frame.

   1. against float64 (tests/removal_ref.py), faint stacks at the staging boundaries     6. a decoy in front of a wall of its colour
   2. against float64, a general cloud and a compressed one, masked where undecided     7. the scene driver and websplat_evaluate --removal
   3. delete-one on the device: the subset without j, rendered, against sum[j]           8. the error cases, padded pitches
   4. a saturating stack: bounds, exact zeros behind the stop, reproducible              9. no pixel changes
   5. E == 1, a mask and its complement, the zero plane, merging, other accumulators

A module-scoped fixture writes one row per comparison (worst excess over bounds(), largest |d|) to removal_report.json in
WEBSPLAT_REPORT_DIR (default: test_reports/ under the repository root, as tests/test_gpu_blend_boundary.py)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref
import removal_ref
import scenes
import weight_ref
from attrib_frames import BG, VIEW, F, _cloud_rows, _compressed, _ctx, _Frame, _ramp_checker, _stack_frame, _u32
from websplat import _lib as L
from websplat import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = float(L.WS_CONTRIB_SUM_SCALE)
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "removal_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _compare(case, got_q, got_m, ref, min_drawn=0):
    tol_sum, tol_max = removal_ref.bounds(ref)
    s = got_q.astype(np.float64) / SCALE
    d_sum, d_max = np.abs(s - ref["sum"]), np.abs(got_m.astype(np.float64) - ref["max"])
    drawn = int((got_q > 0).sum())
    held = np.where(tol_sum > 0, d_sum - tol_sum, -np.inf) if (tol_sum > 0).any() else d_sum - tol_sum   # (tol == 0: never drawn, 0 == 0)
    i, k = int(np.argmax(held)), int(np.argmax(np.where(tol_max > 0, d_max - tol_max, -np.inf) if (tol_max > 0).any() else d_max - tol_max))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref["sum"] > 0, d_sum / ref["sum"], 0.0)
    row = dict(case=case, gaussians=len(d_sum), drawn=drawn, worst_excess_sum=float((d_sum - tol_sum)[i]), worst_excess_max=float((d_max - tol_max)[k]),
               largest_diff_sum=float(d_sum.max()), largest_diff_max=float(d_max.max()), largest_rel_sum=float(rel.max()),
               median_tol_over_sum=float(np.median((tol_sum / np.maximum(ref["sum"], 1e-300))[ref["sum"] > 0])) if (ref["sum"] > 0).any() else 0.0,
               largest_d=float(ref["dmax"]), band_pairs=int(ref["band"].sum()))
    REPORT.append(row)
    print(json.dumps(row))
    assert int(ref["U"].sum()) == 0, "a pair that counts at a pixel with an undecided pair: the plane has to mask it"
    assert drawn > min_drawn
    assert np.array_equal(got_q == 0, got_m == 0)
    assert np.all(d_sum <= tol_sum), f"{int((d_sum > tol_sum).sum())} sums out of bound, worst at {i}: got {s[i]:.9e} ref {ref['sum'][i]:.9e} tol {tol_sum[i]:.3e}"
    assert np.all(d_max <= tol_max), f"{int((d_max > tol_max).sum())} maxima out of bound, worst at {k}"
    return row


def _compare_base(row, base, ref, saturating=False, mask=None):
    tol_f, tol_t = removal_ref.base_bounds(ref, saturating)
    d_f = np.abs(base[..., :3].astype(np.float64) - ref["F"]).max(axis=-1)
    d_t = np.abs(base[..., 3].astype(np.float64) - ref["T"])
    ok = np.ones(d_t.shape, bool) if mask is None else mask
    row["base_worst_excess"] = float(max((d_f - tol_f)[ok].max(), (d_t - tol_t)[ok].max()))
    row["base_largest_diff"] = float(max(d_f[ok].max(), d_t[ok].max()))
    print(f"base: largest |dF| {d_f[ok].max():.3e} |dT| {d_t[ok].max():.3e}, worst excess {row['base_worst_excess']:.3e}")
    assert np.all(d_f[ok] <= tol_f[ok]) and np.all(d_t[ok] <= tol_t[ok])


# ---- 1. faint stacks at the staging boundaries ---------------------------------------------------------------------------------
BOUNDARY_CASES = [({}, k) for k in (1, 512, 513, 1025)] + [({"tile_qw": 2, "tile_qh": 2}, k) for k in (256, 257)] + [({"tile_qw": 4, "tile_qh": 2}, 513)]


@pytest.mark.parametrize("cfg,k", BOUNDARY_CASES, ids=[f"{c.get('tile_qw', 4)}x{c.get('tile_qh', 4)}-{k}" for c, k in BOUNDARY_CASES])
def test_against_f64_faint_stacks_at_staging_boundaries(ws, cfg, k):
    """Tile lists of exactly k entries (STAGE = 512 at the 4x4 and 4x2 tiles, 256 at 2x2), every splat over the whole viewport:
    nothing saturates, no pair is near the cut-off, no pixel is masked."""
    c = _ctx(ws, bin_request=0, **cfg)
    try:
        f = _stack_frame(ws, c, k, 0.002)
        try:
            assert int(f.r.tile_stats()["list_len"].max()) == k
            frame = f.frame()
            for kind in ("sq", "abs"):
                scale = 64.0 if kind == "sq" else 1.0   # (d ~ 1e-3 here: d^2 ~ 1e-6 would leave 12 bits above the 2^-32 grid)
                q, m, base = f.removal(kind=kind, scale=scale, base=True)
                ref = removal_ref.removal_f64(frame, 32, 32, k, BG, kind=kind, scale=scale)
                assert int(ref["und"].sum()) == 0 and ref["T"].min() > 2.0 ** -13 and int(ref["band"].sum()) == 0
                row = _compare(f"1-{cfg.get('tile_qw', 4)}x{cfg.get('tile_qh', 4)}-k{k}-{kind}", q, m, ref)
                assert np.all(q > 0)
                _compare_base(row, base, ref)
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. a general cloud --------------------------------------------------------------------------------------------------------
def _cloud_frame(ws, c):
    return _Frame(ws, c, *blend_ref.device_scene(ws, _cloud_rows(), VIEW))


_REF = {}  # K1 and the depth sort do not depend on the tile configuration: one float64 walk serves the cases that share a frame


def _cloud_ref(f):
    """(frame, weight plane E, its mask, the float64 reference under E with scale 1, sq) of the general cloud's frame."""
    frame = f.frame()
    hit = _REF.get("cloud")
    if hit is None or not all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
        w, h = VIEW
        plain = removal_ref.base_f64(frame, w, h, BG)
        ok = ~removal_ref.undecided_mask(plain)
        share = 1.0 - ok.mean()
        print(f"general cloud: {100 * share:.2f} % of the viewport masked (undecided pair or T_end < 2^-13), T_end min {plain['T'].min():.3e}")
        assert share <= 0.02
        E = (_ramp_checker(w, h) * ok).astype(F)
        hit = _REF["cloud"] = (frame, E, ok, removal_ref.removal_f64(frame, w, h, f.n, BG, E=E))
    return hit


F64_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"blend_split": 1}]
_ids = lambda cfgs: ["-".join(f"{k}{v}" for k, v in c.items()) or "default" for c in cfgs]  # noqa: E731


@pytest.mark.parametrize("cfg", F64_CONFIGS, ids=_ids(F64_CONFIGS))
def test_against_f64_general_cloud(ws, cfg):
    c = _ctx(ws, **cfg)
    try:
        f = _cloud_frame(ws, c)
        try:
            frame, E, ok, ref = _cloud_ref(f)
            q, m, base = f.removal(weight=E, base=True)
            row = _compare("2-cloud-" + _ids([cfg])[0], q, m, ref, 1000)
            _compare_base(row, base, ref, mask=ok)
        finally:
            f.close()
    finally:
        c.close()


def test_against_f64_compressed_cloud(ws):
    c = _ctx(ws)
    try:
        gpc, args = _compressed(ws, n=3000)   # (4000 points leave 1.8 % of the view saturated, 6000 14 %; 3000: 0.13 %)
        f = _Frame(ws, c, gpc, args, compressed=True)
        try:
            frame = f.frame()
            plain = removal_ref.base_f64(frame, 400, 300, BG)
            ok = ~removal_ref.undecided_mask(plain)
            share = 1.0 - ok.mean()
            print(f"compressed cloud: {100 * share:.2f} % of the viewport masked, T_end min {plain['T'].min():.3e}")
            assert share <= 0.02
            E = (_ramp_checker(400, 300) * ok).astype(F)
            q, m = f.removal(kind="abs", weight=E)
            _compare("2-compressed-abs", q, m, removal_ref.removal_f64(frame, 400, 300, f.n, BG, kind="abs", E=E), 1000)
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. delete-one on the device ---------------------------------------------------------------------------------------------
def test_delete_one_on_the_device(ws):
    """The test that does not depend on the reference's formula: F of the cloud without j, by the device, against sum[j]."""
    c = _ctx(ws)
    try:
        rows = _cloud_rows()
        gpc, args = blend_ref.device_scene(ws, rows, VIEW)
        f = _Frame(ws, c, gpc, args)
        try:
            frame, _, ok, _ = _cloud_ref(f)
            mask = ok.astype(F)
            q, m, base = f.removal(weight=mask, base=True)
            ref = removal_ref.removal_f64(frame, VIEW[0], VIEW[1], f.n, BG, E=mask)
            tol_sum, _ = removal_ref.bounds(ref)
            nz = np.nonzero(q > 0)[0]
            rng = np.random.default_rng(23)
            picks = [int(nz[np.argmax(q[nz])]), int(nz[np.argmin(q[nz])])] + [int(j) for j in rng.choice(nz, 3, replace=False)]
            for j in picks:
                sub = f.pc.subset(np.delete(np.arange(f.n, dtype=np.uint32), j))
                r = ws.GaussianRenderer(c, "rgba32float", 3, False)
                acc = ws.Contrib(c, f.n - 1)
                try:
                    r.enable_contrib(True)
                    r.prepare(sub, args)
                    r.accumulate_removal(sub, acc, background=BG, base=True)
                    without = r.download_removal_base()
                finally:
                    acc.close()
                    r.close()
                    sub.close()
                dF = without[..., :3].astype(np.float64) - base[..., :3].astype(np.float64)
                brute = float(((dF * dF).mean(axis=-1) * ok).sum())
                # the rounding of the two base planes, 2 (L + 2) 2^-24 cmax per pixel, through the square -- with the float64
                # change of the pixel for its magnitude, and only where j is: elsewhere both planes run the same arithmetic
                dF_ref = removal_ref.base_f64(frame, VIEW[0], VIEW[1], BG, skip=j)["F"] - ref["F"]
                eps = 2.0 * (ref["L"] + 2) * 2.0 ** -24 * ref["cmax"]
                touched = np.abs(dF_ref).max(axis=-1) > 0
                planes = float((((2.0 * np.abs(dF_ref) + eps[..., None]) * eps[..., None]).mean(axis=-1) * ok * touched).sum())
                got = q[j] / SCALE
                row = dict(case=f"3-delete-{j}", sum=got, brute=brute, diff=abs(got - brute), allowance=float(tol_sum[j] + planes),
                           reference=float(ref["sum"][j]))
                REPORT.append(row)
                print(json.dumps(row))
                assert np.array_equal(_u32(without[~touched]), _u32(base[~touched])), "a pixel j does not reach changed"
                assert abs(got - brute) <= tol_sum[j] + planes, j
        finally:
            f.close()
    finally:
        c.close()


# ---- 4. saturation -------------------------------------------------------------------------------------------------------------
def test_saturating_stack(ws):
    """The opaque 32 x 32 stack with k = 513: every quadrant saturates after a few layers and the walk and the batch loop take
    their early exits.  A wave looks at its pixels' T after every fourth record, so at most three records behind the first one
    whose pixels are all below T_MIN are still walked -- one more for the gap between the device's f32 T and the reference's --
    and they score 0 by the Tb >= 2^-14 rule anyway: everything from the eighth on is exactly 0."""
    c = _ctx(ws, bin_request=0)
    try:
        f = _stack_frame(ws, c, 513, 0.9)
        try:
            frame = f.frame()
            q, m, base = f.removal(base=True)
            ref = removal_ref.removal_f64(frame, 32, 32, 513, BG, saturating=True)
            assert int(ref["und"].sum()) == 0
            row = _compare("4-saturating-513", q, m, ref)
            _compare_base(row, base, ref, saturating=True)
            # Tb per layer at the pixel that saturates last: layer i is in front of T = prod (1 - b)
            T = np.ones((32, 32))
            first = None
            for i, (j, blk, a, keep, und, alpha) in enumerate(weight_ref.records(frame, 32, 32)):
                assert j == i and keep.all()
                if first is None and T.max() < 2.0 ** -14:
                    first = i
                T[blk] -= weight_ref.weights(a, keep, alpha, T[blk])
            print(f"first all-saturated layer {first}; non-zero sums {int((q > 0).sum())}, the last at {int(np.nonzero(q)[0].max())}")
            # (the last layers in front of it are alive at the corners only, with weights whose d * d truncates to 0 on the q32 grid)
            assert first is not None and first + 8 < 513 and np.all(q[:first // 2] > 0)
            assert not q[first + 8:].any() and not _u32(m)[first + 8:].any()
            q2, m2, base2 = f.removal(base=True)
            assert np.array_equal(q, q2) and np.array_equal(_u32(m), _u32(m2)) and np.array_equal(_u32(base), _u32(base2))
        finally:
            f.close()
    finally:
        c.close()


# ---- 5. exact properties -------------------------------------------------------------------------------------------------------
def _mask(width, height, rect, dots):
    a = np.zeros((height, width), F)
    x0, x1, y0, y1 = rect
    a[y0:y1, x0:x1] = 1
    for x, y in dots:
        assert a[y, x] == 0
        a[y, x] = 1
    return a


def _check_exact(f, width, height, mask):
    q, m = f.removal()
    anything = np.random.default_rng(1).uniform(-1e6, 1e6, size=(height, width)).astype(F)
    for name, plane, scale, bias in (("ones", np.ones((height, width), F), 1.0, 0.0), ("threes clamped", np.full((height, width), 3.0, F), 1.0, 0.0),
                                     ("anything, scale 0 bias 1", anything, 0.0, 1.0)):
        qw, mw = f.removal(weight=plane, weight_scale=scale, weight_bias=bias)
        assert np.array_equal(qw, q) and np.array_equal(_u32(mw), _u32(m)), name
    qa, ma = f.removal(weight=mask)
    qb, mb = f.removal(weight=F(1.0) - mask)
    print(f"non-zero {int((q > 0).sum())} in A {int((qa > 0).sum())} in B {int((qb > 0).sum())} in both {int(((qa > 0) & (qb > 0)).sum())}")
    assert ((qa > 0) & (qb > 0)).any() and (qa > 0).any() and (qb > 0).any()
    assert np.array_equal(qa + qb, q)
    assert np.array_equal(np.maximum(_u32(ma), _u32(mb)), _u32(m))
    return q


def test_unit_plane_and_partition_are_exact_general_cloud(ws):
    c = _ctx(ws)
    try:
        f = _cloud_frame(ws, c)
        try:
            q = _check_exact(f, *VIEW, _mask(*VIEW, (13, 211, 9, 150), [(300, 200), (250, 3), (5, 233), (317, 239), (0, 0)]))
            assert (q > 0).sum() > 1000
        finally:
            f.close()
    finally:
        c.close()


def test_unit_plane_and_partition_are_exact_saturating_stack(ws):
    c = _ctx(ws, bin_request=0)
    try:
        f = _stack_frame(ws, c, 513, 0.9)
        try:
            q = _check_exact(f, 32, 32, _mask(32, 32, (3, 21, 5, 14), [(30, 2), (1, 29), (25, 25)]))
            assert (q == 0).any() and (q > 0).any()
        finally:
            f.close()
    finally:
        c.close()


def _orbit_args(ws, gpc, index):
    cj = synth.orbit_cameras(5, VIEW[0], VIEW[1], float(VIEW[0]), float(VIEW[0]))[index]
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, cj.width, cj.height)
    cam.fit_near_far(gpc.aabb)
    return ws.SplattingArgs(camera=cam, viewport=VIEW, max_sh_deg=3)


def test_zero_plane_merging_and_other_accumulators(ws):
    c = _ctx(ws)
    try:
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(_cloud_rows(), 3)
        pc = ws.PointCloud(c, gpc)
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        zero, a1, ab, b_only, plain, plain_again = (ws.Contrib(c, n) for _ in range(6))
        try:
            r.enable_contrib(True)
            r.prepare(pc, _orbit_args(ws, gpc, 0))
            # an all-zero plane adds nothing but counts as a frame
            r.accumulate_removal(pc, zero, background=BG, weight=np.zeros((VIEW[1], VIEW[0]), F))
            r.accumulate_removal(pc, zero, background=BG, weight=np.ones((VIEW[1], VIEW[0]), F), weight_scale=-1.0)
            _, qz, mz = zero.download()
            assert zero.frames == 2 and not qz.any() and not _u32(mz).any()
            # the plain contribution sums of the frame do not see a removal call into another accumulator
            r.accumulate_contrib(pc, plain)
            _, qp, mp = plain.download()
            for acc in (a1, ab):
                r.accumulate_removal(pc, acc, background=BG, kind="abs")
            r.accumulate_contrib(pc, plain_again)
            _, qp2, mp2 = plain_again.download()
            _, qp1, mp1 = plain.download()
            assert (qp > 0).sum() > 1000 and np.array_equal(qp, qp2) and np.array_equal(_u32(mp), _u32(mp2))
            assert np.array_equal(qp, qp1) and np.array_equal(_u32(mp), _u32(mp1)) and plain.frames == 1
            # two frames into one accumulator == the merge of two accumulators
            r.prepare(pc, _orbit_args(ws, gpc, 2))
            for acc in (ab, b_only):
                r.accumulate_removal(pc, acc, background=BG, kind="abs")
            _, q1, m1 = a1.download()
            _, qab, mab = ab.download()
            _, qb, mb = b_only.download()
            assert ab.frames == 2 and (q1 > 0).sum() > 1000 and not np.array_equal(qb, q1)
            a1.add(qb, mb)
            _, qsum, msum = a1.download()
            assert np.array_equal(qsum, qab) and np.array_equal(_u32(msum), _u32(mab))
            assert np.array_equal(qab, q1 + qb) and np.array_equal(mab, np.maximum(m1, mb))
            assert r.frame_stats()["overflow"] == 0
        finally:
            for a in (zero, a1, ab, b_only, plain, plain_again):
                a.close()
            r.close()
            pc.close()
    finally:
        c.close()


# ---- 6. the question the contribution sum cannot answer ------------------------------------------------------------------------
def test_a_decoy_in_front_of_a_wall_of_its_colour(ws):
    """Eight layers at 0.99 over the whole 64 x 64 view, all of one colour; in front of them two Gaussians of one shape and
    opacity side by side, one of the wall's colour, one of another.  They draw the same; deleting the first changes nothing."""
    c = _ctx(ws, bin_request=0)
    try:
        layers = 8
        wall_dc, other_dc = np.array([0.6, -0.4, 0.2], F), np.array([-1.2, 1.4, -0.9], F)
        z = np.concatenate([[-0.5, -0.5], np.linspace(0.0, 0.4, layers)]).astype(F)
        x = np.concatenate([[-0.14, 0.14], np.zeros(layers)]).astype(F)
        xyz = np.stack([x, np.zeros_like(x), z], axis=1)
        f_dc = np.tile(wall_dc, (layers + 2, 1))
        f_dc[1] = other_dc
        log_scale = np.full((layers + 2, 3), np.log(4.0), F)     # the wall: so wide that the view sees its flat top
        log_scale[:2] = np.log(0.03)
        op = np.concatenate([[0.5, 0.5], np.full(layers, 1.0 - 1e-6)])
        rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], F), (layers + 2, 1))
        rows = synth._rows(xyz, f_dc, np.zeros((layers + 2, 45), F), np.log(op / (1.0 - op)).astype(F), log_scale, rot)
        f = _Frame(ws, c, *blend_ref.device_scene(ws, rows, (64, 64)))
        try:
            qc, _ = f.plain()
            q, m = f.removal(background=(0.0, 0.0, 0.0))
            drew, effect = qc.astype(np.float64) / SCALE, q.astype(np.float64) / SCALE
            print(f"decoy: drew {drew[0]:.4f} effect {effect[0]:.3e}; the other: drew {drew[1]:.4f} effect {effect[1]:.3e}")
            assert drew[0] > 5 and abs(drew[0] - drew[1]) <= 0.01 * drew[1]
            assert effect[1] > 0.1 and effect[0] < 1e-3 * effect[1]
        finally:
            f.close()
    finally:
        c.close()


# ---- 7. the scene driver, the tool -------------------------------------------------------------------------------------------
SMALL = (160, 120)


def test_scene_driver_equals_the_manual_loop_and_the_tool_lists_it(ws, tmp_path):
    c = _ctx(ws)
    try:
        ply, cj = tmp_path / "cloud.ply", tmp_path / "cameras.json"
        synth.write_ply(str(ply), synth.scene_c1(n=10_000, seed=0))
        pc = ws.PointCloud.load(c, str(ply))   # (the tool's own loader)
        n = pc.num_points()
        cams = synth.orbit_cameras(3, SMALL[0], SMALL[1], 150.0, 150.0, radius=3.0, height_off=0.4)
        text = json.dumps([cj.to_json() for cj in cams])
        scene = ws.Scene.from_json_text(text)
        accs = [ws.Contrib(c, n) for _ in range(5)]
        effect, weight, alone, m_effect, m_weight = accs
        r = ws.GaussianRenderer(c, "rgba16float", pc.sh_deg(), False)
        try:
            assert ws.accumulate_removal_scene(c, pc, scene, "test", effect, weight) + ws.accumulate_removal_scene(c, pc, scene, "train", effect, weight) == 3
            assert ws.accumulate_removal_scene(c, pc, scene, "test", alone) + ws.accumulate_removal_scene(c, pc, scene, "train", alone) == 3
            bg = pc.background_color() or (0.0, 0.0, 0.0)
            r.enable_contrib(True)
            for cam in scene.cameras(None):   # the frames of ws_render_views: ws_scene_accumulate_contrib's set-up
                pcam = cam.to_perspective().fit_near_far(pc.bbox())
                r.prepare(pc, ws.SplattingArgs(camera=pcam, viewport=SMALL, max_sh_deg=pc.sh_deg(), walltime=100.0))
                r.accumulate_removal(pc, m_effect, background=bg)
                r.accumulate_contrib(pc, m_weight)
            assert r.errors()[0] == 0
            (_, qe, me), (_, qw, mw), (_, qa, ma) = effect.download(), weight.download(), alone.download()
            (_, qme, mme), (_, qmw, mmw) = m_effect.download(), m_weight.download()
            assert effect.frames == 3 and weight.frames == 3 and (qe > 0).sum() > 1000
            assert np.array_equal(qe, qme) and np.array_equal(_u32(me), _u32(mme))
            assert np.array_equal(qw, qmw) and np.array_equal(_u32(mw), _u32(mmw))
            assert np.array_equal(qa, qe) and np.array_equal(_u32(ma), _u32(me))
            # the tool: the same three indices, and the count of drawn Gaussians with no effect at all
            cj.write_text(text)
            exe = os.path.join(os.path.dirname(os.path.dirname(L.LIB_PATH)), "bin", "websplat_evaluate")
            listed = {}
            for split in ("test", "train"):
                out = subprocess.run([exe, str(ply), str(cj), "--removal", "3", "--split", split], capture_output=True, text=True, timeout=120)
                assert out.returncode == 0, out.stderr
                lines = out.stdout.splitlines()
                head = [i for i, ln in enumerate(lines) if ln.startswith("removal (sq effect")]
                assert len(head) == 1 and "PSNR" not in out.stdout
                listed[split] = [int(ln.split()[0]) for ln in lines[head[0] + 2:head[0] + 5]]
                assert re.search(r"removal: \d+ of \d+ drawn Gaussians have an effect of exactly 0", lines[-1])
            per_split = {}
            for split in ("test", "train"):
                acc = ws.Contrib(c, n)
                try:
                    ws.accumulate_removal_scene(c, pc, scene, split, acc)
                    qs = acc.download()[1]
                finally:
                    acc.close()
                per_split[split] = sorted(range(n), key=lambda i: (-int(qs[i]), i))[:3]
            assert listed == per_split
        finally:
            for a in accs:
                a.close()
            r.close()
            scene.close()
            pc.close()
    finally:
        c.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_error_cases_and_padded_pitches(ws):
    c = _ctx(ws)
    cut = _ctx(ws, debug_cut=2)
    try:
        gpc, args = blend_ref.device_scene(ws, _cloud_rows(), VIEW)
        pc, pc_cut = ws.PointCloud(c, gpc), ws.PointCloud(cut, gpc)
        n = pc.num_points()
        w, h = VIEW
        r, r_cut = ws.GaussianRenderer(c, "rgba32float", 3, False), ws.GaussianRenderer(cut, "rgba32float", 3, False)
        acc, small, acc_cut = ws.Contrib(c, n), ws.Contrib(c, n - 1), ws.Contrib(cut, n)
        pad = 5
        d_base = c.malloc((w + pad) * h * 16)

        def code_of(fn):
            with pytest.raises(ws.WebSplatError) as e:
                fn()
            assert "ws_renderer_accumulate_removal" in str(e.value)
            return e.value.code

        try:
            # not prepared; prepared without contributions; another size; DSSIM; debug_cut
            r.enable_contrib(True)
            assert code_of(lambda: r.accumulate_removal(pc, acc)) == L.WS_ERR_STATE
            r.enable_contrib(False)
            r.prepare(pc, args)
            assert code_of(lambda: r.accumulate_removal(pc, acc)) == L.WS_ERR_STATE
            r.enable_contrib(True)
            r.prepare(pc, args)
            assert code_of(lambda: r.accumulate_removal(pc, small)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_removal(pc, acc, kind="dssim")) == L.WS_ERR_INVALID
            r_cut.enable_contrib(True)
            r_cut.prepare(pc_cut, args)
            assert code_of(lambda: r_cut.accumulate_removal(pc_cut, acc_cut)) == L.WS_ERR_UNSUPPORTED
            # pitches below the row
            assert code_of(lambda: r.accumulate_removal(pc, acc, base_ptr=d_base, base_pitch=(w - 1) * 16)) == L.WS_ERR_INVALID
            assert code_of(lambda: r.accumulate_removal(pc, acc, weight=d_base, weight_pitch=(w - 1) * 4)) == L.WS_ERR_INVALID
            assert acc.frames == 0
            # padded rows are honoured: NaN behind the weight plane's rows is never read, a sentinel behind the base's never written
            rng = np.random.default_rng(5)
            plane = rng.uniform(-0.5, 1.5, size=(h, w)).astype(F)
            padded = np.full((h, w + 13), np.nan, F)
            padded[:, :w] = plane
            r.accumulate_removal(pc, acc, background=BG, weight=plane, base=True)
            want_base = r.download_removal_base()
            _, want_q, want_m = acc.download()
            assert (want_q > 0).sum() > 1000
            acc.reset()
            sentinel = np.full((h, w + pad, 4), -7.5, F)
            c.upload(d_base, sentinel)
            r.accumulate_removal(pc, acc, background=BG, weight=padded, base_ptr=d_base, base_pitch=(w + pad) * 16)
            _, q, m = acc.download()
            got = c.download(d_base, (h, w + pad, 4), F)
            assert np.array_equal(q, want_q) and np.array_equal(_u32(m), _u32(want_m))
            assert np.array_equal(_u32(got[:, :w]), _u32(want_base)) and np.all(got[:, w:] == F(-7.5))
        finally:
            c.sync()
            c.free(d_base)
            for a in (acc, small, acc_cut):
                a.close()
            r.close()
            r_cut.close()
            pc.close()
            pc_cut.close()
    finally:
        cut.close()
        c.close()


# ---- 9. no pixel changes -----------------------------------------------------------------------------------------------------
def test_removal_call_changes_no_pixel(ws, oracle):
    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=VIEW)
        pc = ws.PointCloud(c, sc.gpc)
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        acc = ws.Contrib(c, pc.num_points())
        try:
            r.enable_contrib(True)
            r.prepare(pc, sc.args)
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            before = r.download_target().copy()
            r.accumulate_removal(pc, acc, background=BG, weight=_ramp_checker(*VIEW), base=True)
            r.render(pc, background=(0.1, 0.2, 0.3, 0.4))
            after = r.download_target().copy()
            assert (before[..., 3] > 0.5).mean() > 0.05
            assert np.array_equal(_u32(before), _u32(after))
            assert acc.frames == 1 and (acc.download()[1] > 0).sum() > 1000
        finally:
            acc.close()
            r.close()
            pc.close()
    finally:
        c.close()
