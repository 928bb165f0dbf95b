"""CPU tests of the geometry gradient's chain (include/websplat.h "Geometry gradients"; tests/geometry_ref.py).

   1. the analytic position and covariance gradients against central differences of a float64 forward, in each of the 9 parameters
   2. four defective chains each fail that check                     4. ws_geom_spread_rows against spread_f64
   3. a Gaussian on K1's lambda2 clamp has covariance sums of 0       5. the p0, p1 error term of bounds() against ws_debug_stage_splat

   6. stage_a_f64 on oracle frames (blend_ref.oracle_frame: no device), the frames of geometry_frames.py: the cap rule leaves the
      uncapped cases' sums and bounds where they were; the general anisotropic cloud at 96 x 72 has bounds that say something; each
      stage-A mutant is told from the right walk on the frame meant for it; the clamped core; the cap frame is exact

The finite differences.  A cloud of 12 Gaussians of SH degree 0 (the colour does not depend on the position), mip off, walltime far
past the fade-in, under two cameras on a 64 x 48 viewport; L = sum G . F + G_T T_end for gradient_frames.signed_ramp.  Central
differences at a relative step of 1e-6 leave about 1e-10 of the gradient (truncation h^2, rounding 1e-16 |L| / h); the bound is 1e-5
of the Gaussian's gradient norm (position and covariance each against their own norm), the margin covering conditioning.  The
cloud is chosen so that no pair's kept verdict and no pair's clamp verdict differs between -h and +h: asserted for every step."""
import ctypes as C
import functools
import os
import time

import numpy as np

import blend_ref
import geometry_frames as gf
import geometry_ref as ref
import gradient_ref
import k1_edges
import oracle_lib as oracle
import removal_ref
from attrib_frames import _stack
from gradient_frames import signed_ramp
from websplat import synth

VIEW = (64, 48)
N = 12
BG = (0.25, 0.5, 0.75)
KERNEL_SIZE = 0.05            # below K1's 0.1: a needle's minor axis lands on the clamp
CLAMPED = 11                  # the needle
REL_STEP = 1e-6
BOUND = 1e-5
BBOX = ((-4.0, -4.0, -1.0), (4.0, 4.0, 9.0))


def _cloud():
    rng = np.random.default_rng(2024)
    xyz = np.stack([rng.uniform(-0.9, 0.9, N), rng.uniform(-0.6, 0.6, N), rng.uniform(3.4, 4.6, N)], axis=1)
    cov6 = np.empty((N, 6))
    for i in range(N):
        a = rng.normal(size=(3, 3))
        q, _ = np.linalg.qr(a)
        s = rng.uniform(0.12, 0.4, 3) ** 2
        c = (q * s) @ q.T
        cov6[i] = c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]
    cov6[CLAMPED] = (0.09, 0.0, 0.0, 1e-8, 0.0, 1e-8)       # 4.8 px by a hair, axis-aligned: lambda2_raw = kernel size + ~0
    xyz[CLAMPED] = (0.1, -0.05, 4.0)
    opacity = rng.uniform(0.2, 0.6, N)
    sh = np.zeros((N, 16, 3))
    sh[:, 0, :] = rng.uniform(-1.0, 1.5, (N, 3))
    return xyz, opacity, cov6, sh


def _uniforms(ws, which):
    w, h = VIEW
    if which == 0:
        cj = synth.SceneCamera(0, "axis", w, h, [0.0, 0.0, 0.0], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], float(w), float(w))
    else:
        cj = synth.look_at_camera(1, [1.6, -1.1, 0.4], [0.0, 0.0, 4.0], w, h, float(w), float(w))
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
    cam.znear, cam.zfar = 0.5, 16.0
    cu = oracle.copy_struct(oracle.CameraUniform, cam.uniform(VIEW))
    rs = oracle.settings_uniform(oracle.make_aabb(*BBOX), [0.0, 0.0, 4.0], max_sh_deg=0, mip_splatting=False, kernel_size=KERNEL_SIZE,
                                 walltime=100.0)
    return cu, rs, k1_edges.uniforms_f64(cu, rs)


@functools.lru_cache(maxsize=None)
def _case(which):
    """(cloud, u, analytic gradients, finite differences [N, 9]) under camera `which`, computed once."""
    import websplat as ws
    xyz, opacity, cov6, sh = _cloud()
    _, _, u = _uniforms(ws, which)
    G = signed_ramp(*VIEW).astype(np.float64)
    ana = ref.analytic_from_cloud(xyz, opacity, cov6, sh, u, *VIEW, G, BG)
    assert not ana["culled"].any(), "every Gaussian of the cloud is in view"
    base = ref.forward_from_cloud(xyz, opacity, cov6, sh, u, *VIEW, G, BG)
    assert np.array_equal(base["order"], ana["order"])
    assert base["T_end"].min() > 2.0 ** -10 and not base["clamped"].any() and base["kept"].reshape(N, -1).sum(axis=1).min() >= 12
    fd = np.zeros((N, 9))
    for i in range(N):
        for k in range(9):
            L = []
            for sign in (-1.0, 1.0):
                p, c = xyz.copy(), cov6.copy()
                if k < 3:
                    p[i, k] += sign * REL_STEP * 4.0
                    h = REL_STEP * 4.0
                else:
                    h = REL_STEP * (cov6[i, 0] + cov6[i, 3] + cov6[i, 5])
                    c[i, k - 3] += sign * h
                got = ref.forward_from_cloud(p, opacity, c, sh, u, *VIEW, G, BG, order=base["order"])
                assert np.array_equal(got["kept"], base["kept"]) and np.array_equal(got["clamped"], base["clamped"]), \
                    f"Gaussian {i}, parameter {k}: a pair's verdict changes within the step"
                L.append(got["L"])
            fd[i, k] = (L[1] - L[0]) / (2.0 * h)
    return (xyz, opacity, cov6, sh), u, ana, fd


def _deviation(chain, fd):
    """Per Gaussian the largest |analytic - finite difference| of the position and of the covariance, each as a fraction of the
    finite differences' norm of that block."""
    dp = np.abs(chain["position"] - fd[:, :3]).max(axis=1) / np.linalg.norm(fd[:, :3], axis=1)
    dc = np.abs(chain["covariance"] - fd[:, 3:]).max(axis=1) / np.linalg.norm(fd[:, 3:], axis=1)
    return dp, dc


FREE = np.array([i for i in range(N) if i != CLAMPED])


def test_analytic_gradients_against_central_differences(ws):
    worst = 0.0
    for which in (0, 1):
        _, _, ana, fd = _case(which)
        assert ana["free"][FREE].all() and not ana["free"][CLAMPED]
        assert (np.linalg.norm(fd[FREE, :3], axis=1) > 1e-3).all() and (np.linalg.norm(fd[FREE, 3:], axis=1) > 1e-2).all()
        dp, dc = _deviation(ana, fd)
        print(f"camera {which}: largest deviation, position {dp[FREE].max():.2e}, covariance {dc[FREE].max():.2e} of the gradient norm")
        assert (dp[FREE] <= BOUND).all() and (dc[FREE] <= BOUND).all(), (dp, dc)
        worst = max(worst, float(dp[FREE].max()), float(dc[FREE].max()))
    print(f"largest deviation over both cameras: {worst:.2e} (bound {BOUND:.0e})")


def test_defective_chains_fail(ws):
    for mutate in ref.MUTATIONS:
        failed = 0
        for which in (0, 1):
            (xyz, _, cov6, _), u, ana, fd = _case(which)
            I = ref.records_from_cloud(*_cloud(), u, *VIEW)["I"]
            bad = ref.chain_f64(ana["m"], ana["S"], I, xyz, cov6, u, *VIEW, mutate=mutate)
            dp, dc = _deviation(bad, fd)
            failed += int(((dp[FREE] > BOUND) | (dc[FREE] > BOUND)).sum())
        print(f"{mutate}: fails on {failed} of {2 * len(FREE)} Gaussians")
        assert failed >= 1, mutate


def test_lambda2_clamp_has_no_covariance_sums(ws):
    for which in (0, 1):
        _, _, ana, fd = _case(which)
        assert ana["lambda2_raw"][CLAMPED] < ref.C_0P1 and (ana["lambda2_raw"][FREE] > 0.5).all()
        assert not ana["covariance"][CLAMPED].any() and np.abs(ana["m"][CLAMPED]).max() > 0 and np.abs(ana["position"][CLAMPED]).max() > 0
        assert (ana["covariance"][FREE] != 0).all()


def _rows(ws, which, seed):
    """Random rows for the twin: plausible records, positions in view, covariances as f16, sums up to 2^40; rows 3 and 17 all zero."""
    rng = np.random.default_rng(seed)
    n = 40
    cu, rs, u = _uniforms(ws, which)
    xyz = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.6, 0.6, n), rng.uniform(3.4, 4.6, n)], axis=1).astype(np.float32)
    cov = np.empty((n, 6))
    for i in range(n):
        a = rng.normal(size=(3, 3)) * rng.uniform(0.05, 0.4)
        c = a @ a.T
        cov[i] = c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]
    cov[5] = (0.09, 0.0, 0.0, 1e-7, 0.0, 1e-7)                 # on the clamp
    cov_bits = cov.astype(np.float16).view(np.uint16)
    k = k1_edges.k1_f64(xyz.astype(np.float64), np.full(n, 0.5), cov_bits.view(np.float16).astype(np.float64), np.zeros((n, 16, 3)), u)
    vp = np.array(VIEW, np.float64)
    rec_bits = np.concatenate([k["v1"] / vp, k["v2"] / vp], axis=1).astype(np.float16).view(np.uint16)
    q5 = rng.integers(-2 ** 40, 2 ** 40, size=(n, 5), dtype=np.int64)
    q5[[3, 17]] = 0
    q5[9, 1:] = 0                                             # one sum alone keeps a row alive
    return q5, rec_bits, xyz, cov_bits, cu, rs, u, k


def test_host_twin_equals_spread_f64(ws):
    from websplat import _lib as L
    for which, scale in ((0, 1.0), (1, 0.125), (1, 3.0)):
        q5, rec_bits, xyz, cov_bits, cu, rs, u, k = _rows(ws, which, 7 + which)
        got = ws.geom_spread_rows(q5, rec_bits, xyz, cov_bits, oracle.copy_struct(L.ws_camera_uniform, cu),
                                  oracle.copy_struct(L.ws_settings_uniform, rs), geometry_scale=scale)
        want = ref.spread_f64(q5, rec_bits, xyz, cov_bits, u, *VIEW, geometry_scale=scale)
        assert np.array_equal(got["seen"], want["seen"]) and got["seen"].sum() == len(q5) - 2 and got["seen"].dtype == np.uint64
        assert k["lambda2_raw"][5] < ref.C_0P1 and not got["covariance"][5].any() and got["position"][5].any()
        for key in ("position", "covariance", "screen_norm"):
            g, w = got[key].reshape(len(q5), -1), want[key].reshape(len(q5), -1)
            assert np.isfinite(g).all()
            size = np.abs(w).max(axis=1, keepdims=True)
            assert (np.abs(g - w) <= 1e-12 * size).all(), (key, float((np.abs(g - w) / np.maximum(size, 1e-300)).max()))
            assert (size[got["seen"] == 1] > 0).all() or key == "covariance"
        assert not got["position"][[3, 17]].any() and not got["screen_norm"][[3, 17]].any()
        # the twin ADDS: a second call doubles every sum exactly
        again = {k2: v.copy() for k2, v in got.items()}
        rc = ws.lib.ws_geom_spread_rows(q5.ctypes.data_as(C.POINTER(C.c_int64)), rec_bits.ctypes.data_as(L._u16p), xyz.ctypes.data_as(L._f32p),
                                        cov_bits.ctypes.data_as(L._u16p), C.byref(oracle.copy_struct(L.ws_camera_uniform, cu)),
                                        C.byref(oracle.copy_struct(L.ws_settings_uniform, rs)), scale, len(q5),
                                        again["position"].ctypes.data_as(L._f64p), again["covariance"].ctypes.data_as(L._f64p),
                                        again["screen_norm"].ctypes.data_as(L._f64p), again["seen"].ctypes.data_as(L._u64p))
        assert rc == L.WS_OK
        assert all(np.array_equal(again[k2], 2 * got[k2]) for k2 in got)


def test_p_error_bound_against_the_host_decode(ws):
    """bounds()' e_p0, e_p1: the staged record ws_debug_stage_splat makes in f32 (decode's own code, compiled for the host), taken
    through the walk's two fused multiply-adds in float64, against the float64 p of the same halves."""
    rng = np.random.default_rng(11)
    W, H = 640.0, 480.0
    worst = 0.0
    for trial in range(400):
        ang = rng.uniform(0, np.pi)
        s1, s2 = np.exp(rng.uniform(np.log(0.6), np.log(120.0), 2))          # axes of 0.6 .. 120 px
        e = np.array([np.cos(ang), np.sin(ang)])
        v1, v2 = s1 * e, s2 * np.array([e[1], -e[0]])
        centre = rng.uniform(-1.1, 1.1, 2)
        halves = np.array([v1[0] / W, v1[1] / H, v2[0] / W, v2[1] / H, centre[0], centre[1], 0.5, 0.5, 0.5, 0.5], np.float16)
        words = halves.view(np.uint32)
        tile = (32.0 * rng.integers(0, 20), 32.0 * rng.integers(0, 15))
        rec, _ = ws.stage_splat(words, (W, H), tile, (32, 32))
        r = rec.astype(np.float64)
        I, (cx, cy) = ref._iprime(halves.astype(np.float64), W, H)
        lx = np.arange(32)[None, :] + 0.5
        ly = np.arange(32)[:, None] + 0.5
        got = (r[0] * lx + r[1] * ly + r[2], r[3] * lx + r[4] * ly + r[5])
        dx, dy = tile[0] + lx - cx, tile[1] + ly - cy
        want = (I[0, 0] * dx + I[0, 1] * dy, I[1, 0] * dx + I[1, 1] * dy)
        err = ref.p_error(I, dx, dy, cx, cy, W, H)
        for k in range(2):
            frac = np.abs(got[k] - want[k]) / err[k]
            worst = max(worst, float(frac.max()))
    print(f"largest |p(f32 record) - p(f64)| as a fraction of e_p: {worst:.3f}")
    assert worst <= 1.0


# ---- 6. stage_a_f64 on oracle frames: the cap rule, the general cloud, the mutants ------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_stage_a_uncapped.npz")
UNCAPPED = {"tile": (24, 0.03, 8.0, False), "long": (513, 0.002, 64.0, False), "saturating": (513, 0.9, 1.0 / 128, True)}


def test_cap_rule_leaves_the_uncapped_cases_where_they_were():
    """The stacks of test_gpu_geometry's existing cases (one tile of 24 layers, the 513-entry list, the saturating stack) on oracle
    frames: sum and tol as stage_a_f64 gave them before it knew of the cap (golden/geometry_stage_a_uncapped.npz, recorded with
    that version; 1e-12 relative, for a libm that rounds exp differently -- on the recording machine the arrays are equal)."""
    gold = np.load(GOLDEN)
    for name, (k, opacity, s, sat) in UNCAPPED.items():
        frame = blend_ref.oracle_frame(oracle, _stack(k, opacity), gf.TILE)
        base = removal_ref.base_f64(frame, 32, 32, BG)
        ok = (base["und"] == 0) if sat else ~removal_ref.undecided_mask(base)
        g = (signed_ramp(32, 32) * ok[..., None]).astype(np.float32)
        got = ref.stage_a_f64(frame, 32, 32, k, gradient_ref.plane_G(g), BG, geometry_scale=s, saturating=sat)
        assert not got["capped"].any() and not got["straddling"].any() and not got["net"].any()
        assert np.array_equal(got["counted"] > 0, (got["sum"] != 0).any(axis=1)) and got["open_px"].any()
        for key in ("sum", "tol"):
            want = gold[f"{name}_{key}"]
            assert np.abs(want).max() > 0 and np.allclose(got[key], want, rtol=1e-12, atol=0), (name, key)


@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    """(frame, n, view, plane, plane scale, geometry_scale, reference) of one of geometry_frames' frames, computed once."""
    if name == "general":
        rows, view, s, ps = gf.general_rows(), gf.GENERAL_VIEW, gf.GENERAL_S, gf.GENERAL_PLANE_SCALE
    elif name.startswith("clamped"):
        rows, view, s, ps = gf.clamped_rows(), gf.TILE, gf.CLAMPED_S[int(name[-1])], 1.0
    else:
        rows, view, s, ps = gf.cap_rows(), gf.TILE, gf.CAP_S, 1.0
    frame = blend_ref.oracle_frame(oracle, rows, view)
    g, share = gf.masked_ramp(frame, view, gf.MASK_CAP_GENERAL)
    t0 = time.perf_counter()
    want = gf.stage_a(frame, view, len(rows), g, s, ps)
    print(f"{name}: {len(frame['src_index'])} visible of {len(rows)}, {100 * share:.2f} % of the pixels masked, reference in {time.perf_counter() - t0:.2f} s")
    return frame, len(rows), view, g, ps, s, want


def test_general_frame_has_bounds_that_say_something():
    frame, n, view, g, ps, s, want = _oracle_case("general")
    tol = ref.bounds(want)
    drawn = want["pairs"] > 0
    halves = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)[: len(frame["src_index"])]
    cx, cy = (halves[:, 4] * 0.5 + 0.5) * view[0], (0.5 - halves[:, 5] * 0.5) * view[1]
    outside = (cx < 0) | (cx > view[0]) | (cy < 0) | (cy > view[1])
    nz = np.abs(want["sum"]) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        over = [float(np.median((tol[:, k] / np.abs(want["sum"][:, k]))[nz[:, k]])) for k in range(5)]
    big = (np.abs(want["sum"]) > 4 * tol)[drawn].mean(axis=0)
    print(f"general: {int(drawn.sum())} Gaussians with pairs, {int(outside.sum())} centres outside the viewport ({int((cx < 0).sum())} left, "
          f"{int((cx > view[0]).sum())} right), band {int(want['band'].sum())}, clamped {int(want['clamped'].sum())}, T_end >= {want['T'].min():.3f}, "
          f"median bound / value {['%.2e' % v for v in over]}, |sum| > 4 tol {np.round(big, 3).tolist()}")
    assert n - len(frame["src_index"]) > 2000 and drawn.sum() >= 500
    assert (cx < 0).sum() >= 10 and (cx > view[0]).sum() >= 10 and (cy < 0).sum() >= 10 and (cy > view[1]).sum() >= 10
    assert int(want["U"].sum()) == 0 and int(want["band"].sum()) == 0 and int(want["clamped"].sum()) == 0
    assert not want["capped"].any() and not want["straddling"].any()
    assert (big > 0.9).all(), big


def test_each_stage_a_mutant_is_told_apart():
    """Under every mutant the UNMUTATED float64 sums lie outside the mutant's bounds (in at least one of the five channels) for at
    least half of the Gaussians it can touch.  clamped_pairs_counted: under the plane of geometry_frames.clamped_corner -- under
    the whole signed ramp the twelve clamped pairs move layer 0's sums by 0.35 to 0.54 of the bound (S01: 0.001), see there."""
    shares = {}
    frame, n, view, g, ps, s, want = _oracle_case("general")
    for m in gf.GENERAL_MUTANTS:
        wrong = gf.stage_a(frame, view, n, g, s, ps, mutate=m)
        shares[m], count, outside = gf.told_apart(want["sum"], wrong)
        print(f"{m}: {100 * shares[m]:.1f} % of {count} Gaussians out of bounds; per channel {np.round(outside[wrong['pairs'] > 0].mean(axis=0), 3).tolist()}")
        assert count >= 500
    for i, s in enumerate(gf.CLAMPED_S):
        frame, n, view, g, ps, _, whole = _oracle_case(f"clamped{i}")
        wrong = gf.stage_a(frame, view, n, g, s, mutate="clamped_pairs_counted")
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"clamped core, whole ramp, geometry_scale {s}: layer 0 moves by {np.round(np.abs(whole['sum'] - wrong['sum'])[0] / ref.bounds(wrong)[0], 4).tolist()} of the bound")
        corner = gf.clamped_corner(frame, view)
        gc = (signed_ramp(*view) * corner[..., None]).astype(np.float32)
        right, wrong = gf.stage_a(frame, view, n, gc, s), gf.stage_a(frame, view, n, gc, s, mutate="clamped_pairs_counted")
        touched = right["clamped"] > 0
        assert corner.sum() >= 2 and int(right["pairs"][0]) == int(corner.sum()) and int(right["counted"][0]) == 0 and int(right["band"].sum()) == 0
        assert 4 <= right["clamped"][0] <= 16 and not right["clamped"][1:].any()
        assert not right["sum"][0].any() and not ref.bounds(right)[0].any(), "every pair of layer 0 under this plane is clamped: exactly 0"
        share, count, outside = gf.told_apart(right["sum"], wrong, touched=touched)
        print(f"clamped_pairs_counted, corner plane of {int(corner.sum())} pixels, geometry_scale {s}: {100 * share:.0f} % of {count}, channels {outside[0].tolist()}")
        assert count == 1 and outside[0].all()
        shares["clamped_pairs_counted"] = min(share, shares.get("clamped_pairs_counted", 1.0))
    frame, n, view, _, _, s, _ = _oracle_case("cap")
    for plane in (gf.red_plane(*view), gf.masked_ramp(frame, view, gf.MASK_CAP_GENERAL)[0]):
        right, wrong = gf.stage_a(frame, view, n, plane, s), gf.stage_a(frame, view, n, plane, s, mutate="cap_ignored")
        share, count, _ = gf.told_apart(right["sum"], wrong)
        shares["cap_ignored"] = min(share, shares.get("cap_ignored", 1.0))
        assert count == n
    print(shares)
    assert set(shares) == set(ref.STAGE_A_MUTATIONS) and all(v >= 0.5 for v in shares.values()), shares


def test_clamped_core_frame():
    for i, s in enumerate(gf.CLAMPED_S):
        frame, n, view, g, ps, _, want = _oracle_case(f"clamped{i}")
        tol = ref.bounds(want)
        print(f"geometry_scale {s}: clamped pairs per layer {want['clamped'].tolist()}, band {int(want['band'].sum())}, capped {int(want['capped'].sum())}, "
              f"straddling {int(want['straddling'].sum())}, largest bound / value {float((tol / np.abs(want['sum'])).max()):.3e}")
        assert 4 <= want["clamped"][0] <= 16 and not want["clamped"][1:].any()
        assert int(want["band"].sum()) == 0 and int(want["U"].sum()) == 0 and (np.abs(want["sum"]) > 4 * tol).all()
    assert int(_oracle_case("clamped0")[6]["capped"].sum()) == 0 and int(_oracle_case("clamped1")[6]["capped"].sum()) > 0


def test_cap_frame_is_exact():
    """_stack(3, 0.3) under (1, 0, 0, 0) at geometry_scale 2^20: every pair of every layer counts and all five values of every pair
    are decidedly capped, so the sums are integers times 2^-32 -- net (2^32 - 256) -- and the tolerance is exactly 0.  Under the
    signed ramp kappa changes sign inside the view: a pair or two per layer straddle."""
    frame, n, view, _, _, s, ramp = _oracle_case("cap")
    g, want, share = gf.exact_cap_plane(frame, view, n, gf.red_plane(*view))
    assert share == 0.0 and want["counted"].tolist() == [1024] * 3 and (want["capped"] == 1024).all()
    assert not ref.bounds(want).any() and not want["straddling"].any()
    q = want["net"] * ref.Q_CAP
    assert np.array_equal(want["sum"] * 2.0 ** 32, q.astype(np.float64)) and np.array_equal(np.abs(want["net"][:, [2, 4]]), np.full((3, 2), 1024))
    assert ref.Q_CAP == int(ref.V_CAP * 2.0 ** 32) and ref.V_CAP == float(np.float32(ref.V_CAP))
    # the ramp: 1 - 2 straddling pairs in some layer and channel; a straddling pair carries at most 2 V_CAP, a pair that is neither
    # straddling nor capped has |v| + slack < V_CAP, a capped one nothing
    tol = ref.bounds(ramp)
    print(f"cap frame under the ramp: straddling {ramp['straddling'].tolist()}, capped {ramp['capped'].tolist()}, bounds {np.round(tol, 4).tolist()}")
    assert 1 <= ramp["straddling"].max() <= 2 and int(ramp["band"].sum()) == 0 and (ramp["capped"] >= 1020).all()
    loose = ramp["counted"][:, None] - ramp["capped"] - ramp["straddling"]
    assert (loose >= 0).all() and (tol <= ref.V_CAP * (2 * ramp["straddling"] + loose) + 2.0 ** -32 * loose).all() and not tol[(ramp["straddling"] + loose) == 0].any()
    # ... and masked where a pair is open, the ramp's sums are exact too, and not symmetric: m0, m1 and S01 are not 0
    g, want, share = gf.exact_cap_plane(frame, view, n, gf.masked_ramp(frame, view, gf.MASK_CAP_GENERAL)[0])
    assert 0 < share <= gf.MASK_CAP_OPEN and (want["net"] != 0).all() and np.array_equal(want["sum"] * 2.0 ** 32, (want["net"] * ref.Q_CAP).astype(np.float64))
