"""CPU tests of the geometry gradient's chain (include/websplat.h "Geometry gradients"; tests/geometry_ref.py).

   1. the analytic position and covariance gradients against central differences of a float64 forward, in each of the 9 parameters
   2. four defective chains each fail that check                     4. ws_geom_spread_rows against spread_f64
   3. a Gaussian on K1's lambda2 clamp has covariance sums of 0       5. the p0, p1 error term of bounds() against ws_debug_stage_splat

The finite differences.  A cloud of 12 Gaussians of SH degree 0 (the colour does not depend on the position), mip off, walltime far
past the fade-in, under two cameras on a 64 x 48 viewport; L = sum G . F + G_T T_end for gradient_frames.signed_ramp.  Central
differences at a relative step of 1e-6 leave about 1e-10 of the gradient (truncation h^2, rounding 1e-16 |L| / h); the bound is 1e-5
of the Gaussian's gradient norm (position and covariance each against their own norm), the margin covering conditioning.  The
cloud is chosen so that no pair's kept verdict and no pair's clamp verdict differs between -h and +h: asserted for every step."""
import ctypes as C
import functools

import numpy as np

import geometry_ref as ref
import k1_edges
import oracle_lib as oracle
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
