"""CPU tests of the SH gradient and SH refit ABI (include/websplat.h "SH gradients", ws_refit_step_sh): declared, exported, bound,
usable from C99, the new descriptor's layout shared with the Python stub, every descriptor error refused before any handle is looked
at; the basis of tests/sh_refit_ref.py against the oracle's K1; and the reference by itself: against float64, against the host twin
ws_sh_spread_rows bit for bit, and step_sh with lr_sh = 0 against refit_ref.step."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as oracle
import refit_ref
import sh_refit_ref as ref
from websplat import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ws_shgrad_create", "ws_shgrad_destroy", "ws_shgrad_reset", "ws_shgrad_num_points", "ws_shgrad_sh_deg", "ws_shgrad_frames",
           "ws_shgrad_download", "ws_shgrad_add", "ws_renderer_accumulate_sh_gradient", "ws_sh_spread_rows", "ws_scene_accumulate_sh_gradient",
           "ws_refit_enable_sh", "ws_refit_step_sh", "ws_refit_download_sh", "ws_scene_refit_sh")
FIELDS = ("base", "lr_sh", "reserved")
F = np.float32


def test_sh_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    assert header.index("Gradients of an image loss:") < header.index("---- SH gradients:") < header.index("Refitting colour and opacity:")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared
    assert re.search(r"typedef struct ws_refit_sh_params \{[^}]*\} ws_refit_sh_params;", code)
    assert re.search(r"typedef struct ws_shgrad ws_shgrad;", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3   # additive: the ABI version stays where it was
    assert callable(ws.accumulate_sh_gradient_scene) and callable(ws.sh_spread_rows)
    assert all(hasattr(ws.ShGrad, m) for m in ("download", "add", "reset", "frames", "close", "num_points", "sh_deg"))
    assert all(hasattr(ws.Refit, m) for m in ("enable_sh", "step_sh", "download_sh")) and hasattr(ws.GaussianRenderer, "accumulate_sh_gradient")
    from websplat import shard
    a = {"sh": np.arange(24, dtype=np.int64).reshape(2, 4, 3), "opacity": np.array([5, -7], np.int64)}
    b = shard.reduce_shgrad(a)   # (one rank: a copy)
    assert np.array_equal(b["sh"], a["sh"]) and np.array_equal(b["opacity"], a["opacity"]) and b["sh"] is not a["sh"]


def test_sh_entry_points_compile_as_c99_and_descriptor_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){name}," for name in ENTRIES]
    src += ["  };", "  ws_refit_sh_params v; (void)v;", "  int ok = 1; for (unsigned i = 0; i < sizeof p / sizeof p[0]; ++i) ok &= p[i] != 0;",
            '  printf("%d", ok);', '  printf(" %d", (int)sizeof(ws_refit_sh_params));']
    src += [f'  printf(" %d", (int)offsetof(ws_refit_sh_params, {f}));' for f in FIELDS]
    src += ['  printf(" %d %d\\n", (int)sizeof v.lr_sh, (int)sizeof v.reserved);', "  return 0;", "}"]
    c = tmp_path / "sh_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "sh_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.ws_refit_sh_params
    assert out == [1, C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [4, 12]
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] == [72, 0, 56, 60]


def test_sh_entry_points_refuse_bad_descriptors_without_a_device(ws):
    """Everything that can be judged from a descriptor alone is refused before the handles are looked at: this tier has no device,
    so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib
    inf, nan = float("inf"), float("nan")

    def params(reserved=(0, 0, 0), base_reserved=(0, 0, 0, 0), lr_sh=0.000125, **kw):
        p = L.ws_refit_sh_params()
        vals = dict(refit_ref.DEFAULTS, colour_unit=2.0 ** -32, opacity_unit=2.0 ** -25)
        vals.update(kw)
        for k, v in vals.items():
            setattr(p.base, k, v)
        p.lr_sh = lr_sh
        for i, w in enumerate(reserved):
            p.reserved[i] = w
        for i, w in enumerate(base_reserved):
            p.base.reserved[i] = w
        return p

    def call(p):
        rc = lib.ws_refit_step_sh(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_refit_step_sh" in msg, (rc, msg)
        return msg

    def scene_call(p, kind=L.WS_ERROR_SQ, opacity_scale=1.0 / 128, split=L.WS_SPLIT_TRAIN):
        rc = lib.ws_scene_refit_sh(None, None, None, split, None, None, kind, opacity_scale, None, C.byref(p) if p is not None else None, 1, 0, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_scene_refit_sh" in msg, (rc, msg)
        return msg

    assert b"null params" in call(None) and b"null params" in scene_call(None)
    assert b"null argument" in call(params()) and b"null argument" in scene_call(params())
    assert b"null argument" in call(params(lr_sh=0.0, lr_colour=0.0, lr_opacity=0.0, beta1=0.0, beta2=0.0, opacity_min=1.0))   # the ends that are allowed
    for bad in (-1.0, inf, nan, -1e-30):
        assert b"lr_sh" in call(params(lr_sh=bad)) and b"lr_sh" in scene_call(params(lr_sh=bad))
        assert b"lr_colour" in call(params(lr_colour=bad)) and b"lr_opacity" in call(params(lr_opacity=bad))
    for bad in (1.0, -0.5, inf, nan):
        assert b"beta1" in call(params(beta1=bad)) and b"beta2" in scene_call(params(beta2=bad))
    for bad in (0.0, inf, nan):
        assert b"eps" in call(params(eps=bad)) and b"eps" in scene_call(params(eps=bad))
    for bad in (-0.01, 1.01, nan):
        assert b"opacity_min" in call(params(opacity_min=bad))
    for bad in (0.0, -1.0, inf, nan):
        assert b"colour_unit" in call(params(colour_unit=bad)) and b"opacity_unit" in call(params(opacity_unit=bad))
        assert b"null argument" in scene_call(params(colour_unit=bad, opacity_unit=bad))   # the driver computes the units itself
    for i in range(3):
        assert b"reserved" in call(params(reserved=tuple(int(k == i) for k in range(3))))
    for i in range(4):
        assert b"reserved" in call(params(base_reserved=tuple(int(k == i) for k in range(4))))
    assert b"kind" in scene_call(params(), kind=L.WS_ERROR_DSSIM) and b"split" in scene_call(params(), split=7)
    for bad in (0.0, -1.0, inf, nan):
        assert b"opacity_scale" in scene_call(params(), opacity_scale=bad)

    # the per-frame call: ws_renderer_accumulate_gradient's descriptor, under its own name
    def gparams(**kw):
        p = L.ws_gradient_params()
        p.scale, p.opacity_scale, p.d_grad, p.grad_pitch_bytes = 1.0, 1.0, 4096, 64
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def gcall(p):
        rc = lib.ws_renderer_accumulate_sh_gradient(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_renderer_accumulate_sh_gradient" in msg, (rc, msg)
        return msg

    assert b"null params" in gcall(None) and b"null argument" in gcall(gparams())
    for bad in (0.0, -1.0, inf, nan):
        assert b"scale" in gcall(gparams(scale=bad)) and b"opacity_scale" in gcall(gparams(opacity_scale=bad))
    assert b"null d_grad" in gcall(gparams(d_grad=None)) and b"multiples of 16" in gcall(gparams(d_grad=4100))
    assert b"multiples of 16" in gcall(gparams(grad_pitch_bytes=60)) and b"d_base" in gcall(gparams(d_base=4100, base_pitch_bytes=64))
    assert b"reserved" in gcall(gparams(reserved0=1))
    p = gparams()
    p.reserved[2] = 1
    assert b"reserved" in gcall(p)
    p = gparams()
    p.background[1] = nan
    assert b"background" in gcall(p)

    def sgcall(kind=L.WS_ERROR_SQ, scale=1.0, opacity_scale=1.0, split=L.WS_SPLIT_TRAIN):
        rc = lib.ws_scene_accumulate_sh_gradient(None, None, None, split, None, None, kind, scale, opacity_scale, None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_scene_accumulate_sh_gradient" in msg, (rc, msg)
        return msg

    assert b"null argument" in sgcall() and b"kind" in sgcall(kind=9) and b"split" in sgcall(split=7)
    assert b"scale" in sgcall(scale=0.0) and b"opacity_scale" in sgcall(opacity_scale=nan)
    # the objects' own calls refuse a null handle
    h = C.c_void_p()
    assert lib.ws_shgrad_create(None, 4, 3, C.byref(h)) == L.WS_ERR_INVALID and b"ws_shgrad_create" in lib.ws_last_error()
    assert lib.ws_shgrad_reset(None, None) == L.WS_ERR_INVALID and lib.ws_shgrad_download(None, 0, None, None) == L.WS_ERR_INVALID
    assert lib.ws_shgrad_add(None, None, None, 0) == L.WS_ERR_INVALID
    assert lib.ws_shgrad_num_points(None) == 0 and lib.ws_shgrad_sh_deg(None) == 0 and lib.ws_shgrad_frames(None) == 0
    lib.ws_shgrad_destroy(None)
    assert lib.ws_refit_enable_sh(None, None, None) == L.WS_ERR_INVALID and b"ws_refit_enable_sh" in lib.ws_last_error()
    assert lib.ws_refit_download_sh(None, 0, None, None, None) == L.WS_ERR_INVALID
    assert lib.ws_sh_spread_rows(None, None, None, 1, 3, 3, None, None) == L.WS_ERR_INVALID
    assert lib.ws_sh_spread_rows(None, None, None, 0, 4, 3, None, None) == L.WS_ERR_UNSUPPORTED


# ---- the basis is K1's --------------------------------------------------------------------------------------------------------
def test_basis_is_the_one_k1_evaluates():
    """The colour is linear in the coefficients before its clamp: one Gaussian per (k, sign) with sh[k][ch] = +-1 and everything
    else 0 has colour max(0, 0.5 +- basis_k(dir)) in the oracle's K1.  Of the two signs the one whose colour is off the clamp is
    compared: colour - 0.5 = +-basis_k within 2^-11, half an f16 ulp of a stored colour in [1, 2) -- the one rounding the
    restatement does not make."""
    rng = np.random.default_rng(7)
    ks = np.repeat(np.arange(1, 16), 2)
    signs = np.tile(np.array([1.0, -1.0], F), 15)
    n = ks.size
    xyz = rng.uniform(-0.4, 0.4, size=(n, 3)).astype(F)
    xyz[0::2] = xyz[1::2]   # the two signs of a coefficient at one place
    f_rest = np.zeros((n, 45), F)
    for ch in range(3):
        f_rest[np.arange(n), ch * 15 + ks - 1] = signs
    rows = synth._rows(xyz, np.zeros((n, 3), F), f_rest, np.full(n, 2.0, F), np.full((n, 3), np.log(0.02), F),
                       np.tile(np.array([1.0, 0.0, 0.0, 0.0], F), (n, 1)))
    g, sh = oracle.ply_rows_convert(rows, 3)
    bbox, center, _ = oracle.pointcloud_stats(g, 28, oracle.make_aabb([0, 0, 0], [0, 0, 0]))
    worst, used = 0.0, set()
    for eye in ([0.0, 0.0, -3.0], [2.5, 0.7, 1.5], [-1.2, -2.4, 1.1]):
        cj = synth.look_at_camera(0, eye, [0.0, 0.0, 0.0], 256, 256, 200.0, 200.0)
        cam = oracle.scene_camera_to_perspective(cj.position, cj.rotation, cj.fx, cj.fy, 256, 256)
        oracle.fit_near_far(cam, oracle.make_aabb([-1, -1, -1], [1, 1, 1]))
        cu = oracle.camera_uniform(cam, 256, 256)
        splats, _, src = oracle.preprocess(g, sh, cu, oracle.settings_uniform(bbox, center))
        assert src.size == n, "a Gaussian of the test left the frustum"
        colour = np.zeros((n, 3))
        colour[src] = np.ascontiguousarray(splats).view(np.float16).reshape(-1, 10)[:, 6:9].astype(np.float64)
        cam32 = np.array(list(cu.view_inv)[12:15], F)
        assert np.allclose(cam32, eye, atol=1e-5)
        bas = ref.basis(ref.direction(xyz, cam32)).astype(np.float64)
        assert np.abs(np.linalg.norm(ref.direction(xyz, cam32).astype(np.float64), axis=1) - 1.0).max() < 1e-6
        for k in range(1, 16):
            pair = np.flatnonzero(ks == k)
            for i in pair:
                want = float(signs[i]) * bas[i, k]
                if 0.5 + want > 2.0 ** -6:   # off the clamp (the other sign of the pair is then the clamped or the dimmer one)
                    assert (colour[i] > 0).all()
                    worst = max(worst, np.abs(colour[i] - 0.5 - want).max())
                    used.add(k)
            assert any(0.5 + float(signs[i]) * bas[i, k] > 2.0 ** -6 for i in pair)
    print(f"colour - 0.5 against +-basis_k over 3 views: largest gap {worst:.3e} (allowed 2^-11 = {2.0 ** -11:.3e})")
    assert used == set(range(1, 16)) and worst <= 2.0 ** -11


# ---- the reference by itself ------------------------------------------------------------------------------------------------------
def _sums(rng, n):
    """(N, 4) int64: magnitudes from 2^8 to 2^61, both signs, exact zeros (test_gpu_refit._sums)"""
    v = rng.integers(2 ** 60, 2 ** 61, size=(n, 4), dtype=np.int64) >> rng.integers(0, 53, size=(n, 4), dtype=np.int64)
    v *= rng.choice(np.array([-1, 1], np.int64), size=(n, 4))
    v[rng.uniform(size=(n, 4)) < 0.1] = 0
    return v


def _gaussians(seed, n=1000):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(F)
    cam = np.array([0.3, -1.7, 2.9], F)
    q4 = _sums(rng, n)
    q4[::9] = 0                                   # rows the spread does not look at
    xyz[3] = cam                                  # dl == 0
    xyz[4, 1], xyz[5, 0], xyz[6, 2] = np.inf, np.nan, -np.inf
    xyz[9] = np.nan                               # (a row of zero sums: the position is not read)
    q4[3:7] = np.array([2 ** 40, -(2 ** 41), 2 ** 33, -(2 ** 35)], np.int64)
    return q4, xyz, cam


def test_reference_spread_agrees_with_float64():
    """The f32 basis against float64.  Where the bound comes from: a basis is reached from xyz by at most 32 rounded f32
    operations (3 subtractions, 3 squares, 2 additions, the root and 3 divisions for the direction; up to 6 products and 5 more
    operations of the polynomial, each read by up to three of the direction's components), every one of them on a value of
    magnitude at most 4 scaled by a constant below 2.9 whose result stays below 1 in the end: one unit of 2^-23 of the product
    q * basis per operation is above each one's half ulp times the polynomial's sensitivity.  Plus 1 for the rounding to an
    integer."""
    q4, xyz, cam = _gaussians(11)
    fin = np.isfinite(xyz).all(axis=1) & (xyz != cam).any(axis=1)
    got, _ = ref.spread(q4[fin], xyz[fin], cam, 3)
    want = ref.spread64(q4[fin], xyz[fin], cam, 3)
    gap = np.abs(got.astype(np.float64) - want)
    allowed = 32.0 * np.abs(q4[fin][:, None, :3].astype(np.float64)) * 2.0 ** -23 + 1.0
    rel = (np.maximum(gap - 1.0, 0.0) / np.maximum(np.abs(q4[fin][:, None, :3].astype(np.float64)), 1.0))[:, 1:, :].max()
    print(f"spread, f32/int64 against float64: largest gap {rel / 2.0 ** -23:.2f} units of |q| 2^-23 (allowed 32, plus 1)")
    assert (gap <= allowed).all() and np.array_equal(got[:, 0, :], q4[fin][:, :3])
    assert np.abs(ref.basis64(ref.direction64(xyz[fin], cam))[:, 1:]).max() <= 1.0   # every basis is bounded by 1 on unit directions


def test_host_twin_equals_the_reference_bit_for_bit(ws):
    q4, xyz, cam = _gaussians(12)
    assert not np.isfinite(ref.direction(xyz, cam)[3:7]).all(axis=1).any()
    for sh_deg, active in ((3, 3), (3, 2), (3, 1), (3, 0), (2, 3), (2, 2), (1, 1), (0, 0), (0, 3)):
        got = ws.sh_spread_rows(q4, xyz, cam, sh_deg, active)
        sh, op = ref.spread(q4, xyz, cam, active, sh_deg)
        assert got["sh"].shape == sh.shape == (1000, (sh_deg + 1) ** 2, 3)
        assert np.array_equal(got["sh"], sh) and np.array_equal(got["opacity"], op), (sh_deg, active)
        nact = (min(sh_deg, active) + 1) ** 2
        assert not got["sh"][:, nact:, :].any() and (nact == 1 or got["sh"][:, 1:nact, :].any())
    # the rows without a finite direction keep their opacity and DC sums and get nothing else
    got = ws.sh_spread_rows(q4, xyz, cam, 3, 3)
    assert np.array_equal(got["sh"][3:7, 0, :], q4[3:7, :3]) and not got["sh"][3:7, 1:, :].any() and np.array_equal(got["opacity"][3:7], q4[3:7, 3])
    assert (got["sh"][10:, 1:, :] != 0).any(axis=(1, 2)).sum() > 800
    # it ADDS: twice the call is twice the sums, and g / -g negate
    from websplat import _lib as L
    i64 = C.POINTER(C.c_int64)
    f32 = C.POINTER(C.c_float)
    acc_sh, acc_op = got["sh"].copy(), got["opacity"].copy()
    assert ws.lib.ws_sh_spread_rows(q4.ctypes.data_as(i64), xyz.ctypes.data_as(f32), cam.ctypes.data_as(f32), 1000, 3, 3,
                                    acc_sh.ctypes.data_as(i64), acc_op.ctypes.data_as(i64)) == L.WS_OK
    assert np.array_equal(acc_sh, 2 * got["sh"]) and np.array_equal(acc_op, 2 * got["opacity"])
    neg = ws.sh_spread_rows(-q4, xyz, cam, 3, 3)
    assert np.array_equal(neg["sh"], -got["sh"]) and np.array_equal(neg["opacity"], -got["opacity"])


def test_reference_step_sh_with_a_frozen_rest_group_is_refit_ref_step():
    rng = np.random.default_rng(13)
    n = 200
    halves = np.concatenate([rng.uniform(-1.5, 1.5, size=(n, 3)), rng.uniform(0.05, 1.0, size=(n, 1))], axis=1).astype(np.float16)
    rest = (rng.standard_normal(size=(n, 15, 3)) * 0.1).astype(np.float16)
    a, b = ref.ShState(halves, rest), refit_ref.State(halves)
    for _ in range(4):
        q_sh = _sums(rng, n * 12).reshape(n, 16, 3)
        q_o = _sums(rng, n)[:, 0].copy()
        ref.step_sh(a, q_sh, q_o, 2.0 ** -32, 2.0 ** -30, lr_sh=0.0, lr_colour=0.01, lr_opacity=0.02)
        refit_ref.step(b, np.concatenate([q_sh[:, 0, :], q_o[:, None]], axis=1), 2.0 ** -32, 2.0 ** -30, lr_colour=0.01, lr_opacity=0.02)
        for k in ("master", "m", "v"):
            assert np.array_equal(getattr(a, k).view(np.uint32), getattr(b, k).view(np.uint32))
        assert a.steps == b.steps and a.p1 == b.p1 and a.p2 == b.p2
    assert np.array_equal(a.rest_halves().view(np.uint16), rest.view(np.uint16)) and not a.sh_m.any() and not a.sh_v.any()
    # ... and with a rate the rest group moves under the same powers, DC and opacity unchanged by that
    c = ref.ShState(halves, rest)
    q_sh = _sums(rng, n * 12).reshape(n, 16, 3)
    q_o = _sums(rng, n)[:, 0].copy()
    d = ref.ShState(halves, rest)
    ref.step_sh(c, q_sh, q_o, 2.0 ** -32, 2.0 ** -30, lr_sh=0.01)
    ref.step_sh(d, q_sh, q_o, 2.0 ** -32, 2.0 ** -30, lr_sh=0.0)
    assert np.array_equal(c.master.view(np.uint32), d.master.view(np.uint32)) and (c.sh_master != d.sh_master).sum() > n * 30
    assert np.array_equal(c.sh_master[q_sh[:, 1:, :] == 0].view(np.uint32), d.sh_master[q_sh[:, 1:, :] == 0].view(np.uint32))
