"""CPU tests of the refit ABI (include/websplat.h "Refitting colour and opacity"): declared, exported, bound, usable from C99, the
descriptor's layout shared with the Python stub, every descriptor error refused before any handle is looked at; and
tests/refit_ref.py by itself: the fixed point, descent on a quadratic, and float64 Adam."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import refit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ws_refit_step"
ENTRIES = (ENTRY, "ws_refit_create", "ws_refit_destroy", "ws_refit_num_points", "ws_refit_steps", "ws_refit_download", "ws_scene_refit")
FIELDS = ("lr_colour", "lr_opacity", "beta1", "beta2", "eps", "opacity_min", "colour_unit", "opacity_unit", "reserved")
F = np.float32


def test_refit_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    assert header.index("Gradients of an image loss:") < header.index("Refitting colour and opacity:") < header.index("---- view batches")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared
    assert re.search(r"typedef struct ws_refit_params \{[^}]*\} ws_refit_params;", code)
    assert re.search(r"typedef struct ws_refit ws_refit;", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3   # additive: the ABI version stays where it was
    assert callable(ws.refit_scene) and all(hasattr(ws.Refit, m) for m in ("step", "download", "steps", "close", "num_points"))


def test_refit_entry_points_compile_as_c99_and_descriptor_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){name}," for name in ENTRIES]
    src += ["  };", "  ws_refit_params v; (void)v;", "  int ok = 1; for (unsigned i = 0; i < sizeof p / sizeof p[0]; ++i) ok &= p[i] != 0;",
            '  printf("%d", ok);', '  printf(" %d", (int)sizeof(ws_refit_params));']
    src += [f'  printf(" %d", (int)offsetof(ws_refit_params, {f}));' for f in FIELDS]
    src += ['  printf(" %d %d\\n", (int)sizeof v.colour_unit, (int)sizeof v.reserved);', "  return 0;", "}"]
    c = tmp_path / "refit_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "refit_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.ws_refit_params
    assert out == [1, C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [8, 16]
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] == [56, 0, 4, 8, 12, 16, 20, 24, 32, 40]


def test_refit_entry_points_refuse_bad_descriptors_without_a_device(ws):
    """Everything that can be judged from the descriptor alone is refused before the handles are looked at: this tier has no
    device, so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib

    def params(reserved=(0, 0, 0, 0), **kw):
        p = L.ws_refit_params()
        vals = dict(refit_ref.DEFAULTS, colour_unit=2.0 ** -32, opacity_unit=2.0 ** -25)
        vals.update(kw)
        for k, v in vals.items():
            setattr(p, k, v)
        for i, w in enumerate(reserved):
            p.reserved[i] = w
        return p

    def call(p):
        rc = lib.ws_refit_step(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and ENTRY.encode() in msg, (rc, msg)
        return msg

    def scene_call(p, kind=L.WS_ERROR_SQ, opacity_scale=1.0 / 128, split=L.WS_SPLIT_TRAIN):
        rc = lib.ws_scene_refit(None, None, None, split, None, None, kind, opacity_scale, None, C.byref(p) if p is not None else None, 1, 0, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_scene_refit" in msg, (rc, msg)
        return msg

    inf, nan = float("inf"), float("nan")
    assert b"null params" in call(None) and b"null params" in scene_call(None)
    assert b"null argument" in call(params())                      # a good descriptor: only the handles are wrong
    assert b"null argument" in call(params(lr_colour=0.0, lr_opacity=0.0, beta1=0.0, beta2=0.0, opacity_min=1.0))   # the ends that are allowed
    assert b"null argument" in scene_call(params())
    for bad in (-1.0, inf, nan, -1e-30):
        assert b"lr_colour" in call(params(lr_colour=bad)) and b"lr_opacity" in call(params(lr_opacity=bad))
        assert b"lr_colour" in scene_call(params(lr_colour=bad))
    for bad in (1.0, -0.5, 1.5, inf, nan):
        assert b"beta1" in call(params(beta1=bad)) and b"beta2" in call(params(beta2=bad))
        assert b"beta2" in scene_call(params(beta2=bad))
    for bad in (0.0, -1e-15, inf, nan):
        assert b"eps" in call(params(eps=bad)) and b"eps" in scene_call(params(eps=bad))
    for bad in (-0.01, 1.01, inf, nan):
        assert b"opacity_min" in call(params(opacity_min=bad)) and b"opacity_min" in scene_call(params(opacity_min=bad))
    for bad in (0.0, -1.0, inf, nan):
        assert b"colour_unit" in call(params(colour_unit=bad)) and b"opacity_unit" in call(params(opacity_unit=bad))
        # the scene driver computes the units itself: it does not look at them
        assert b"null argument" in scene_call(params(colour_unit=bad, opacity_unit=bad))
    for i in range(4):
        assert b"reserved" in call(params(reserved=tuple(int(k == i) for k in range(4))))
    # the scene driver judges its scalars first, too
    assert b"kind" in scene_call(params(), kind=L.WS_ERROR_DSSIM) and b"kind" in scene_call(params(), kind=9)
    for bad in (0.0, -1.0, inf, nan):
        assert b"opacity_scale" in scene_call(params(), opacity_scale=bad)
    assert b"split" in scene_call(params(), split=7)
    # the object's own calls refuse a null handle
    h = C.c_void_p()
    assert lib.ws_refit_create(None, None, C.byref(h)) == L.WS_ERR_INVALID and b"ws_refit_create" in lib.ws_last_error()
    assert lib.ws_refit_download(None, 0, None, None, None) == L.WS_ERR_INVALID and lib.ws_refit_num_points(None) == 0 and lib.ws_refit_steps(None) == 0
    lib.ws_refit_destroy(None)


# ---- the reference by itself ---------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_reference_zero_gradient_is_a_fixed_point_bitwise():
    rng = np.random.default_rng(5)
    halves = np.concatenate([rng.uniform(-1.5, 1.5, size=(200, 3)), rng.uniform(0.0, 1.0, size=(200, 1))], axis=1).astype(np.float16)
    halves[:4, 3] = (0.0, 1.0, 6e-8, 0.5)
    st = refit_ref.State(halves)
    before = st.master.copy()
    for _ in range(3):
        refit_ref.step(st, np.zeros((200, 4), np.int64), 2.0 ** -32, 2.0 ** -32, lr_colour=0.5, lr_opacity=0.5)
    assert np.array_equal(_bits(st.master), _bits(before)) and not st.m.any() and not st.v.any() and st.steps == 3
    assert np.array_equal(st.halves().view(np.uint16), halves.view(np.uint16))
    # a Gaussian of zero sums among moving ones keeps its values, too
    q = rng.integers(-2 ** 40, 2 ** 40, size=(200, 4), dtype=np.int64)
    q[::7] = 0
    refit_ref.step(st, q, 2.0 ** -32, 2.0 ** -32)
    assert np.array_equal(_bits(st.master[::7]), _bits(before[::7])) and (st.master[1::7] != before[1::7]).all()


def test_reference_descends_a_separable_quadratic():
    """L = sum_k a_k (x_k - t_k)^2 / 2 with the derivatives handed over the way a ws_grad holds them: colour sums are
    dL/d colour (the step multiplies by C0), the opacity sum is dL/d ln opacity = x dL/dx (the step divides by x)."""
    rng = np.random.default_rng(9)
    n = 64
    t = np.concatenate([rng.uniform(-1.0, 1.0, size=(n, 3)), rng.uniform(0.35, 0.65, size=(n, 1))], axis=1)
    off = rng.uniform(0.2, 0.3, size=(n, 4)) * rng.choice([-1.0, 1.0], size=(n, 4))
    a = rng.uniform(0.5, 4.0, size=(n, 4))
    st = refit_ref.State((t + off).astype(np.float16))
    start = np.abs(st.master.astype(np.float64) - t)
    for _ in range(200):
        x = st.master.astype(np.float64)
        d = a * (x - t)
        d[:, :3] /= refit_ref.C0
        d[:, 3] *= x[:, 3]
        refit_ref.step(st, np.rint(d * 2.0 ** 32).astype(np.int64), 2.0 ** -32, 2.0 ** -32, lr_colour=0.01, lr_opacity=0.01)
    end = np.abs(st.master.astype(np.float64) - t)
    print(f"|x - t|: start {start.min():.3f} .. {start.max():.3f}, after 200 steps at most {end.max():.4f}")
    assert (end < start).all() and st.steps == 200


def test_reference_agrees_with_float64_adam():
    """20 steps, colour group, x in [0.8, 2.2] throughout (x0 in [1, 2], 20 steps of at most lr = 0.01 each): within a relative
    2^-18 of float64 Adam.  Where the bound comes from: about 10 rounded operations per step, each contributing at most 2^-24,
    over 20 steps, with a margin of 4.  The inputs keep |g| inside [2^-20, 2^20]: nothing is denormal, nothing overflows (asserted
    on the trace)."""
    rng = np.random.default_rng(13)
    n = 256
    x0 = rng.uniform(1.0, 2.0, size=(n, 4)).astype(np.float16)
    st = refit_ref.State(x0)
    grads = []
    trace = []
    for _ in range(20):
        mag = 2.0 ** rng.uniform(-20.0, 20.0, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
        q = np.zeros((n, 4), np.int64)
        q[:, :3] = np.rint(mag * 2.0 ** 32 / refit_ref.C0).astype(np.int64)
        g = q[:, :3].astype(np.float64) * (2.0 ** -32 * refit_ref.C0)
        assert np.abs(g).min() >= 2.0 ** -20.01 and np.abs(g).max() <= 2.0 ** 20.01
        grads.append(g)
        refit_ref.step(st, q, 2.0 ** -32, 2.0 ** -32, lr_colour=0.01, lr_opacity=0.0, trace=trace)
    assert refit_ref.all_zero_or_normal(trace)
    want = refit_ref.adam_f64(x0[:, :3], grads, 0.01)
    rel = np.abs(st.master[:, :3].astype(np.float64) - want) / np.abs(want)
    print(f"f32 step against float64 Adam after 20 steps: largest relative difference 2^{np.log2(rel.max()):.2f}")
    assert rel.max() <= 2.0 ** -18
    assert np.array_equal(_bits(st.master[:, 3]), _bits(x0[:, 3].astype(F))) and not st.m[:, 3].any()   # (the frozen group)
