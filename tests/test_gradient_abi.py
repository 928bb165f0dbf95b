"""CPU tests of the gradient ABI (include/websplat.h "Gradients of an image loss"): declared, exported, bound, usable from C99, the
descriptor's layout shared with the Python stub, every descriptor error refused before any handle is looked at; and
tests/gradient_ref.py against finite differences on a synthetic frame, all in float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ws_renderer_accumulate_gradient"
ENTRIES = (ENTRY, "ws_scene_accumulate_gradient", "ws_image_error_gradient", "ws_grad_create", "ws_grad_destroy", "ws_grad_reset",
           "ws_grad_num_points", "ws_grad_frames", "ws_grad_download", "ws_grad_add")
FIELDS = ("background", "scale", "opacity_scale", "reserved0", "d_grad", "grad_pitch_bytes", "d_base", "base_pitch_bytes", "reserved")


def test_gradient_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared
    assert re.search(r"typedef struct ws_gradient_params \{[^}]*\} ws_gradient_params;", code)
    assert re.search(r"typedef struct ws_grad ws_grad;", code)
    assert re.search(r"#define WS_GRAD_CHANNELS 4\b", code) and re.search(r"#define WS_GRAD_SUM_SCALE 4294967296\.0", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3   # additive: the ABI version stays where it was
    assert hasattr(ws.GaussianRenderer, "accumulate_gradient") and callable(ws.image_error_gradient) and callable(ws.accumulate_gradient_scene)
    assert all(hasattr(ws.Grad, m) for m in ("download", "add", "reset", "frames", "close"))
    from websplat import shard
    q = np.arange(-6, 6, dtype=np.int64).reshape(3, 4)
    got = shard.reduce_grad(q)
    assert got.dtype == np.int64 and np.array_equal(got, q) and got is not q
    assert _lib.WS_GRAD_CHANNELS == 4 and _lib.WS_GRAD_SUM_SCALE == 2.0 ** 32


def test_gradient_entry_points_compile_as_c99_and_descriptor_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){name}," for name in ENTRIES]
    src += ["  };", "  ws_gradient_params v; (void)v;", "  int ok = 1; for (unsigned i = 0; i < sizeof p / sizeof p[0]; ++i) ok &= p[i] != 0;",
            '  printf("%d", ok);', '  printf(" %d", (int)sizeof(ws_gradient_params));']
    src += [f'  printf(" %d", (int)offsetof(ws_gradient_params, {f}));' for f in FIELDS]
    src += ['  printf(" %d %d %d\\n", (int)sizeof v.background, (int)sizeof v.reserved, WS_GRAD_CHANNELS);', "  return 0;", "}"]
    c = tmp_path / "gradient_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "gradient_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.ws_gradient_params
    assert out == [1, C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [12, 16, 4]
    assert (C.sizeof(P), P.scale.offset, P.opacity_scale.offset, P.reserved0.offset, P.d_grad.offset, P.grad_pitch_bytes.offset,
            P.d_base.offset, P.base_pitch_bytes.offset, P.reserved.offset) == (72, 12, 16, 20, 24, 32, 40, 48, 56)


def test_gradient_entry_point_refuses_bad_descriptors_without_a_device(ws):
    """Everything that can be judged from the descriptor alone is refused before the handles are looked at: this tier has no
    device, so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib
    buf = (C.c_float * 64)()          # host memory standing in for device pointers: nothing dereferences them
    ptr = (C.addressof(buf) + 15) // 16 * 16

    def params(background=(0.1, 0.2, 0.3), scale=1.0, opacity_scale=1.0, grad=ptr, grad_pitch=64, base=None, base_pitch=64,
               reserved0=0, reserved=(0, 0, 0, 0)):
        p = L.ws_gradient_params()
        for i in range(3):
            p.background[i] = background[i]
        p.scale, p.opacity_scale, p.reserved0 = scale, opacity_scale, reserved0
        p.d_grad, p.grad_pitch_bytes = grad, grad_pitch
        if base is not None:
            p.d_base, p.base_pitch_bytes = base, base_pitch
        for i, w in enumerate(reserved):
            p.reserved[i] = w
        return p

    def call(p):
        rc = lib.ws_renderer_accumulate_gradient(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and ENTRY.encode() in msg, (rc, msg)
        return msg

    inf, nan = float("inf"), float("nan")
    assert b"null params" in call(None)
    assert b"null argument" in call(params())                                   # a good descriptor: only the handles are wrong
    assert b"null argument" in call(params(base=ptr, scale=0.25, opacity_scale=1.0 / 128))
    for bad in (0.0, -1.0, inf, nan):
        assert b": scale" in call(params(scale=bad))
        assert b"opacity_scale" in call(params(opacity_scale=bad))
    for i in range(3):
        for bad in (inf, nan):
            assert b"background" in call(params(background=tuple(bad if k == i else 0.0 for k in range(3))))
    assert b"null d_grad" in call(params(grad=None))
    assert b"d_grad" in call(params(grad=ptr + 4)) and b"multiples of 16" in lib.ws_last_error()   # 4-B aligned is not enough
    assert b"d_grad" in call(params(grad=ptr + 8))
    assert b"grad_pitch_bytes" in call(params(grad_pitch=72))                   # a multiple of 8, not of 16
    assert b"d_base" in call(params(base=ptr + 4))
    assert b"base_pitch_bytes" in call(params(base=ptr, base_pitch=72))
    assert b"reserved" in call(params(reserved0=1))
    for i in range(4):
        assert b"reserved" in call(params(reserved=tuple(int(k == i) for k in range(4))))
    # the scene driver judges its scalars first, too
    scene = b"ws_scene_accumulate_gradient"
    for kind, scale, oscale, word in ((L.WS_ERROR_DSSIM, 1.0, 1.0, b"kind"), (9, 1.0, 1.0, b"kind"), (L.WS_ERROR_SQ, 0.0, 1.0, b"scale"),
                                      (L.WS_ERROR_SQ, 1.0, nan, b"opacity_scale"), (L.WS_ERROR_ABS, inf, 1.0, b"scale")):
        rc = lib.ws_scene_accumulate_gradient(None, None, None, L.WS_SPLIT_TEST, None, None, kind, scale, oscale, None, None)
        assert rc == L.WS_ERR_INVALID and scene in lib.ws_last_error() and word in lib.ws_last_error()
    assert lib.ws_scene_accumulate_gradient(None, None, None, L.WS_SPLIT_TEST, None, None, L.WS_ERROR_SQ, 1.0, 1.0, None, None) == L.WS_ERR_INVALID
    assert b"null argument" in lib.ws_last_error()
    # the image gradient: nulls, QUANTIZE_U8
    assert lib.ws_image_error_gradient(None, None, None, 4, 4, L.WS_ERROR_SQ, 0, None, 64, None) == L.WS_ERR_INVALID
    assert b"ws_image_error_gradient" in lib.ws_last_error()
    # the accumulator's own calls refuse a null handle
    assert lib.ws_grad_reset(None, None) == L.WS_ERR_INVALID and lib.ws_grad_download(None, 0, None) == L.WS_ERR_INVALID
    assert lib.ws_grad_add(None, None, 0) == L.WS_ERR_INVALID and lib.ws_grad_num_points(None) == 0 and lib.ws_grad_frames(None) == 0


# ---- the reference against finite differences, float64 ---------------------------------------------------------------------------
W, H, N = 64, 48, 300
BG = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def synthetic():
    """test_removal_abi's synthetic frame with opacities so faint that no pair is clamped and no pixel comes near a stop."""
    import gradient_ref
    from gradient_frames import signed_ramp
    from test_removal_abi import _synthetic_frame
    frame = _synthetic_frame(N, W, H, 5, opacity=(0.02, 0.2))
    G = gradient_ref.plane_G(signed_ramp(W, H))
    return frame, G, gradient_ref.gradient_f64(frame, W, H, 2 * N, G, BG)


def _loss(G, F, T):
    return float((G[..., :3].astype(np.float64) * F).sum() + (G[..., 3].astype(np.float64) * T).sum())


def test_reference_equals_finite_differences(synthetic):
    """L = sum_p G . (F, T_end) is linear in every colour and affine in a common factor on a Gaussian's opacity while no clamp and
    no stop intervenes: central differences of the float64 forward pass agree with the reference to float64 rounding."""
    import gradient_ref
    import removal_ref
    import weight_ref
    frame, G, ref = synthetic
    assert int(ref["clamped"].sum()) == 0 and ref["T"].min() > 2.0 ** -13 and int(ref["band"].sum()) == 0
    recs = list(weight_ref.records(frame, W, H))
    col = removal_ref._colours(frame)
    assert (col[np.unique([j for j, *_ in recs])] > 0).all()   # no colour on K1's clamp: every pair counts in every channel
    F0, T0 = gradient_ref.forward_f64(recs, col, BG, W, H)
    assert np.array_equal(F0, ref["F"]) and np.array_equal(T0, ref["T"])
    drawn = np.nonzero(ref["pairs"] > 0)[0]
    assert drawn.size > 100
    mag = np.abs(ref["sum"][drawn, 3])
    rng = np.random.default_rng(3)
    picks = [int(drawn[np.argmax(mag)])] + [int(j) for j in rng.choice(drawn, 5, replace=False)]
    eps = 1e-3   # (exact linearity: any step is valid; a large one keeps the difference's own rounding small)
    worst = 0.0
    for j in picks:
        for ch in range(3):
            hi, lo = col.copy(), col.copy()
            hi[j, ch] += eps
            lo[j, ch] -= eps
            fd = (_loss(G, *gradient_ref.forward_f64(recs, hi, BG, W, H)) - _loss(G, *gradient_ref.forward_f64(recs, lo, BG, W, H))) / (2 * eps)
            scale_of = np.abs(ref["sum"][j, :3]).max()
            worst = max(worst, abs(fd - ref["sum"][j, ch]) / scale_of)
        # d / d ln(factor) at factor 1 of an affine function of the factor: the central difference in the factor itself
        fd = (_loss(G, *gradient_ref.forward_f64(recs, col, BG, W, H, {j: 1 + eps})) -
              _loss(G, *gradient_ref.forward_f64(recs, col, BG, W, H, {j: 1 - eps}))) / (2 * eps)
        worst = max(worst, abs(fd - ref["sum"][j, 3]) / abs(ref["sum"][j, 3]))
    print(f"finite differences vs the reference, {len(picks)} Gaussians x 4: worst relative difference {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("mutation", ["sign_flipped", "r_over_Tb", "clamped_pairs_counted"])
def test_reference_bounds_reject_wrong_formulas(synthetic, mutation):
    """Each mutation leaves bounds() for most Gaussians it can touch.  clamped_pairs_counted needs clamped pairs: every tenth
    Gaussian of the synthetic frame gets alpha 1 (its core sits on the 0.99 clamp), masked where a pair is undecided or the
    pixel saturates."""
    import gradient_ref
    frame, G, ref = synthetic
    if mutation == "clamped_pairs_counted":
        h = frame["splats"].view(np.float16).reshape(N, 10).copy()
        h[::10, 9] = 1.0
        frame = dict(frame, splats=h.view(np.uint8).reshape(N, 20))
        und = gradient_ref.gradient_f64(frame, W, H, 2 * N, G, BG)
        G = G * ((und["und"] == 0) & (und["T"] >= 2.0 ** -13))[..., None]
        ref = gradient_ref.gradient_f64(frame, W, H, 2 * N, G, BG)
        touched = ref["clamped"] > 0
        assert touched.sum() >= 5
    else:
        touched = ref["pairs"] > 0
    tol = gradient_ref.bounds(ref)[:, 3]
    wrong = gradient_ref.gradient_f64(frame, W, H, 2 * N, G, BG, mutate=mutation)
    assert np.array_equal(wrong["sum"][:, :3], ref["sum"][:, :3])   # (the mutations are of the opacity sum)
    out = np.abs(wrong["sum"][:, 3] - ref["sum"][:, 3]) > tol
    share = out[touched].mean()
    print(f"{mutation}: {100 * share:.1f} % of {int(touched.sum())} Gaussians leave bounds(); "
          f"median tol / |sum| = {np.median(tol[touched] / np.maximum(np.abs(ref['sum'][touched, 3]), 1e-300)):.3e}")
    assert share >= 0.5
    assert (gradient_ref.bounds(ref)[ref["pairs"] > 0] > 0).all()


def test_reference_ties(synthetic):
    """The definition's exact consequences hold in the reference too: negation, a mask and its complement, and the colour sum of
    g = (1, 0, 0, 0) is the contribution sum."""
    import contrib_ref
    import gradient_ref
    frame, G, ref = synthetic
    neg = gradient_ref.gradient_f64(frame, W, H, 2 * N, -G, BG)
    assert np.array_equal(neg["sum"], -ref["sum"])
    mask = (np.random.default_rng(11).uniform(size=(H, W)) < 0.4)[..., None]
    a = gradient_ref.gradient_f64(frame, W, H, 2 * N, G * mask, BG)
    b = gradient_ref.gradient_f64(frame, W, H, 2 * N, G * ~mask, BG)
    assert np.abs(a["sum"] + b["sum"] - ref["sum"]).max() <= 1e-12 * np.abs(ref["sum"]).max()
    ones = np.zeros((H, W, 4), np.float32)
    ones[..., 0] = 1
    red = gradient_ref.gradient_f64(frame, W, H, 2 * N, ones, BG)
    plain = contrib_ref.contrib_f64(frame, W, H, 2 * N)
    assert np.abs(red["sum"][:, 0] - plain["sum"]).max() <= 1e-12 * plain["sum"].max() and not red["sum"][:, 1:3].any()
