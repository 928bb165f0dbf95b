"""CPU tests of the removal-effect ABI (include/websplat.h "Removal effect"): declared, exported, bound, usable from C99, the
descriptor's layout shared with the Python stub, every descriptor error refused before any handle is looked at; and
tests/removal_ref.py against brute-force deletion on a synthetic frame, all in float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ws_renderer_accumulate_removal"
SCENE_ENTRY = "ws_scene_accumulate_removal"
FIELDS = ("background", "kind", "scale", "weight", "d_base", "base_pitch_bytes", "reserved")


def test_removal_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert ENTRY in declared and SCENE_ENTRY in declared
    assert re.search(r"typedef struct ws_removal_params \{[^}]*\} ws_removal_params;", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in (ENTRY, SCENE_ENTRY):
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    # additive: the ABI version stays where it was
    assert ws.lib.ws_abi_version() == 3
    assert hasattr(ws.GaussianRenderer, "accumulate_removal") and hasattr(ws.GaussianRenderer, "download_removal_base")
    assert callable(ws.accumulate_removal_scene)


def test_removal_entry_points_compile_as_c99_and_descriptor_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {",
           f"  void* p = (void*){ENTRY}; void* q = (void*){SCENE_ENTRY};", "  ws_removal_params v; (void)v;",
           '  printf("%d", p != 0 && q != 0);', '  printf(" %d", (int)sizeof(ws_removal_params));']
    src += [f'  printf(" %d", (int)offsetof(ws_removal_params, {f}));' for f in FIELDS]
    src += ['  printf(" %d %d\\n", (int)sizeof v.background, (int)sizeof v.reserved);', "  return 0;", "}"]
    c = tmp_path / "removal_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "removal_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.ws_removal_params
    assert out == [1, C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [12, 16]
    assert (C.sizeof(P), P.kind.offset, P.scale.offset, P.weight.offset, P.d_base.offset, P.base_pitch_bytes.offset,
            P.reserved.offset) == (64, 12, 16, 24, 32, 40, 48)


def test_removal_entry_point_refuses_bad_descriptors_without_a_device(ws):
    """Everything that can be judged from the descriptor alone is refused before the handles are looked at: this tier has no
    device, so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib
    buf = (C.c_float * 64)()          # host memory standing in for device pointers: nothing dereferences them
    ptr = (C.addressof(buf) + 15) // 16 * 16

    def params(background=(0.1, 0.2, 0.3), kind=L.WS_ERROR_SQ, scale=1.0, weight=None, base=None, base_pitch=64, reserved=(0, 0, 0, 0)):
        p = L.ws_removal_params()
        for i in range(3):
            p.background[i] = background[i]
        p.kind, p.scale = kind, scale
        if weight is not None:
            p.weight = C.pointer(weight)
        if base is not None:
            p.d_base, p.base_pitch_bytes = base, base_pitch
        for i, w in enumerate(reserved):
            p.reserved[i] = w
        return p

    def plane(pointer=ptr, pitch=64, scale=1.0, bias=0.0):
        v = L.ws_plane_view()
        v.d_values, v.row_pitch_bytes, v.scale, v.bias = pointer, pitch, scale, bias
        return v

    def call(p):
        rc = lib.ws_renderer_accumulate_removal(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and ENTRY.encode() in msg, (rc, msg)
        return msg

    inf, nan = float("inf"), float("nan")
    assert b"null params" in call(None)
    assert b"null argument" in call(params())                                   # a good descriptor: only the handles are wrong
    assert b"null argument" in call(params(kind=L.WS_ERROR_ABS, weight=plane(), base=ptr))
    assert b"kind" in call(params(kind=L.WS_ERROR_DSSIM))
    assert b"kind" in call(params(kind=7))
    assert b"kind" in call(params(kind=-1))
    for bad in (0.0, -1.0, inf, nan):
        assert b"scale" in call(params(scale=bad))
    for i in range(3):
        for bad in (inf, nan):
            assert b"background" in call(params(background=tuple(bad if k == i else 0.0 for k in range(3))))
    assert b"weight" in call(params(weight=plane(pointer=None))) and b"d_values" in lib.ws_last_error()
    assert b"weight" in call(params(weight=plane(scale=nan)))
    assert b"weight" in call(params(weight=plane(bias=inf)))
    assert b"weight" in call(params(weight=plane(pitch=66))) and b"multiples of 4" in lib.ws_last_error()
    assert b"weight" in call(params(weight=plane(pointer=ptr + 2)))
    assert b"d_base" in call(params(base=ptr + 4))                              # 4-B aligned is not enough
    assert b"base_pitch_bytes" in call(params(base=ptr, base_pitch=72))         # a multiple of 8, not of 16
    for i in range(4):
        assert b"reserved" in call(params(reserved=tuple(int(k == i) for k in range(4))))
    # the scene driver judges its scalars first, too
    for kind, scale, word in ((L.WS_ERROR_DSSIM, 1.0, b"kind"), (9, 1.0, b"kind"), (L.WS_ERROR_SQ, 0.0, b"scale"), (L.WS_ERROR_SQ, nan, b"scale")):
        rc = lib.ws_scene_accumulate_removal(None, None, None, L.WS_SPLIT_TEST, kind, scale, None, None, None)
        assert rc == L.WS_ERR_INVALID and SCENE_ENTRY.encode() in lib.ws_last_error() and word in lib.ws_last_error()
    assert lib.ws_scene_accumulate_removal(None, None, None, L.WS_SPLIT_TEST, L.WS_ERROR_SQ, 1.0, None, None, None) == L.WS_ERR_INVALID
    assert b"null argument" in lib.ws_last_error()


# ---- the reference against brute force, float64 -------------------------------------------------------------------------------
W, H, N = 64, 48, 300
BG = (0.25, 0.5, 0.75)


def _synthetic_frame(n, width, height, seed, opacity=(0.02, 0.3)):
    """test_values_abi._synthetic_frame with the opacities of a frame that does not saturate."""
    from test_values_abi import _synthetic_frame as base
    frame = base(n, width, height, seed)
    h = frame["splats"].view(np.float16).reshape(n, 10).copy()
    h[:, 9] = np.random.default_rng(seed + 1).uniform(*opacity, size=n)
    frame["splats"] = h.view(np.uint8).reshape(n, 20)
    return frame


@pytest.fixture(scope="module")
def synthetic():
    import removal_ref
    frame = _synthetic_frame(N, W, H, 5)
    return frame, removal_ref.removal_f64(frame, W, H, 2 * N, BG)


def test_reference_equals_brute_force_deletion(synthetic):
    import removal_ref
    frame, ref = synthetic
    drawn = np.nonzero(ref["sum"] > 0)[0]
    assert drawn.size > 100 and ref["T"].min() > 2.0 ** -13   # no stop, no threshold: the closed form is exact
    rng = np.random.default_rng(3)
    picks = [int(drawn[np.argmax(ref["sum"][drawn])]), int(drawn[np.argmin(ref["sum"][drawn])])] + [int(j) for j in rng.choice(drawn, 4, replace=False)]
    worst = 0.0
    for j in picks:
        without = removal_ref.base_f64(frame, W, H, BG, skip=j)["F"]
        brute = ((without - ref["F"]) ** 2).mean(axis=-1).sum()
        worst = max(worst, abs(brute - ref["sum"][j]) / ref["sum"][j])
    print(f"brute force vs closed form, {len(picks)} Gaussians: worst relative difference {worst:.3e}")
    assert worst <= 1e-9
    # abs: the same deletion, the other measure
    ref_abs = removal_ref.removal_f64(frame, W, H, 2 * N, BG, kind="abs")
    j = picks[0]
    brute = np.abs(removal_ref.base_f64(frame, W, H, BG, skip=j)["F"] - ref["F"]).mean(axis=-1).sum()
    assert abs(brute - ref_abs["sum"][j]) <= 1e-9 * brute


def test_reference_weight_plane_identities(synthetic):
    import removal_ref
    frame, ref = synthetic
    ones = removal_ref.removal_f64(frame, W, H, 2 * N, BG, E=np.ones((H, W), np.float32))
    assert np.array_equal(ones["sum"], ref["sum"]) and np.array_equal(ones["max"], ref["max"])
    rng = np.random.default_rng(11)
    mask = (rng.uniform(size=(H, W)) < 0.4).astype(np.float32)
    a = removal_ref.removal_f64(frame, W, H, 2 * N, BG, E=mask)
    b = removal_ref.removal_f64(frame, W, H, 2 * N, BG, E=1.0 - mask)
    assert np.abs(a["sum"] + b["sum"] - ref["sum"]).max() <= 1e-12 * ref["sum"].max()
    assert np.array_equal(np.maximum(a["max"], b["max"]), ref["max"])
    assert np.array_equal(a["pairs"] + b["pairs"], ref["pairs"])


def _wall_frame(decoy_colour):
    """Ten opaque layers (alpha 1 -> b = 0.99) of one colour over the whole 32 x 32 view, and in front of them one small Gaussian."""
    wall = np.array([0.75, 0.25, 0.5])
    n = 11
    h = np.zeros((n, 10), dtype=np.float16)
    h[:, 0], h[:, 3] = 40.0 / 32, -40.0 / 32          # sigma 40 px: the wall is flat across the view
    h[0, 0], h[0, 3] = 4.0 / 32, -4.0 / 32            # the Gaussian in front, sigma 4 px, at the centre
    h[:, 6:9] = wall
    h[0, 6:9] = decoy_colour
    h[:, 9] = 1.0
    h[0, 9] = 0.9
    order = np.arange(n)[::-1].astype(np.uint32)      # far -> near: record 0 is drawn last, it is the nearest
    return {"splats": h.view(np.uint8).reshape(n, 20), "sorted": order, "src_index": np.arange(n, dtype=np.uint32)}


def test_reference_tells_a_decoy_from_a_highlight():
    import contrib_ref
    import removal_ref
    same, other = _wall_frame([0.75, 0.25, 0.5]), _wall_frame([0.1, 0.9, 0.2])
    for frame, is_decoy in ((same, True), (other, False)):
        ref = removal_ref.removal_f64(frame, 32, 32, 11, (0.0, 0.0, 0.0))
        drew = contrib_ref.contrib_f64(frame, 32, 32, 11)["sum"][0]
        assert drew > 10
        print(f"in front of a wall, {'its' if is_decoy else 'another'} colour: effect {ref['sum'][0]:.3e}, contribution {drew:.3f}")
        assert (ref["sum"][0] < 1e-6 * drew) == is_decoy


@pytest.mark.parametrize("mutation", ["no_background", "prefix_without_i", "r_over_Tb"])
def test_reference_bounds_reject_wrong_formulas(synthetic, mutation):
    import removal_ref
    frame, ref = synthetic
    tol_sum, tol_max = removal_ref.bounds(ref)
    drawn = ref["sum"] > 0
    wrong = removal_ref.removal_f64(frame, W, H, 2 * N, BG, mutate=mutation)
    out = np.abs(wrong["sum"] - ref["sum"]) > tol_sum
    share = out[drawn].mean()
    print(f"{mutation}: {100 * share:.1f} % of {int(drawn.sum())} drawn Gaussians leave bounds(); "
          f"median tol / sum = {np.median(tol_sum[drawn] / ref['sum'][drawn]):.3e}")
    assert share >= 0.5
    assert (tol_sum[drawn] > 0).all() and (tol_max[drawn] > 0).all() and (tol_max <= tol_sum + 1e-300).all()


def test_reference_undecided_share(synthetic):
    import removal_ref
    frame, ref = synthetic
    share = removal_ref.undecided_mask(ref).mean()
    print(f"pixels with an undecided pair or T_end < 2^-13: {100 * share:.2f} %")
    assert share <= 0.02
    assert (ref["und"] > 0).any() and int(ref["U"].sum()) > 0   # ... and the reference reports them per Gaussian
    masked = removal_ref.removal_f64(frame, W, H, 2 * N, BG, E=(~removal_ref.undecided_mask(ref)).astype(np.float32))
    assert int(masked["U"].sum()) == 0 and int(masked["band"].sum()) == 0
