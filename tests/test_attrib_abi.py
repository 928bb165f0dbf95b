"""CPU tests of the attribution ABI (include/websplat.h "Attributing a pixel plane to Gaussians"): declared, exported, bound,
usable from C99, ws_plane_view's layout shared with the Python stub, null handles and bad arguments refused before any device
call; and tests/attrib_ref.py against tests/contrib_ref.py on a synthetic frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ws_renderer_accumulate_weighted", "ws_image_error_plane", "ws_scene_accumulate_error")


def test_attrib_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"typedef struct ws_plane_view \{[^}]*\} ws_plane_view;", code)
    for name, value in (("WS_ERROR_SQ", 0), ("WS_ERROR_ABS", 1), ("WS_ERROR_DSSIM", 2)):
        assert re.search(rf"#define {name}\s+{value}\b", code), name
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert (_lib.WS_ERROR_SQ, _lib.WS_ERROR_ABS, _lib.WS_ERROR_DSSIM) == (0, 1, 2)
    # additive: the ABI version stays where it was
    assert ws.lib.ws_abi_version() == 3
    for name in ("image_error_plane", "accumulate_error_scene"):
        assert hasattr(ws, name)
    assert hasattr(ws.GaussianRenderer, "accumulate_weighted")


def test_attrib_entry_points_compile_as_c99_and_plane_view_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){n}," for n in NEW_ENTRY_POINTS]
    src += ["  };", "  ws_plane_view v;", "  (void)v;",
            '  printf("%d %d %d %d %d %d %d %d %d\\n", (int)(sizeof p / sizeof p[0]), WS_ERROR_SQ, WS_ERROR_ABS, WS_ERROR_DSSIM,',
            "         (int)sizeof(ws_plane_view), (int)offsetof(ws_plane_view, d_values), (int)offsetof(ws_plane_view, row_pitch_bytes),",
            "         (int)offsetof(ws_plane_view, scale), (int)offsetof(ws_plane_view, bias));", "  return 0;", "}"]
    c = tmp_path / "attrib_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "attrib_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    V = _lib.ws_plane_view
    assert out == [str(x) for x in (len(NEW_ENTRY_POINTS), 0, 1, 2, C.sizeof(V), V.d_values.offset, V.row_pitch_bytes.offset,
                                    V.scale.offset, V.bias.offset)]
    assert (C.sizeof(V), V.row_pitch_bytes.offset, V.scale.offset, V.bias.offset) == (24, 8, 16, 20)


def test_attrib_entry_points_refuse_null_and_invalid_arguments(ws):
    """Refused before anything touches a device: this tier has none."""
    from websplat import _lib as L
    lib = ws.lib
    pv = L.ws_plane_view()
    assert lib.ws_renderer_accumulate_weighted(None, None, None, None, None) == L.WS_ERR_INVALID
    assert b"ws_renderer_accumulate_weighted" in lib.ws_last_error()
    assert lib.ws_renderer_accumulate_weighted(None, None, None, C.byref(pv), None) == L.WS_ERR_INVALID
    iv = L.ws_image_view()
    assert lib.ws_image_error_plane(None, None, None, 0, 0, 0, 0, None, 0, None) == L.WS_ERR_INVALID
    assert b"ws_image_error_plane" in lib.ws_last_error()
    assert lib.ws_image_error_plane(None, C.byref(iv), C.byref(iv), 4, 4, L.WS_ERROR_SQ, 0, None, 16, None) == L.WS_ERR_INVALID
    assert lib.ws_scene_accumulate_error(None, None, None, L.WS_SPLIT_TEST, None, None, L.WS_ERROR_SQ, 0, None, None, None) == L.WS_ERR_INVALID
    assert b"ws_scene_accumulate_error" in lib.ws_last_error()
    n = C.c_uint32(7)
    assert lib.ws_scene_accumulate_error(None, None, None, L.WS_SPLIT_TEST, None, b"/nowhere", L.WS_ERROR_DSSIM, 0, None, None,
                                         C.byref(n)) == L.WS_ERR_INVALID


def _synthetic_frame(n, width, height, seed):
    """Splat records (10 halves: the 2 x 2 screen matrix, the centre in NDC, colour, alpha), a draw order and source indices."""
    rng = np.random.default_rng(seed)
    h = np.zeros((n, 10), dtype=np.float16)
    s = rng.uniform(3.0, 12.0, size=(n, 2))          # pixels
    th = rng.uniform(0, np.pi, size=n)
    m00, m01 = s[:, 0] * np.cos(th) / width, -s[:, 1] * np.sin(th) / width
    m10, m11 = s[:, 0] * np.sin(th) / height, s[:, 1] * np.cos(th) / height
    h[:, 0], h[:, 2], h[:, 1], h[:, 3] = m00, m01, -m10, -m11
    h[:, 4:6] = rng.uniform(-1.1, 1.1, size=(n, 2))
    h[:, 6:9] = rng.uniform(0, 1, size=(n, 3))
    h[:, 9] = rng.uniform(0.05, 1.0, size=n)
    return {"splats": h.view(np.uint8).reshape(n, 20), "sorted": rng.permutation(n).astype(np.uint32),
            "src_index": rng.permutation(2 * n)[:n].astype(np.uint32)}


def test_reference_with_unit_plane_is_the_contribution_reference():
    """attrib_ref restates contrib_ref's walk: with E == 1 every field agrees exactly; with a 0/1 mask and its complement the two
    sums add up to it; a zero plane gives zeros."""
    import attrib_ref
    import contrib_ref
    W, H, n = 64, 48, 300
    frame = _synthetic_frame(n, W, H, 5)
    plain = contrib_ref.contrib_f64(frame, W, H, 2 * n)
    assert (plain["sum"] > 0).sum() > 100 and (plain["P"] > 0).any()
    one = attrib_ref.attrib_f64(frame, W, H, 2 * n, np.ones((H, W), np.float32))
    for k in ("sum", "max", "kept", "P", "U", "T"):
        assert np.array_equal(one[k], plain[k]), k
    mask = np.zeros((H, W), np.float32)
    mask[9:30, 13:41] = 1
    a = attrib_ref.attrib_f64(frame, W, H, 2 * n, mask)
    b = attrib_ref.attrib_f64(frame, W, H, 2 * n, 1 - mask)
    assert np.allclose(a["sum"] + b["sum"], plain["sum"], rtol=1e-12, atol=0)
    assert np.array_equal(np.maximum(a["max"], b["max"]), plain["max"])
    assert np.array_equal(a["kept"] + b["kept"], plain["kept"]) and np.array_equal(a["P"] + b["P"], plain["P"])
    zero = attrib_ref.attrib_f64(frame, W, H, 2 * n, np.zeros((H, W), np.float32))
    assert not zero["sum"].any() and not zero["kept"].any() and np.array_equal(zero["T"], plain["T"])
    # the clamp: NaN -> 0, +-inf and values outside [0, 1] to the ends
    e = attrib_ref.clamp_plane(np.array([[-1, 2, np.nan, np.inf, -np.inf, 0.25]], np.float32))
    assert e.tolist() == [[0, 1, 0, 1, 0, 0.25]]
    assert attrib_ref.clamp_plane(np.array([[0.2, 1.0]], np.float32), -0.5, 0.5).tolist() == [[np.float32(0.4), 0.0]]
