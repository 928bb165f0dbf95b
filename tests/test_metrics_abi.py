"""CPU tests of the image-metrics ABI (include/websplat.h "Image metrics"): declared, exported, bound, usable from C99, struct
sizes shared with the Python stub, null handles refused before any device call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ws_metrics_create", "ws_metrics_destroy", "ws_metrics_reset", "ws_metrics_count", "ws_metrics_add",
                    "ws_metrics_download", "ws_png_read_rgba8", "ws_host_free", "ws_scene_evaluate")


def test_metrics_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"typedef struct ws_metrics ws_metrics;", code)
    assert re.search(r"#define WS_METRICS_QUANTIZE_U8 1u", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.WS_METRICS_QUANTIZE_U8 == 1
    # additive: the ABI version stays where it was
    assert ws.lib.ws_abi_version() == 3
    for name in ("Metrics", "ImageView", "image_metrics", "read_png", "evaluate_scene"):
        assert hasattr(ws, name)
    for name in ("add", "download", "reset", "count", "close", "maps"):
        assert hasattr(ws.Metrics, name)


def test_metrics_entry_points_compile_as_c99_and_struct_sizes_match(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){n}," for n in NEW_ENTRY_POINTS]
    src += ["  };", "  ws_metrics* m = 0;", "  ws_image_view v;", "  ws_image_metrics r;", "  (void)m; (void)v; (void)r;",
            '  printf("%d %u %d %d %d %d %d %d\\n", (int)(sizeof p / sizeof p[0]), WS_METRICS_QUANTIZE_U8, (int)sizeof(ws_image_view),',
            "         (int)sizeof(ws_image_metrics), (int)offsetof(ws_image_view, row_pitch_bytes), (int)offsetof(ws_image_view, background),",
            "         (int)offsetof(ws_image_metrics, sse_u8), (int)offsetof(ws_image_metrics, flags));", "  return 0;", "}"]
    c = tmp_path / "metrics_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "metrics_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    V, R = _lib.ws_image_view, _lib.ws_image_metrics
    assert out == [str(x) for x in (len(NEW_ENTRY_POINTS), 1, C.sizeof(V), C.sizeof(R), V.row_pitch_bytes.offset, V.background.offset,
                                    R.sse_u8.offset, R.flags.offset)]
    assert (C.sizeof(V), C.sizeof(R)) == (40, 48)


def test_metrics_entry_points_refuse_null_handles(ws):
    """Null handles are refused before anything touches a device."""
    from websplat import _lib as L
    lib = ws.lib
    assert lib.ws_metrics_create(None, 4, None) == L.WS_ERR_INVALID
    assert b"ws_metrics_create" in lib.ws_last_error()
    assert lib.ws_metrics_reset(None, None) == L.WS_ERR_INVALID
    assert lib.ws_metrics_count(None) == 0
    v = L.ws_image_view()
    assert lib.ws_metrics_add(None, C.byref(v), C.byref(v), 4, 4, 0, None, 0, None) == L.WS_ERR_INVALID
    assert b"ws_metrics_add" in lib.ws_last_error()
    assert lib.ws_metrics_add(None, None, None, 0, 0, 0, None, 0, None) == L.WS_ERR_INVALID
    assert lib.ws_metrics_download(None, 0, None, None) == L.WS_ERR_INVALID
    assert lib.ws_scene_evaluate(None, None, None, L.WS_SPLIT_TEST, None, None, 0, None, None) == L.WS_ERR_INVALID
    assert b"ws_scene_evaluate" in lib.ws_last_error()
    assert lib.ws_png_read_rgba8(None, None, None, None) == L.WS_ERR_INVALID
    lib.ws_metrics_destroy(None)  # no-ops
    lib.ws_host_free(None)
