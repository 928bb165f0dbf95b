"""CPU tests of the auxiliary-plane ABI (include/websplat.h ws_renderer_enable_depth / ws_renderer_render_aux /
ws_renderer_download_depths, ws_aux_targets): declared, exported, bound, and the ctypes mirror agrees with the C header."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ws_renderer_enable_depth", "ws_renderer_render_aux", "ws_renderer_download_depths")


def test_aux_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"typedef struct ws_aux_targets\s*\{", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the ABI version stays where it was: the additions are additive
    assert ws.lib.ws_abi_version() == 3


def test_aux_targets_layout_matches_the_c_header(ws, tmp_path):
    from websplat import _lib
    fields = [n for n, _ in _lib.ws_aux_targets._fields_]
    assert fields == ["depth", "depth_pitch", "median_depth", "median_depth_pitch", "alpha", "alpha_pitch", "reserved"]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(ws_aux_targets));']
    src += [f'  printf("{n} %zu\\n", offsetof(ws_aux_targets, {n}));' for n in fields]
    src += ['  printf("reserved_size %zu\\n", sizeof(((ws_aux_targets*)0)->reserved));', "  return 0;", "}"]
    c = tmp_path / "aux_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "aux_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(_lib.ws_aux_targets) == 64
    for n in fields:
        assert int(out[n]) == getattr(_lib.ws_aux_targets, n).offset, n
    assert int(out["reserved_size"]) == C.sizeof(C.c_uint32 * 4)


def test_aux_entry_points_check_their_arguments_without_a_gpu(ws):
    """Null renderers are refused before anything touches a device."""
    from websplat import _lib as L
    assert ws.lib.ws_renderer_enable_depth(None, 1) == L.WS_ERR_INVALID
    assert ws.lib.ws_renderer_render_aux(None, None, None, None, 0, None, None) == L.WS_ERR_INVALID
    assert ws.lib.ws_renderer_download_depths(None, 0, None, None) == L.WS_ERR_INVALID
