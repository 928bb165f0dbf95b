"""CPU tests of the composite ABI (include/websplat.h ws_renderer_render_composite, ws_composite_desc, ws_occluder_kind): declared,
exported, bound; the ctypes mirror agrees with the C header; and a C99 twin of the header's NDC -> view-z expression agrees with
numpy's float32 evaluation of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ws_renderer_render_composite",)


def test_composite_entry_point_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"typedef struct ws_composite_desc\s*\{", code)
    assert re.search(r"WS_OCCLUDER_VIEW_Z\s*=\s*0", code) and re.search(r"WS_OCCLUDER_NDC_DEPTH\s*=\s*1", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3  # additive: the ABI version stays


def _probe(tmp_path, name, lines):
    c = tmp_path / f"{name}.c"
    c.write_text("\n".join(["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"'] + lines))
    exe = tmp_path / name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


def test_composite_desc_layout_matches_the_c_header(ws, tmp_path):
    from websplat import _lib
    fields = [n for n, _ in _lib.ws_composite_desc._fields_]
    assert fields == ["load", "occluder_kind", "occluder", "occluder_pitch", "reserved"]
    src = ["int main(void) {", '  printf("sizeof %zu\\n", sizeof(ws_composite_desc));']
    src += [f'  printf("{n} %zu\\n", offsetof(ws_composite_desc, {n}));' for n in fields]
    src += ['  printf("reserved_size %zu\\n", sizeof(((ws_composite_desc*)0)->reserved));',
            '  printf("kinds %d %d\\n", (int)WS_OCCLUDER_VIEW_Z, (int)WS_OCCLUDER_NDC_DEPTH);', "  return 0;", "}"]
    out = dict(line.split(None, 1) for line in _probe(tmp_path, "comp_layout", src).splitlines())
    assert int(out["sizeof"]) == C.sizeof(_lib.ws_composite_desc) == 40
    for n in fields:
        assert int(out[n]) == getattr(_lib.ws_composite_desc, n).offset, n
    assert int(out["reserved_size"]) == C.sizeof(C.c_uint32 * 4)
    assert out["kinds"].split() == [str(_lib.WS_OCCLUDER_VIEW_Z), str(_lib.WS_OCCLUDER_NDC_DEPTH)]


def ndc_to_view_z_f32(d, n, f):
    """The header's expression in numpy float32, in its stated order: (n * f) / (f - d * (f - n)); d >= 1 -> +inf."""
    d = np.asarray(d, dtype=np.float32)
    n, f = np.float32(n), np.float32(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (n * f) / (f - d * (f - n))
    return np.where(d >= np.float32(1.0), np.float32(np.inf), D).astype(np.float32)


def test_ndc_conversion_c99_twin_matches_numpy(tmp_path):
    rng = np.random.default_rng(11)
    cases = [(0.01, 100.0), (0.1, 1000.0), (2.5, 7.25), (1e-3, 1e4)]
    ds = np.concatenate([rng.uniform(0.0, 1.0, 400), [0.0, 0.5, 0.999999, 1.0, 1.5, -0.25]]).astype(np.float32)
    src = ["#include <string.h>", "#include <stdint.h>",
           "static float conv(float d, float n, float f) { return d >= 1.0f ? (float)INFINITY_ : (n * f) / (f - d * (f - n)); }",
           "int main(void) {", "  uint32_t bits; float d, n, f;",
           "  while (scanf(\"%f %f %f\", &d, &n, &f) == 3) { float D = conv(d, n, f); memcpy(&bits, &D, 4); printf(\"%u\\n\", bits); }",
           "  return 0;", "}"]
    src = [s.replace("INFINITY_", "__builtin_inff()") for s in src]
    c = tmp_path / "ndc.c"
    c.write_text("\n".join(["#include <stdio.h>", '#include "websplat.h"'] + src))
    exe = tmp_path / "ndc"
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe)], check=True)
    lines, want = [], []
    for n, f in cases:
        n32, f32 = np.float32(n), np.float32(f)
        for d in ds:
            lines.append(f"{float(d)!r} {float(n32)!r} {float(f32)!r}")
        want.append(ndc_to_view_z_f32(ds, n32, f32))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(x) for x in out], dtype=np.uint32).view(np.float32)
    want = np.concatenate(want)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # d = 0 is the near plane, d -> 1 the far plane
    assert np.allclose(ndc_to_view_z_f32([0.0], 0.1, 100.0), 0.1, rtol=1e-6)


def test_composite_entry_point_checks_its_arguments_without_a_gpu(ws):
    from websplat import _lib as L
    d = L.ws_composite_desc()
    assert ws.lib.ws_renderer_render_composite(None, None, None, None, 0, None, C.byref(d), None) == L.WS_ERR_INVALID
    assert ws.lib.ws_renderer_render_composite(None, None, None, None, 0, None, None, None) == L.WS_ERR_INVALID
