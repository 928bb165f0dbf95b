"""CPU tests of the geometry gradient ABI (include/websplat.h "Geometry gradients"): declared, exported, bound, usable from C99,
the descriptor's layout shared with the Python stub, and every descriptor error refused before any handle is looked at."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ws_geomgrad_create", "ws_geomgrad_destroy", "ws_geomgrad_reset", "ws_geomgrad_num_points", "ws_geomgrad_frames",
           "ws_geomgrad_download", "ws_geomgrad_add", "ws_renderer_accumulate_geometry_gradient", "ws_geom_spread_rows", "ws_scene_accumulate_geometry_gradient")
FIELDS = ("background", "scale", "geometry_scale", "reserved0", "d_grad", "grad_pitch_bytes", "d_base", "base_pitch_bytes", "reserved")


def test_geometry_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    assert header.index("---- SH gradients:") < header.index("---- Geometry gradients:") < header.index("Refitting colour and opacity:")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared
    assert re.search(r"typedef struct ws_geometry_params \{[^}]*\} ws_geometry_params;", code)
    assert re.search(r"typedef struct ws_geomgrad ws_geomgrad;", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3   # additive: the ABI version stays where it was
    assert callable(ws.geom_spread_rows) and callable(ws.accumulate_geometry_gradient_scene)
    assert all(hasattr(ws.GeomGrad, m) for m in ("download", "add", "reset", "frames", "close", "num_points"))
    assert hasattr(ws.GaussianRenderer, "accumulate_geometry_gradient")
    assert not any("GaussianSums" in s for s in exported)   # the store's members stay hidden (gaussian_sums.h)


def test_geometry_entry_points_compile_as_c99_and_descriptor_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){name}," for name in ENTRIES]
    src += ["  };", "  ws_geometry_params v; (void)v;", "  int ok = 1; for (unsigned i = 0; i < sizeof p / sizeof p[0]; ++i) ok &= p[i] != 0;",
            '  printf("%d", ok);', '  printf(" %d %d", (int)sizeof(ws_geometry_params), (int)sizeof(ws_gradient_params));']
    src += [f'  printf(" %d", (int)offsetof(ws_geometry_params, {f}));' for f in FIELDS]
    src += ['  printf("\\n");', "  return 0;", "}"]
    c = tmp_path / "geometry_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "geometry_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.ws_geometry_params
    assert out == [1, C.sizeof(P), C.sizeof(_lib.ws_gradient_params)] + [getattr(P, f).offset for f in FIELDS]
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] == [72, 0, 12, 16, 20, 24, 32, 40, 48, 56]
    # ws_gradient_params plus geometry_scale, in opacity_scale's place: every other member where it was
    Q = _lib.ws_gradient_params
    assert all(getattr(P, f).offset == getattr(Q, f).offset for f in FIELDS if f != "geometry_scale") and P.geometry_scale.offset == Q.opacity_scale.offset


def test_geometry_entry_points_refuse_without_a_device(ws):
    """Everything that can be judged from a descriptor alone is refused before the handles are looked at: this tier has no device,
    so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib
    inf, nan = float("inf"), float("nan")
    plane = (C.c_float * 64)()                              # 16-B aligned by ctypes' allocator? not promised: aligned below
    addr = (C.addressof(plane) + 15) & ~15

    def params(scale=1.0, geometry_scale=1.0, background=(0.0, 0.0, 0.0), reserved0=0, reserved=(0, 0, 0, 0), d_grad=addr, pitch=64,
               d_base=None, base_pitch=0):
        p = L.ws_geometry_params()
        p.scale, p.geometry_scale, p.reserved0 = scale, geometry_scale, reserved0
        for i in range(3):
            p.background[i] = background[i]
        for i, w in enumerate(reserved):
            p.reserved[i] = w
        p.d_grad, p.grad_pitch_bytes, p.d_base, p.base_pitch_bytes = d_grad, pitch, d_base, base_pitch
        return p

    def call(p):
        rc = lib.ws_renderer_accumulate_geometry_gradient(None, None, None, C.byref(p) if p is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and b"ws_renderer_accumulate_geometry_gradient" in msg, (rc, msg)
        return msg

    assert b"null params" in call(None)
    assert b"null argument" in call(params())
    for bad in (0.0, -1.0, inf, nan):
        assert b"geometry_scale" in call(params(geometry_scale=bad))
        assert b"scale must be finite" in call(params(scale=bad)) and b"geometry_scale" not in call(params(scale=bad))
    for bad in (inf, nan):
        assert b"background" in call(params(background=(0.0, bad, 0.0)))
    assert b"reserved" in call(params(reserved0=1))
    for i in range(4):
        assert b"reserved" in call(params(reserved=tuple(int(k == i) for k in range(4))))
    assert b"null d_grad" in call(params(d_grad=None))
    assert b"multiples of 16" in call(params(d_grad=addr + 4)) and b"multiples of 16" in call(params(pitch=72))
    assert b"d_base" in call(params(d_base=addr + 8, base_pitch=64)) and b"d_base" in call(params(d_base=addr, base_pitch=24))
    # the handle's own entry points
    h = C.c_void_p()
    assert lib.ws_geomgrad_create(None, 10, C.byref(h)) == L.WS_ERR_INVALID and b"ws_geomgrad_create" in lib.ws_last_error()
    assert lib.ws_geomgrad_reset(None, None) == L.WS_ERR_INVALID and b"null accumulator" in lib.ws_last_error()
    assert lib.ws_geomgrad_download(None, 0, None, None, None, None) == L.WS_ERR_INVALID and b"ws_geomgrad_download" in lib.ws_last_error()
    assert lib.ws_geomgrad_add(None, None, None, None, None, 0) == L.WS_ERR_INVALID and b"ws_geomgrad_add" in lib.ws_last_error()
    assert lib.ws_geomgrad_num_points(None) == 0 and lib.ws_geomgrad_frames(None) == 0
    lib.ws_geomgrad_destroy(None)
    # the host twin
    cu, rs = L.ws_camera_uniform(), L.ws_settings_uniform()
    assert lib.ws_geom_spread_rows(None, None, None, None, None, C.byref(rs), 1.0, 0, None, None, None, None) == L.WS_ERR_INVALID
    assert lib.ws_geom_spread_rows(None, None, None, None, C.byref(cu), C.byref(rs), 1.0, 1, None, None, None, None) == L.WS_ERR_INVALID
    assert b"null argument" in lib.ws_last_error()
    assert lib.ws_geom_spread_rows(None, None, None, None, C.byref(cu), C.byref(rs), 0.0, 0, None, None, None, None) == L.WS_ERR_INVALID
    assert b"geometry_scale" in lib.ws_last_error()
    assert lib.ws_geom_spread_rows(None, None, None, None, C.byref(cu), C.byref(rs), 1.0, 0, None, None, None, None) == L.WS_OK   # no rows
