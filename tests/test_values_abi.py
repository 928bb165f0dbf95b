"""CPU tests of the value-rendering ABI (include/websplat.h "Rendering per-Gaussian values"): declared, exported, bound, usable
from C99, the two descriptors' layouts shared with the Python stub, bad descriptors and null handles refused before any device
call; and tests/values_ref.py against tests/contrib_ref.py and tests/attrib_ref.py on a synthetic frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ws_renderer_render_values"


def test_values_entry_point_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert ENTRY in set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert re.search(r"typedef struct ws_values_view \{[^}]*\} ws_values_view;", code)
    assert re.search(r"typedef struct ws_value_targets \{[^}]*\} ws_value_targets;", code)
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    assert ENTRY in exported and ENTRY in _lib.SIGNATURES
    assert getattr(ws.lib, ENTRY).argtypes == _lib.SIGNATURES[ENTRY][1]
    # additive: the ABI version stays where it was
    assert ws.lib.ws_abi_version() == 3
    assert hasattr(ws.GaussianRenderer, "render_values") and hasattr(ws.GaussianRenderer, "download_values")


def test_values_entry_point_compiles_as_c99_and_descriptor_layouts(tmp_path):
    fields_v = ("d_values", "stride_bytes", "num_points", "channels")
    fields_t = ("plane", "pitch", "winner", "winner_pitch", "reserved")
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "websplat.h"', "int main(void) {",
           f"  void* p = (void*){ENTRY};", "  ws_values_view v; ws_value_targets t;", "  (void)v; (void)t;",
           '  printf("%d", p != 0);', '  printf(" %d", (int)sizeof(ws_values_view));']
    src += [f'  printf(" %d", (int)offsetof(ws_values_view, {f}));' for f in fields_v]
    src += ['  printf(" %d", (int)sizeof(ws_value_targets));']
    src += [f'  printf(" %d", (int)offsetof(ws_value_targets, {f}));' for f in fields_t]
    src += ['  printf(" %d %d\\n", (int)sizeof t.plane, (int)sizeof t.reserved);', "  return 0;", "}"]
    c = tmp_path / "values_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "values_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    V, T = _lib.ws_values_view, _lib.ws_value_targets
    want = [1, C.sizeof(V)] + [getattr(V, f).offset for f in fields_v] + [C.sizeof(T)] + [getattr(T, f).offset for f in fields_t]
    want += [C.sizeof(C.c_void_p * 4), 16]
    assert out == want
    assert (C.sizeof(V), V.stride_bytes.offset, V.num_points.offset, V.channels.offset) == (24, 8, 16, 20)
    assert (C.sizeof(T), T.pitch.offset, T.winner.offset, T.winner_pitch.offset, T.reserved.offset) == (96, 32, 64, 72, 80)


def test_values_entry_point_refuses_invalid_arguments_without_a_device(ws):
    """Everything that can be judged from the descriptors alone is refused before the handles are looked at: this tier has no
    device, so the handles are null throughout and a descriptor that passes ends at "null argument"."""
    from websplat import _lib as L
    lib = ws.lib
    buf = (C.c_float * 64)()          # host memory standing in for device pointers: nothing dereferences them
    ptr = C.addressof(buf)

    def view(channels=1, stride=None, pointer=ptr, num_points=7):
        v = L.ws_values_view()
        v.d_values, v.stride_bytes, v.num_points, v.channels = pointer, 4 * channels if stride is None else stride, num_points, channels
        return v

    def targets(planes=(0,), pitch=64, winner=False, winner_pitch=64, reserved=(0, 0, 0, 0), pointer=ptr):
        t = L.ws_value_targets()
        for c in planes:
            t.plane[c], t.pitch[c] = pointer, pitch
        if winner:
            t.winner, t.winner_pitch = ptr, winner_pitch
        for i, w in enumerate(reserved):
            t.reserved[i] = w
        return t

    def call(v, t):
        rc = lib.ws_renderer_render_values(None, None, C.byref(v) if v is not None else None, C.byref(t) if t is not None else None, None)
        msg = lib.ws_last_error()
        assert rc == L.WS_ERR_INVALID and ENTRY.encode() in msg, (rc, msg)
        return msg

    assert b"null targets" in call(view(), None)
    assert b"null argument" in call(view(), targets())                          # a good pair: only the handles are wrong
    assert b"null argument" in call(None, targets(planes=(), winner=True))      # winner only, values NULL
    assert b"null argument" in call(view(4, stride=32), targets(planes=(0, 3), winner=True))
    assert b"no output" in call(view(), targets(planes=()))
    assert b"no output" in call(None, targets(planes=()))
    assert b"channels" in call(view(0, stride=4), targets())
    assert b"channels" in call(view(5), targets())
    assert b"number of channels" in call(view(2), targets(planes=(0, 2)))       # a plane at c >= channels
    assert b"number of channels" in call(None, targets(planes=(0,)))            # no values: every plane is above
    assert b"stride" in call(view(3, stride=8), targets())                      # below 4 x channels
    assert b"stride" in call(view(1, stride=6), targets())                      # not a multiple of 4
    assert b"aligned" in call(view(pointer=ptr + 2), targets())
    assert b"d_values" in call(view(pointer=None), targets())
    assert b"multiples of 4" in call(view(), targets(pitch=66))
    assert b"multiples of 4" in call(view(), targets(pointer=ptr + 1))
    assert b"multiples of 4" in call(None, targets(planes=(), winner=True, winner_pitch=30))
    for i in range(4):
        assert b"reserved" in call(view(), targets(reserved=tuple(int(k == i) for k in range(4))))


def _synthetic_frame(n, width, height, seed):
    """test_attrib_abi._synthetic_frame: Splat records (10 halves: the 2 x 2 screen matrix, the centre in NDC, colour, alpha), a
    draw order and source indices."""
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


def test_reference_is_consistent_with_the_contribution_and_attribution_references():
    import attrib_ref
    import contrib_ref
    import values_ref
    W, H, n = 64, 48, 300
    frame = _synthetic_frame(n, W, H, 5)
    plain = contrib_ref.contrib_f64(frame, W, H, 2 * n)
    drawn = np.nonzero(plain["sum"] > 0)[0]
    assert drawn.size > 100
    # f == 1: the drawn mass
    ones = values_ref.values_f64(frame, W, H, np.ones(2 * n, np.float32))
    assert ones["out"].shape == (H, W, 1) and (ones["n"] > 0).sum() > 1000
    assert np.abs(ones["out"][..., 0] - (1.0 - ones["T"])).max() <= 1e-12
    assert np.array_equal(ones["T"], plain["T"]) and int(ones["n"].sum()) == int(plain["kept"].sum())
    assert np.array_equal(ones["win"] >= 0, ones["wmax"] > 0) and (ones["und"] > 0).any()
    # one-hot at j: the plane holds j's weights
    rng = np.random.default_rng(9)
    picks = [int(drawn[np.argmax(plain["sum"][drawn])]), int(drawn[np.argmin(plain["sum"][drawn])])] + [int(j) for j in rng.choice(drawn, 2)]
    f = np.zeros((2 * n, len(picks)), np.float32)
    f[picks, np.arange(len(picks))] = 1
    hot = values_ref.values_f64(frame, W, H, f, watch=np.full((H, W), picks[0]))
    for c, j in enumerate(picks):
        o = hot["out"][..., c]
        assert abs(o.sum() - plain["sum"][j]) <= 1e-12 * plain["sum"][j], j
        assert o.max() == plain["max"][j], j
        assert int((o > 0).sum()) <= plain["kept"][j]
    assert np.array_equal(hot["wwatch"], hot["out"][..., 0])
    assert np.array_equal(hot["win"], ones["win"]) and np.array_equal(hot["wmax"], ones["wmax"])
    # the winner's own weight is the largest one
    w_of_winner = values_ref.values_f64(frame, W, H, np.zeros(2 * n, np.float32), watch=ones["win"])["wwatch"]
    assert np.array_equal(w_of_winner, ones["wmax"])
    # the adjoint identity: <E, A f> == <A^T E, f>
    fv = rng.uniform(0, 1, size=2 * n).astype(np.float32)
    E = rng.uniform(0, 1, size=(H, W)).astype(np.float32)
    E[rng.uniform(size=(H, W)) < 0.3] = 0
    lhs = (E.astype(np.float64) * values_ref.values_f64(frame, W, H, fv)["out"][..., 0]).sum()
    rhs = (fv.astype(np.float64) * attrib_ref.attrib_f64(frame, W, H, 2 * n, E)["sum"]).sum()
    print(f"adjoint: lhs {lhs:.15e} rhs {rhs:.15e}")
    assert rhs > 1 and abs(lhs - rhs) <= 1e-12 * rhs
    # a non-finite value reaches only the pixels its Gaussian reaches
    fn = np.ones(2 * n, np.float32)
    fn[picks[1]] = np.inf
    bad = ~np.isfinite(values_ref.values_f64(frame, W, H, fn)["out"][..., 0])
    assert bad.any() and np.array_equal(bad, hot["out"][..., 1] > 0)
    # the tolerance: non-negative everywhere, the undecided pixels carry their allowance
    tol = values_ref.tolerance(ones, 1.0)
    assert tol.shape == (H, W) and (tol >= 0).all() and (tol[ones["und"] > 0] >= 2 * contrib_ref.CUT_STEP).all()
