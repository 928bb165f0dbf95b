"""CPU tests of saving a point cloud (include/websplat.h "Saving a point cloud"): the ABI, the host twin ws_ply_rows_encode against
its inverse ws_ply_rows_convert and against the float64 definition (tests/ply_encode_ref.py), and the file writer ws_ply_write
against the reader ws_ply_read and against websplat.synth.write_ply."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ply_encode_ref as per
import ply_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ws_pointcloud_encode_ply_rows", "ws_pointcloud_save_ply", "ws_ply_write", "ws_ply_rows_encode",
           "ws_pointcloud_encode_ply_rows_device", "ws_pointcloud_decode_ply_rows_device")
F = np.float32
DEGREES = (0, 1, 2, 3)


def _encode(ws, g, s, sh_deg):
    return ws.encode_ply_rows(g, s, sh_deg)


def _decode(ws, rows, sh_deg):
    n = rows.shape[0]
    g, s = np.empty((n, 28), np.uint8), np.empty((n, 96), np.uint8)
    ws.check(ws.lib.ws_ply_rows_convert(rows.ctypes.data_as(C.c_void_p), n, sh_deg, g.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
    return g, s


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_save_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    assert header.index("Refitting colour and opacity:") < header.index("Saving a point cloud:") < header.index("---- view batches")
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared
    assert re.search(r"#define WS_ABI_VERSION 3\b", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in ENTRIES:
        assert name in exported and name in _lib.SIGNATURES
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ws.lib.ws_abi_version() == 3   # additive: the ABI version stays where it was
    assert callable(ws.write_ply_rows) and callable(ws.encode_ply_rows) and all(hasattr(ws.PointCloud, m) for m in ("to_ply_rows", "save_ply", "encode_ply_rows_device", "decode_ply_rows_device"))


def test_save_entry_points_compile_as_c99(tmp_path):
    src = ["#include <stdio.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){name}," for name in ENTRIES]
    src += ["  };", "  int ok = 1; for (unsigned i = 0; i < sizeof p / sizeof p[0]; ++i) ok &= p[i] != 0;",
            "  ok &= ws_pointcloud_save_ply(0, 0) == WS_ERR_INVALID && ws_pointcloud_encode_ply_rows(0, 0, 0) == WS_ERR_INVALID;",
            "  ok &= ws_ply_write(0, 0, 0, 3, 0) == WS_ERR_INVALID && ws_ply_rows_encode(0, 0, 1, 3, 0) == WS_ERR_INVALID;",
            '  printf("%d\\n", ok);', "  return 0;", "}"]
    c = tmp_path / "save_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "save_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["1"]


def test_host_refusals(ws, tmp_path):
    from websplat import _lib as L
    lib = ws.lib
    rows = np.zeros((1, 62), F)
    assert lib.ws_ply_rows_encode(None, None, 1, 3, None) == L.WS_ERR_INVALID and b"ws_ply_rows_encode" in lib.ws_last_error()
    g, s = np.zeros((1, 28), np.uint8), np.zeros((1, 96), np.uint8)
    assert lib.ws_ply_rows_encode(g.ctypes.data, s.ctypes.data, 1, 4, rows.ctypes.data) == L.WS_ERR_UNSUPPORTED
    assert lib.ws_ply_rows_encode(None, None, 0, 3, None) == L.WS_OK
    assert lib.ws_ply_write(None, rows.ctypes.data, 1, 3, None) == L.WS_ERR_INVALID and b"ws_ply_write" in lib.ws_last_error()
    assert lib.ws_ply_write(str(tmp_path / "a.ply").encode(), None, 1, 3, None) == L.WS_ERR_INVALID
    assert lib.ws_ply_write(str(tmp_path / "a.ply").encode(), rows.ctypes.data, 1, 4, None) == L.WS_ERR_UNSUPPORTED
    assert not (tmp_path / "a.ply").exists()
    assert lib.ws_pointcloud_encode_ply_rows(None, rows.ctypes.data, rows.nbytes) == L.WS_ERR_INVALID
    assert lib.ws_pointcloud_save_ply(None, b"x.ply") == L.WS_ERR_INVALID and b"ws_pointcloud_save_ply" in lib.ws_last_error()
    assert lib.ws_pointcloud_encode_ply_rows_device(None, None, 0, None) == L.WS_ERR_INVALID and b"encode_ply_rows_device" in lib.ws_last_error()
    assert lib.ws_pointcloud_decode_ply_rows_device(None, None, 0, None) == L.WS_ERR_INVALID and b"decode_ply_rows_device" in lib.ws_last_error()


# ---- the host twin against its inverse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_deg", DEGREES)
@pytest.mark.parametrize("name", per.CLOUDS + ("edges",))
def test_rows_encode_then_convert_gives_the_cloud_back(ws, name, sh_deg):
    g0, s0 = per.blobs(name, sh_deg)
    rows = _encode(ws, g0, s0, sh_deg)
    assert rows.shape == (g0.shape[0], ply_rows.row_len(sh_deg)) and rows.dtype == F
    g1, s1 = _decode(ws, rows, sh_deg)
    out = per.round_trip(g0, s0, g1, s1, label=f"{name} deg {sh_deg}")
    if name != "edges":
        assert name == "flat" or out["margin_rows"] > 1000                       # (the cap is not vacuous; flat has no such row)
    per.tail_is_sound(rows, g0, s0, sh_deg)


@pytest.mark.parametrize("name", per.CLOUDS + ("edges",))
def test_log_columns_agree_with_the_float64_definition(ws, name):
    """Logits everywhere, log-scales where the eigenvalues are separated (there the Jacobi and eigh agree far inside an f32 ulp):
    within 1 f32 ulp, as sorted triples.  Everything that is not computed -- positions, normals, SH -- is equal bit for bit."""
    sh_deg = 3
    g0, s0 = per.blobs(name, sh_deg)
    rows, ref = _encode(ws, g0, s0, sh_deg), per.encode_ref(g0, s0, sh_deg)
    t = ply_rows.tail_col(sh_deg)
    head, head_ref = rows[:, :t].view(np.uint32), ref[:, :t].view(np.uint32)
    nan = np.isnan(rows[:, :t]) & np.isnan(ref[:, :t])
    assert ((head == head_ref) | nan).all()
    u_op = per.ulps_f32(rows[:, t], ref[:, t])
    _, _, cov, _ = per.split(g0, s0)
    sep = per.separated(cov)
    u_sc = per.ulps_f32(np.sort(rows[sep, t + 1:t + 4], axis=1), np.sort(ref[sep, t + 1:t + 4], axis=1))
    print(f"{name}: logits at most {u_op.max():.2f} ulp apart; {int(sep.sum())} separated rows, log-scales at most {u_sc.max() if sep.any() else 0:.2f} ulp apart")
    assert u_op.max() <= 1.0
    if name != "flat" and name != "edges":
        assert sep.sum() > 1000
    assert not sep.any() or u_sc.max() <= 1.0


def test_edges_are_deterministic_and_as_stated(ws):
    sh_deg = 3
    g0, s0 = per.blobs("edges", sh_deg)
    a, b = _encode(ws, g0, s0, sh_deg), _encode(ws, g0, s0, sh_deg)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _, op, cov, _ = per.split(g0, s0)
    t = ply_rows.tail_col(sh_deg)
    # the logits of the stated cases
    stated = {0x0000: per.FLOOR, 0x8000: per.FLOOR, 0x3C00: per.CEIL, 0x3E00: per.CEIL, 0x7BFF: per.CEIL, 0xB800: per.FLOOR, 0x3800: 0.0}
    for half, want in stated.items():
        assert (a[op == half, t] == F(want)).all(), hex(half)
    assert np.isnan(a[ply_rows.is_nan_half(op), t]).all()
    assert np.isfinite(a[op == 0x0001, t]).all() and np.isfinite(a[op == 0x3BFF, t]).all()
    # a covariance with a half that is not finite: identity quaternion, scales from the diagonal by the rule
    bad = ~per.finite_cov(cov)
    assert bad.sum() == (len(per.COVARIANCES) - per.N_FINITE_COV) * len(per.OPACITY_HALVES)
    assert np.array_equal(a[bad, t + 4:t + 8], np.tile(np.array([1, 0, 0, 0], F), (int(bad.sum()), 1)))
    want = per.log_scale(per.nonfinite_extents(cov[bad])).astype(F)
    assert per.ulps_f32(a[bad, t + 1:t + 4], want).max() <= 1.0 and np.isfinite(a[bad, t + 1:t + 8]).all()
    assert np.array_equal(a[bad, t + 1:t + 4] == F(per.FLOOR), want == F(per.FLOOR))
    # zero and negative extents are written as -20
    zero = (cov == 0).all(axis=1)
    assert (a[zero, t + 1:t + 4] == F(per.FLOOR)).all()
    lam = per.eigenvalues(cov)
    fin = per.finite_cov(cov)
    floors = (a[fin, t + 1:t + 4] == F(per.FLOOR)).sum(axis=1)               # (the eigenvalues are not sorted: count them)
    assert ((lam[fin] < -1e-3).sum(axis=1) <= floors).all() and (floors <= (lam[fin] < 1e-9).sum(axis=1)).all()
    assert (lam[fin] < -1e-3).any()
    # a cloud saved twice is stable: encode(decode(encode(x))) == encode(decode(x)) on the rows whose covariance came back identical
    g1, s1 = _decode(ws, a, sh_deg)
    g2, s2 = _decode(ws, _encode(ws, g1, s1, sh_deg), sh_deg)
    fin = per.finite_cov(cov)
    assert np.array_equal(per.split(g1, s1)[2][fin], per.split(g2, s2)[2][fin])


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
METAS = (dict(), dict(kernel_size=0.1), dict(mip_splatting=True), dict(mip_splatting=False, kernel_size=1.0 / 3.0, background_color=(0.1, 1e-8, 3.0e38)),
         dict(background_color=(0.0, 1.0, 0.5)), dict(kernel_size=1.17549435e-38, mip_splatting=True, background_color=(1.0 / 3.0, 2.0 / 3.0, 1e-45)))


@pytest.mark.parametrize("sh_deg", DEGREES)
def test_write_then_read(ws, tmp_path, sh_deg):
    from websplat import synth
    rows = synth.scene_c1(n=257, seed=3 + sh_deg, sh_deg=sh_deg)
    rows[:, 3:6] = 0.0
    want_g, want_s = _decode(ws, rows, sh_deg)
    for k, meta in enumerate(METAS):
        p = tmp_path / f"m{k}.ply"
        ws.write_ply_rows(str(p), rows, sh_deg, **meta)
        raw = p.read_bytes()
        body = raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
        assert body == rows.astype("<f4").tobytes()                                   # the rows survive byte for byte
        pc = ws.read_ply(str(p))
        assert pc.num_points == 257 and pc.sh_deg == sh_deg
        assert np.array_equal(pc.gaussians, want_g) and np.array_equal(pc.sh_coefs, want_s)
        assert pc.mip_splatting == meta.get("mip_splatting")
        ks = meta.get("kernel_size")
        assert (pc.kernel_size is None) if ks is None else (F(pc.kernel_size) == F(ks))
        bg = meta.get("background_color")
        assert (pc.background_color is None) if bg is None else np.array_equal(np.array(pc.background_color, F), np.array(bg, F))
        assert raw.count(b"comment ") == len(meta)


def test_write_empty_unwritable_and_synth_identity(ws, tmp_path):
    from websplat import _lib as L
    from websplat import synth
    p = tmp_path / "empty.ply"
    ws.write_ply_rows(str(p), np.zeros((0, 62), F), 3, kernel_size=0.25)
    pc = ws.read_ply(str(p))
    assert pc.num_points == 0 and pc.sh_deg == 3 and pc.kernel_size == 0.25 and p.read_bytes().endswith(b"end_header\n")
    rows = synth.scene_c1(n=100, seed=9, sh_deg=2)
    bad = tmp_path / "no_such_directory" / "x.ply"
    with pytest.raises(ws.WebSplatError) as e:
        ws.write_ply_rows(str(bad), rows, 2)
    assert e.value.code == L.WS_ERR_IO and not bad.exists() and not bad.parent.exists()
    with pytest.raises(ValueError):
        ws.write_ply_rows(str(tmp_path / "y.ply"), rows, 3)
    for sh_deg in DEGREES:
        rows = synth.scene_c1(n=65, seed=sh_deg, sh_deg=sh_deg)
        a, b = tmp_path / f"a{sh_deg}.ply", tmp_path / f"b{sh_deg}.ply"
        synth.write_ply(str(a), rows, sh_deg)
        ws.write_ply_rows(str(b), rows, sh_deg)
        assert a.read_bytes() == b.read_bytes()
