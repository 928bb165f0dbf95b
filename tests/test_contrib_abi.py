"""CPU tests of the contribution ABI (include/websplat.h "Per-Gaussian contributions"): declared, exported, bound, usable from
C99, null handles refused; and shard.reduce_contrib over a two-rank gloo group."""
import os
import re
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ws_contrib_create", "ws_contrib_destroy", "ws_contrib_reset", "ws_contrib_num_points", "ws_contrib_frames",
                    "ws_renderer_enable_contrib", "ws_renderer_accumulate_contrib", "ws_contrib_download", "ws_contrib_add",
                    "ws_pointcloud_create_subset", "ws_scene_accumulate_contrib")


def test_contrib_entry_points_declared_exported_and_bound(ws):
    header = open(os.path.join(ROOT, "include", "websplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"typedef struct ws_contrib ws_contrib;", code)
    assert re.search(r"#define WS_CONTRIB_SUM_SCALE 4294967296\.0", code)
    from websplat import _lib
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.split()}
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(ws.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.WS_CONTRIB_SUM_SCALE == 2.0 ** 32
    # additive: the ABI version stays where it was
    assert ws.lib.ws_abi_version() == 3
    for name in ("Contrib", "accumulate_contrib_scene"):
        assert hasattr(ws, name)
    assert hasattr(ws.PointCloud, "subset") and hasattr(ws.GaussianRenderer, "enable_contrib")
    assert hasattr(ws.GaussianRenderer, "accumulate_contrib")


def test_contrib_entry_points_compile_as_c99(tmp_path):
    src = ["#include <stdio.h>", '#include "websplat.h"', "int main(void) {", "  void* p[] = {"]
    src += [f"    (void*){n}," for n in NEW_ENTRY_POINTS]
    src += ["  };", "  ws_contrib* c = 0;", "  (void)c;",
            '  printf("%d %.1f\\n", (int)(sizeof p / sizeof p[0]), WS_CONTRIB_SUM_SCALE);', "  return 0;", "}"]
    c = tmp_path / "contrib_abi.c"
    c.write_text("\n".join(src))
    from websplat import _lib
    exe = tmp_path / "contrib_abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe),
                    "-L", libdir, "-lwebsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(len(NEW_ENTRY_POINTS)), "4294967296.0"]


def test_contrib_entry_points_refuse_null_handles(ws):
    """Null handles are refused before anything touches a device."""
    from websplat import _lib as L
    lib = ws.lib
    assert lib.ws_contrib_create(None, 10, None) == L.WS_ERR_INVALID
    assert b"ws_contrib_create" in lib.ws_last_error()
    assert lib.ws_contrib_reset(None, None) == L.WS_ERR_INVALID
    assert lib.ws_contrib_num_points(None) == 0 and lib.ws_contrib_frames(None) == 0
    assert lib.ws_renderer_enable_contrib(None, 1) == L.WS_ERR_INVALID
    assert lib.ws_renderer_accumulate_contrib(None, None, None, None) == L.WS_ERR_INVALID
    assert lib.ws_contrib_download(None, 0, None, None) == L.WS_ERR_INVALID
    assert lib.ws_contrib_add(None, None, None, 0) == L.WS_ERR_INVALID
    assert lib.ws_pointcloud_create_subset(None, None, None, 0, None) == L.WS_ERR_INVALID
    assert lib.ws_scene_accumulate_contrib(None, None, None, L.WS_SPLIT_TRAIN, None, None) == L.WS_ERR_INVALID
    assert b"ws_scene_accumulate_contrib" in lib.ws_last_error()
    lib.ws_contrib_destroy(None)  # a no-op


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_arrays(rank, n=1000):
    rng = np.random.default_rng(100 + rank)
    q = rng.integers(0, 1 << 61, n, dtype=np.uint64)
    q[rng.random(n) < 0.3] = 0
    q[0] = (1 << 62) - 1 - rank   # the sum of two ranks stays below 2^63
    m = rng.random(n).astype(np.float32) * np.float32(0.99)
    m[q == 0] = 0
    return q, m


def _worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "web-splat_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from websplat.shard import reduce_contrib
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        sq, mw = _rank_arrays(rank)
        rq, rm = reduce_contrib(sq, mw, dist, "cpu")
        dist.barrier()
        q.put((rank, rq, rm))
    finally:
        dist.destroy_process_group()


def test_reduce_contrib_two_rank_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (q0, m0), (q1, m1) = _rank_arrays(0), _rank_arrays(1)
    want_q, want_m = q0 + q1, np.maximum(m0, m1)
    for _, rq, rm in results:
        assert rq.dtype == np.uint64 and rm.dtype == np.float32
        assert np.array_equal(rq, want_q)
        assert np.array_equal(rm.view(np.uint32), want_m.view(np.uint32))


def test_reduce_contrib_single_process_and_int64_range():
    sys.path.insert(0, os.path.join(ROOT, "web-splat_amd"))
    import pytest
    from websplat.shard import reduce_contrib
    sq, mw = _rank_arrays(0)
    rq, rm = reduce_contrib(sq, mw)  # no process group: the arrays themselves
    assert np.array_equal(rq, sq) and np.array_equal(rm, mw)
    with pytest.raises(OverflowError):
        reduce_contrib(np.array([1 << 63], dtype=np.uint64), np.zeros(1, dtype=np.float32))
