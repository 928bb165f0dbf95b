"""Cost of one image comparison (ws_metrics_add: k_image_metrics + k_metrics_finalize) at 1920x1080, f16 against f16, beside the k_blend of the same hd1m frame.

Two rendered views of the hd1m workload of bench.py (Rgba16Float targets) are compared.  Alternating arms for REPS repetitions,
medians:
  * arm "blend":   prepare + render of the hd1m frame with per-kernel timers (enable_timers(2)): k_blend's median over the frames
  * arm "metrics": BATCH comparisons enqueued back to back on one stream into one accumulator, one sync: wall time / BATCH is the
                   device time of one add (main kernel + the one-workgroup sum behind it; launches overlap the kernels), plain and
                   with WS_METRICS_QUANTIZE_U8, and with the SSIM map written
--parent-lib PATH: k_blend is measured once more in a child process that loads another build of the library (the parent
commit's, through WEBSPLAT_LIB) -- this change does not touch the blend, and this is the record of it.
A record, not a gate.  Writes profiles/metrics/metrics_cost.json.

    python scripts/metrics_cost.py [--reps 5] [--frames 40] [--batch 200] [--parent-lib path/to/libwebsplat_hip.so]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "web-splat_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402

import bench  # noqa: E402
import websplat as ws  # noqa: E402


def blend_arm(ctx, pc, views, compressed, sh_deg, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba16float", sh_deg, compressed)
    try:
        for i in range(warmup):
            r.prepare(pc, views[0])
            r.render(pc)
        ctx.sync()
        r.enable_timers(2)
        blend = []
        for i in range(frames):
            r.prepare(pc, views[0])
            r.render(pc)
            ctx.sync()
            blend += [ms for name, ms in r.kernel_times() if name == "k_blend"]
        assert r.frame_stats()["overflow"] == 0 and blend
        return float(np.median(blend))
    finally:
        r.close()


def metrics_arm(ctx, va, vb, w, h, batch, **kw):
    m = ws.Metrics(ctx, batch)
    d_map = ctx.malloc(w * h * 4) if kw.pop("ssim_map", False) else None
    try:
        from websplat import _lib as L
        import ctypes as C
        ca, cb = va.to_c(), vb.to_c()
        flags = L.WS_METRICS_QUANTIZE_U8 if kw.get("quantize_u8") else 0

        def add():  # (the C entry point directly: one map plane reused by every add of the batch)
            ws.check(ws.lib.ws_metrics_add(m.handle, C.byref(ca), C.byref(cb), w, h, flags, C.c_void_p(d_map or 0), w * 4 if d_map else 0, None))

        for _ in range(3):
            add()
        ctx.sync()
        m.reset()
        t0 = time.perf_counter()
        for _ in range(batch):
            add()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / batch
        rec = m.download()[0]
        return ms, rec
    finally:
        m.close()
        if d_map:
            ctx.free(d_map)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--blend-only", action="store_true", help="(child mode) print k_blend's median as JSON and leave")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "metrics_cost.json"))
    a = ap.parse_args()
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        gpc, views, (w, h), _ = bench.build_workload(ws, "hd1m", 16)
        pc = ws.PointCloud(ctx, gpc)
        compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
        if a.blend_only:
            reps = [blend_arm(ctx, pc, views, compressed, sh_deg, a.frames, a.warmup) for _ in range(a.reps)]
            print("BLEND_ONLY " + json.dumps({"k_blend_ms": float(np.median(reps)), "reps": reps, "lib": ws.LIB_PATH}))
            pc.close()
            return
        # the two images: views 0 and 1 of the workload, Rgba16Float
        r = ws.GaussianRenderer(ctx, "rgba16float", sh_deg, compressed)
        targets = [ctx.malloc(w * h * 8) for _ in range(2)]
        for t, v in zip(targets, views[:2]):
            r.prepare(pc, v)
            r.render(pc, t, w * 8)
        ctx.sync()
        assert r.errors()[0] == 0
        r.close()
        va, vb = (ws.ImageView(t, "rgba16float", w * 8, (0.0, 0.0, 0.0)) for t in targets)
        arms = {"blend": [], "metrics": [], "metrics_quantize_u8": [], "metrics_with_map": []}
        rec = None
        for rep in range(a.reps):  # alternating arms
            order = ("blend", "metrics") if rep % 2 == 0 else ("metrics", "blend")
            for arm in order:
                if arm == "blend":
                    arms["blend"].append(blend_arm(ctx, pc, views, compressed, sh_deg, a.frames, a.warmup))
                else:
                    ms, rec = metrics_arm(ctx, va, vb, w, h, a.batch)
                    arms["metrics"].append(ms)
                    arms["metrics_quantize_u8"].append(metrics_arm(ctx, va, vb, w, h, a.batch, quantize_u8=True)[0])
                    arms["metrics_with_map"].append(metrics_arm(ctx, va, vb, w, h, a.batch, ssim_map=True)[0])
        for t in targets:
            ctx.free(t)
        pc.close()
        med = {k: float(np.median(v)) for k, v in arms.items()}
        result = {"what": __doc__.splitlines()[0], "viewport": [w, h], "formats": "rgba16float / rgba16float, over black",
                  "reps": a.reps, "frames": a.frames, "batch": a.batch, "device": ctx.device_info(),
                  "k_blend_ms": med["blend"], "metrics_add_ms": med["metrics"], "metrics_add_quantize_u8_ms": med["metrics_quantize_u8"],
                  "metrics_add_with_map_ms": med["metrics_with_map"], "metrics_add_over_k_blend": med["metrics"] / med["blend"],
                  "bytes_read_per_add": 2 * w * h * 8, "effective_read_GBps": 2 * w * h * 8 / (med["metrics"] * 1e-3) / 1e9,
                  "record": rec, "arms": arms}
    finally:
        ctx.close()
    if a.parent_lib:
        env = dict(os.environ, WEBSPLAT_LIB=os.path.abspath(a.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--blend-only", "--reps", str(a.reps), "--frames", str(a.frames),
                              "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, check=True, timeout=300).stdout
        line = [ln for ln in out.splitlines() if ln.startswith("BLEND_ONLY ")][-1]
        parent = json.loads(line[len("BLEND_ONLY "):])
        result["parent_library"] = {"k_blend_ms": parent["k_blend_ms"], "reps": parent["reps"]}
        result["metrics_add_over_parent_k_blend"] = result["metrics_add_ms"] / parent["k_blend_ms"]
    print(json.dumps({k: v for k, v in result.items() if k != "arms"}, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
