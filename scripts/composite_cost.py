"""Cost of compositing over a loaded target behind an occluder (ws_renderer_render_composite) against the colour-only blend.

Per workload (hd1m, c3, c5 of bench.py) and arm, alternating arms for REPS repetitions:
  * one-in-flight frame time: prepare + blend + stream sync per frame, wall clock, median over the frames
  * stage timers and per-kernel times (enable_timers(2)), medians over the frames
Arms:
  colour     render() over the clear colour (depth off)
  load       render_composite(load=True) (depth off)
  load_inf   load + an occluder of +inf everywhere (depth on: the pure cost of staging z and the per-pair test)
  load_half  load + an occluder over the lower half of the screen at the frame's median splat depth (+inf above): the gain of
             the per-tile drop
The occluder planes are device buffers made once per view (the frame's median z from a depth-on prepare).  Writes
profiles/composite/composite_cost.json.

    python scripts/composite_cost.py [--workloads hd1m,c3,c5] [--reps 3] [--frames 60]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "web-splat_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402

import bench  # noqa: E402
import websplat as ws  # noqa: E402

ARMS = ("colour", "load", "load_inf", "load_half")


def occluder_planes(ctx, pc, views, compressed, sh_deg, w, h):
    """{arm: [device pointer per view]} of the two occluded arms."""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    planes = {"load_inf": [], "load_half": []}
    try:
        r.enable_depth(True)
        inf = np.full((h, w), np.inf, dtype=np.float32)
        for v in views:
            r.prepare(pc, v)
            zmed = np.float32(np.median(r.download_depths()))
            half = inf.copy()
            half[h // 2:, :] = zmed
            for arm, img in (("load_inf", inf), ("load_half", half)):
                p = ctx.malloc(w * h * 4)
                ctx.upload(p, img)
                planes[arm].append(p)
    finally:
        r.close()
    return planes


def run_arm(ctx, pc, views, compressed, sh_deg, arm, planes, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    try:
        r.enable_depth(arm in ("load_inf", "load_half"))
        wall, stages, kernels = [], [], {}

        def frame(i):
            k = i % len(views)
            r.prepare(pc, views[k])
            if arm == "colour":
                r.render(pc)
            elif arm == "load":
                r.render_composite(pc, load=True)
            else:
                r.render_composite(pc, load=True, occluder=planes[arm][k])
            ctx.sync()

        for i in range(warmup):
            frame(i)
        for i in range(frames):  # one in flight, no instrumentation
            t0 = time.perf_counter()
            frame(i)
            wall.append((time.perf_counter() - t0) * 1e3)
        r.enable_timers(2)
        for i in range(frames):
            frame(i)
            stages.append(r.stage_times())
            for name, ms in r.kernel_times():
                kernels.setdefault(name, []).append(ms)
        assert r.frame_stats()["overflow"] == 0
        return {
            "frame_ms_median": float(np.median(wall)),
            "stage_ms_median": {k: float(np.median([s[k] for s in stages])) for k in stages[0]},
            "kernel_ms_median": {k: float(np.median(v)) for k, v in kernels.items()},
        }
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="hd1m,c3,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite", "composite_cost.json"))
    a = ap.parse_args()
    ctx = ws.Context(0, ws.config_from_env({}))
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    try:
        for name in a.workloads.split(","):
            gpc, views, (w, h), _ = bench.build_workload(ws, name, 16)
            pc = ws.PointCloud(ctx, gpc)
            compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
            reps = {arm: [] for arm in ARMS}
            planes = {}
            try:
                planes = occluder_planes(ctx, pc, views, compressed, sh_deg, w, h)
                for rep in range(a.reps):  # alternating arms
                    order = ARMS if rep % 2 == 0 else ARMS[::-1]
                    for arm in order:
                        reps[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm, planes, a.frames, a.warmup))
            finally:
                for ps in planes.values():
                    for p in ps:
                        ctx.free(p)
                pc.close()

            def med(arm, f):
                return float(np.median([f(x) for x in reps[arm]]))

            def blend(x):
                return x["kernel_ms_median"].get("k_blend", x["stage_ms_median"]["rasterization"])

            summary = {}
            for label, f in (("frame_ms", lambda x: x["frame_ms_median"]), ("blend_kernel_ms", blend),
                             ("rasterization_stage_ms", lambda x: x["stage_ms_median"]["rasterization"])):
                c = med("colour", f)
                summary[label] = {"colour": c}
                for arm in ARMS[1:]:
                    x = med(arm, f)
                    summary[label][arm] = x
                    summary[label][arm + "_delta_pct"] = 100.0 * (x - c) / c if c else None
            result["workloads"][name] = {"viewport": [w, h], "summary": summary, "reps": reps}
            print(name, json.dumps(summary), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
