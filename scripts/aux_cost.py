"""Cost of the auxiliary planes (ws_renderer_render_aux): colour only against colour + depth + median depth + coverage.

Per workload (hd1m, c3, c5 of bench.py) and arm, alternating arms for REPS repetitions:
  * one-in-flight frame time: prepare + render (+ planes) + stream sync per frame, wall clock, median over the frames
  * stage timers (ws_renderer_stage_times: preprocess / sorting / binning / rasterization) and per-kernel times
    (enable_timers(2)), medians over the frames
The colour-only arm is a renderer with depth off calling render(); the aux arm has depth on (K1's DEPTH form) and calls
render_aux() with all three planes.  Writes profiles/aux/aux_cost.json.

    python scripts/aux_cost.py [--workloads hd1m,c3,c5] [--reps 3] [--frames 60]"""
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


def run_arm(ctx, pc, views, compressed, sh_deg, aux, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    try:
        r.enable_depth(aux)
        wall, stages, kernels = [], [], {}

        def frame(i, timed):
            r.prepare(pc, views[i % len(views)])
            if aux:
                r.render_aux(pc, depth=True, median_depth=True, alpha=True)
            else:
                r.render(pc)
            ctx.sync()

        for i in range(warmup):
            frame(i, False)
        for i in range(frames):  # one in flight, no instrumentation
            t0 = time.perf_counter()
            frame(i, True)
            wall.append((time.perf_counter() - t0) * 1e3)
        r.enable_timers(2)
        for i in range(frames):
            frame(i, True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux", "aux_cost.json"))
    a = ap.parse_args()
    ctx = ws.Context(0, ws.config_from_env({}))
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    try:
        for name in a.workloads.split(","):
            gpc, views, (w, h), _ = bench.build_workload(ws, name, 16)
            pc = ws.PointCloud(ctx, gpc)
            compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
            reps = {"colour": [], "aux": []}
            try:
                for rep in range(a.reps):  # alternating arms
                    for arm in (("colour", "aux") if rep % 2 == 0 else ("aux", "colour")):
                        reps[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm == "aux", a.frames, a.warmup))
            finally:
                pc.close()

            def med(arm, f):
                return float(np.median([f(x) for x in reps[arm]]))

            def blend(x):
                return x["kernel_ms_median"].get("k_blend", x["stage_ms_median"]["rasterization"])

            def k1(x):
                ks = x["kernel_ms_median"]
                return ks.get("k_preprocess", ks.get("k_preprocess<compressed>", x["stage_ms_median"]["preprocess"]))

            summary = {}
            for label, f in (("frame_ms", lambda x: x["frame_ms_median"]), ("blend_kernel_ms", blend), ("k1_kernel_ms", k1),
                             ("rasterization_stage_ms", lambda x: x["stage_ms_median"]["rasterization"]),
                             ("preprocess_stage_ms", lambda x: x["stage_ms_median"]["preprocess"])):
                c, x = med("colour", f), med("aux", f)
                summary[label] = {"colour": c, "aux": x, "delta_pct": 100.0 * (x - c) / c if c else None}
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
