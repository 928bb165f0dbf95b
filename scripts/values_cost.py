"""Cost of drawing per-Gaussian values (ws_renderer_render_values) beside the contribution pass and the blend's depth form.

On hd1m (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, per-kernel times from
enable_timers(2), every arm on the SAME views of one renderer set-up (contributions and depths kept by K1 in all of them):
  * k_values of arm "values1" (1 channel), "values4" (4 channels) and "values4w" (4 channels + winner)
  * k_contrib of arm "contrib" (the unweighted accumulate_contrib)
  * k_blend of arm "depth" (render_aux with the depth, median-depth and coverage planes)
The expectation to confirm or refute: k_values below k_contrib (no DPP reductions, no atomics) and near the blend's depth form.
Writes profiles/values/values_cost.json.

    python scripts/values_cost.py [--reps 3] [--frames 40]"""
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

WORKLOAD = "hd1m"
ARMS = {"values1": "k_values", "values4": "k_values", "values4w": "k_values", "contrib": "k_contrib", "depth": "k_blend"}


def run_arm(ctx, pc, views, compressed, sh_deg, arm, d_values, frames, warmup):
    """The median over `frames` frames of the arm's kernel time (ms) and of the frame's wall time."""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(ctx, pc.num_points())
    label = ARMS[arm]
    try:
        r.enable_contrib(True)
        r.enable_depth(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            if arm == "contrib":
                r.accumulate_contrib(pc, acc)
            elif arm == "depth":
                r.render_aux(pc, depth=True, median_depth=True, alpha=True)
            else:
                channels = 1 if arm == "values1" else 4
                r.render_values(pc, d_values, winner=arm == "values4w", stride=16, channels=channels)
            ctx.sync()

        for i in range(warmup):
            frame(i)
        wall, kernel = [], []
        for i in range(frames):
            t0 = time.perf_counter()
            frame(i)
            wall.append((time.perf_counter() - t0) * 1e3)
        r.enable_timers(2)
        for i in range(frames):
            frame(i)
            kernel += [ms for name, ms in r.kernel_times() if name == label]
        assert len(kernel) == frames and r.frame_stats()["overflow"] == 0
        return {"kernel_ms_median": float(np.median(kernel)), "frame_ms_median": float(np.median(wall))}
    finally:
        acc.close()
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "values", "values_cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "workload": WORKLOAD, "reps": a.reps, "frames": a.frames}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        gpc, views, (w, h), _ = bench.build_workload(ws, WORKLOAD, 16)
        pc = ws.PointCloud(ctx, gpc)
        compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
        vals = np.random.default_rng(0).uniform(-1, 1, size=(pc.num_points(), 4)).astype(np.float32)
        d_values = ctx.malloc(vals.nbytes)
        try:
            ctx.upload(d_values, vals)
            arms = tuple(ARMS)
            reps = {arm: [] for arm in arms}
            for rep in range(a.reps):  # alternating arms
                for arm in (arms if rep % 2 == 0 else arms[::-1]):
                    reps[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm, d_values, a.frames, a.warmup))
                    print(arm, reps[arm][-1], flush=True)
            med = {arm: float(np.median([x["kernel_ms_median"] for x in reps[arm]])) for arm in arms}
            spread = {arm: float(np.ptp([x["kernel_ms_median"] for x in reps[arm]])) for arm in arms}
            result["viewport"] = [w, h]
            result["kernel"] = ARMS
            result["kernel_ms"] = med
            result["kernel_ms_spread_over_reps"] = spread
            result["over_k_contrib"] = {arm: med[arm] / med["contrib"] for arm in arms}
            result["over_k_blend_depth_form"] = {arm: med[arm] / med["depth"] for arm in arms}
            result["arm_reps"] = reps
            print(json.dumps({k: result[k] for k in ("kernel_ms", "over_k_contrib", "over_k_blend_depth_form")}), flush=True)
        finally:
            ctx.sync()
            ctx.free(d_values)
            pc.close()
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
