"""Cost of the removal effect (ws_renderer_accumulate_removal) beside the contribution pass, on the same prepared frames.

On hd1m and c1 (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, per-launch times
from stream events (enable_timers(2)), every arm on the SAME views of one renderer set-up (contributions kept by K1 in all):
  * the two launches of arm "removal" (k_removal_base + k_removal, one pair of events around both), unweighted, "sq"
  * the same with a weight plane of ones, arm "removal_weighted"
  * k_contrib of arm "contrib" (the unweighted accumulate_contrib)
The expectation to confirm or refute: about twice k_contrib plus a W x H x 16-byte plane written once and read once.
Writes profiles/removal/removal_cost.json.

    python scripts/removal_cost.py [--reps 3] [--frames 30]"""
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

ARMS = {"removal": "k_removal_base+k_removal", "removal_weighted": "k_removal_base+k_removal", "contrib": "k_contrib"}


def run_arm(ctx, pc, views, compressed, sh_deg, arm, d_ones, width, frames, warmup):
    """The median over `frames` frames of the arm's launch time (ms) and of the frame's wall time."""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(ctx, pc.num_points())
    label = ARMS[arm]
    try:
        r.enable_contrib(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            if arm == "contrib":
                r.accumulate_contrib(pc, acc)
            elif arm == "removal":
                r.accumulate_removal(pc, acc)
            else:
                r.accumulate_removal(pc, acc, weight=d_ones, weight_pitch=width * 4)
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


def run_workload(ctx, workload, reps, frames, warmup):
    gpc, views, (w, h), _ = bench.build_workload(ws, workload, 16)
    pc = ws.PointCloud(ctx, gpc)
    compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
    d_ones = ctx.malloc(w * h * 4)
    try:
        ctx.upload(d_ones, np.ones((h, w), np.float32))
        arms = tuple(ARMS)
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (arms if rep % 2 == 0 else arms[::-1]):
                got[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm, d_ones, w, frames, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["kernel_ms_median"] for x in got[arm]])) for arm in arms}
        return {"viewport": [w, h], "gaussians": pc.num_points(), "launches": ARMS, "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["kernel_ms_median"] for x in got[arm]])) for arm in arms},
                "over_k_contrib": {arm: med[arm] / med["contrib"] for arm in arms}, "base_plane_bytes": w * h * 16, "arm_reps": got}
    finally:
        ctx.sync()
        ctx.free(d_ones)
        pc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workloads", default="hd1m,c1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "removal", "removal_cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.frames, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "over_k_contrib")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
