"""Cost of the loss gradients (ws_renderer_accumulate_gradient) beside the removal effect and the contribution pass.

On hd1m and c1 (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, per-launch times
from stream events (enable_timers(2)), every arm on the SAME views of one renderer set-up (contributions kept by K1 in all):
  * the two launches of arm "gradient" (k_removal_base + k_gradient, one pair of events around both), a signed ramp in all four
    components of the plane (no quadrant is idle)
  * the two launches of arm "removal" (k_removal_base + k_removal), unweighted, "sq"
  * k_contrib of arm "contrib" (the unweighted accumulate_contrib)
Nothing is promised: the pair loop carries removal's arithmetic, four more multiplies, three fused multiply-adds and six DPP wave
sums where removal has three.  Writes profiles/gradient/gradient_cost.json.

    python scripts/gradient_cost.py [--reps 3] [--frames 15]"""
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

ARMS = {"gradient": "k_removal_base+k_gradient", "removal": "k_removal_base+k_removal", "contrib": "k_contrib"}


def run_arm(ctx, pc, views, compressed, sh_deg, arm, d_plane, width, frames, warmup):
    """The median over `frames` frames of the arm's launch time (ms) and of the frame's wall time."""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Grad(ctx, pc.num_points()) if arm == "gradient" else ws.Contrib(ctx, pc.num_points())
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
                r.accumulate_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
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
    d_plane = ctx.malloc(w * h * 16)
    try:
        x, y = np.arange(w, dtype=np.float32)[None, :] / w, np.arange(h, dtype=np.float32)[:, None] / h
        ctx.upload(d_plane, np.stack([0.9 * np.sin(2.3 * x + 1.1 * y + 0.3), 0.8 * np.cos(1.7 * x - 2.9 * y + 0.2), 0.7 * (x - y) + 0.013,
                                      0.6 * np.sin(3.1 * (x + y)) - 0.21], axis=-1).astype(np.float32))
        arms = tuple(ARMS)
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (arms if rep % 2 == 0 else arms[::-1]):
                got[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm, d_plane, w, frames, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["kernel_ms_median"] for x in got[arm]])) for arm in arms}
        return {"viewport": [w, h], "gaussians": pc.num_points(), "launches": ARMS, "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["kernel_ms_median"] for x in got[arm]])) for arm in arms},
                "over_k_contrib": {arm: med[arm] / med["contrib"] for arm in arms},
                "over_removal": {arm: med[arm] / med["removal"] for arm in arms}, "plane_bytes": w * h * 16, "arm_reps": got}
    finally:
        ctx.sync()
        ctx.free(d_plane)
        pc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workloads", default="hd1m,c1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient", "gradient_cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.frames, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "over_k_contrib", "over_removal")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
