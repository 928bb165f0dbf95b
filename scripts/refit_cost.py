"""Cost of one refit step (ws_refit_step, k_refit_step) beside the gradient pass that feeds it.

On hd1m and c1 (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, times from stream
events, both arms on the SAME prepared frames of one renderer set-up (contributions kept by K1):
  * arm "gradient": the two launches k_removal_base + k_gradient (one pair of events around both, enable_timers(2)), a signed
    ramp in all four components of the plane
  * arm "refit": k_refit_step behind that gradient pass, on the sums it left -- one pair of events around the one launch (so the
    interval holds the dispatch latency of a dependent launch, as every per-launch time of this library does), and the mean of
    ten steps enqueued back to back between one pair of events, where that latency overlaps
Expectation from the code: ~140 B per Gaussian (32 B of sums, 3 x 16 B read and written, 12 B of the planes' words written and 8
read), purely streaming.  Nothing is promised and nothing is gated.  Writes profiles/refit/refit_cost.json.

    python scripts/refit_cost.py [--reps 3] [--frames 15]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "web-splat_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (its events time the legacy default stream, the one the library's calls below enqueue on)

import bench  # noqa: E402
import websplat as ws  # noqa: E402

GRADIENT = "k_removal_base+k_gradient"
BYTES_PER_GAUSSIAN = 32 + 3 * 16 * 2 + 12 + 8
BACK_TO_BACK = 10


def run_gradient(ctx, pc, views, sh_deg, d_plane, width, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, False)
    acc = ws.Grad(ctx, pc.num_points())
    try:
        r.enable_contrib(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            r.accumulate_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            ctx.sync()

        for i in range(warmup):
            frame(i)
        r.enable_timers(2)
        kernel = []
        for i in range(frames):
            frame(i)
            kernel += [ms for name, ms in r.kernel_times() if name == GRADIENT]
        assert len(kernel) == frames and r.frame_stats()["overflow"] == 0
        return {"launch_ms_median": float(np.median(kernel))}
    finally:
        acc.close()
        r.close()


def run_refit(ctx, pc, views, sh_deg, d_plane, width, frames, warmup):
    """(A rate of 0 would skip its group's work; tiny rates do all of it and keep the scene where it is for the other arm.)"""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, False)
    acc = ws.Grad(ctx, pc.num_points())
    fit = ws.Refit(ctx, pc)
    adam = dict(lr_colour=1e-7, lr_opacity=1e-7, opacity_scale=1.0 / 16)
    try:
        r.enable_contrib(True)

        def frame(i, steps):
            acc.reset()
            r.prepare(pc, views[i % len(views)])
            r.accumulate_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fit.step(pc, acc, **adam)
            b.record()
            ctx.sync()
            b.synchronize()
            return a.elapsed_time(b) / steps

        for i in range(warmup):
            frame(i, 1)
        one = [frame(i, 1) for i in range(frames)]
        many = [frame(i, BACK_TO_BACK) for i in range(frames)]
        assert r.frame_stats()["overflow"] == 0
        return {"launch_ms_median": float(np.median(one)), "back_to_back_ms_median": float(np.median(many))}
    finally:
        fit.close()
        acc.close()
        r.close()


def run_workload(ctx, workload, reps, frames, warmup):
    gpc, views, (w, h), _ = bench.build_workload(ws, workload, 16)
    assert not gpc.compressed
    pc = ws.PointCloud(ctx, gpc)
    n, sh_deg = pc.num_points(), min(3, gpc.sh_deg)
    d_plane = ctx.malloc(w * h * 16)
    try:
        x, y = np.arange(w, dtype=np.float32)[None, :] / w, np.arange(h, dtype=np.float32)[:, None] / h
        ctx.upload(d_plane, np.stack([0.9 * np.sin(2.3 * x + 1.1 * y + 0.3), 0.8 * np.cos(1.7 * x - 2.9 * y + 0.2), 0.7 * (x - y) + 0.013,
                                      0.6 * np.sin(3.1 * (x + y)) - 0.21], axis=-1).astype(np.float32))
        arms = {"gradient": run_gradient, "refit": run_refit}
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (tuple(arms) if rep % 2 == 0 else tuple(arms)[::-1]):
                got[arm].append(arms[arm](ctx, pc, views, sh_deg, d_plane, w, frames, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["launch_ms_median"] for x in got[arm]])) for arm in arms}
        b2b = float(np.median([x["back_to_back_ms_median"] for x in got["refit"]]))
        expected = n * BYTES_PER_GAUSSIAN
        return {"viewport": [w, h], "gaussians": n, "launches": {"gradient": GRADIENT, "refit": "k_refit_step"}, "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["launch_ms_median"] for x in got[arm]])) for arm in arms},
                "refit_back_to_back_ms": b2b, "refit_over_gradient": med["refit"] / med["gradient"],
                "expected_bytes": expected, "expected_bytes_per_gaussian": BYTES_PER_GAUSSIAN,
                "GB_per_s_if_expected_bytes": {"single": expected / (med["refit"] * 1e-3) / 1e9, "back_to_back": expected / (b2b * 1e-3) / 1e9},
                "arm_reps": got}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "refit_cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.frames, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "refit_back_to_back_ms", "refit_over_gradient",
                                                                                        "GB_per_s_if_expected_bytes")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
