"""Cost of the SH spread (k_sh_spread) and of one SH refit step (ws_refit_step_sh, k_refit_step_sh) beside the gradient pass they follow.

On hd1m and c1 (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, times from stream
events, all arms on the SAME prepared frames of one renderer set-up (contributions kept by K1), a signed ramp in all four components
of the plane:
  * arm "gradient": the two launches k_removal_base + k_gradient into a Grad (one pair of events around both, enable_timers(2))
  * arm "sh_gradient": the three launches k_removal_base + k_gradient + k_sh_spread into a ShGrad, timed the same way; the spread
    is the difference of the two arms' medians
  * arm "refit_sh": k_refit_step_sh behind that pass, on the sums it left -- one pair of events around the one launch (so the
    interval holds the dispatch latency of a dependent launch), and the mean of ten steps enqueued back to back
PREDICTION, written from the code before any measurement:
  k_sh_spread       32 B per Gaussian (its scratch row), plus 32 + 16 + 16 (3 ncoef + 1) B per Gaussian whose row is not zero (the row
                    written back, the plane-0 chunk, a read-modify-write of 8 B per element): 0.83 KB at degree 3
  k_refit_step_sh   36 B per element (8 B sum; master, m, v read and written: 24 B; 2 x 2 B of the half) over 3 ncoef + 1 elements:
                    1.76 KB per Gaussian at degree 3, more than the Infinity Cache holds on hd1m, so bound by HBM: against the
                    ~6.3 TB/s a copy achieves on this part, ~0.28 ms per million Gaussians
Nothing is promised and nothing is gated.  Writes profiles/sh_refit/cost.json, the prediction beside the measurement.

    python scripts/sh_refit_cost.py [--reps 3] [--frames 15]"""
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

MARKS = {"gradient": "k_removal_base+k_gradient", "sh_gradient": "k_removal_base+k_gradient+k_sh_spread"}
BACK_TO_BACK = 10
COPY_TB_PER_S = 6.3


def run_pass(arm, ctx, pc, views, sh_deg, d_plane, width, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", 3, False)
    acc = ws.Grad(ctx, pc.num_points()) if arm == "gradient" else ws.ShGrad(ctx, pc.num_points(), sh_deg)
    call = r.accumulate_gradient if arm == "gradient" else r.accumulate_sh_gradient
    try:
        r.enable_contrib(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            call(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            ctx.sync()

        for i in range(warmup):
            frame(i)
        r.enable_timers(2)
        kernel = []
        for i in range(frames):
            frame(i)
            kernel += [ms for name, ms in r.kernel_times() if name == MARKS[arm]]
        assert len(kernel) == frames and r.frame_stats()["overflow"] == 0
        out = {"launch_ms_median": float(np.median(kernel))}
        if arm == "gradient":   # how many Gaussians one frame touches: the rows of the last frame alone that are not zero
            acc.reset()
            frame(0)
            out["touched"] = int((acc.download() != 0).any(axis=1).sum())
        return out
    finally:
        acc.close()
        r.close()


def run_refit(arm, ctx, pc, views, sh_deg, d_plane, width, frames, warmup):
    """(A rate of 0 would skip its group's work; tiny rates do all of it and keep the scene where it is for the other arms.)"""
    r = ws.GaussianRenderer(ctx, "rgba32float", 3, False)
    acc = ws.ShGrad(ctx, pc.num_points(), sh_deg)
    fit = ws.Refit(ctx, pc)
    fit.enable_sh(pc)
    adam = dict(lr_colour=1e-7, lr_opacity=1e-7, lr_sh=1e-7, opacity_scale=1.0 / 16)
    try:
        r.enable_contrib(True)

        def frame(i, steps):
            acc.reset()
            r.prepare(pc, views[i % len(views)])
            r.accumulate_sh_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fit.step_sh(pc, acc, **adam)
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
    n, sh_deg = pc.num_points(), pc.sh_deg()
    ncoef = (sh_deg + 1) ** 2
    d_plane = ctx.malloc(w * h * 16)
    try:
        x, y = np.arange(w, dtype=np.float32)[None, :] / w, np.arange(h, dtype=np.float32)[:, None] / h
        ctx.upload(d_plane, np.stack([0.9 * np.sin(2.3 * x + 1.1 * y + 0.3), 0.8 * np.cos(1.7 * x - 2.9 * y + 0.2), 0.7 * (x - y) + 0.013,
                                      0.6 * np.sin(3.1 * (x + y)) - 0.21], axis=-1).astype(np.float32))
        arms = {"gradient": run_pass, "sh_gradient": run_pass, "refit_sh": run_refit}
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (tuple(arms) if rep % 2 == 0 else tuple(arms)[::-1]):
                got[arm].append(arms[arm](arm, ctx, pc, views, sh_deg, d_plane, w, frames, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["launch_ms_median"] for x in got[arm]])) for arm in arms}
        b2b = float(np.median([x["back_to_back_ms_median"] for x in got["refit_sh"]]))
        touched = got["gradient"][0]["touched"]
        spread_bytes = 32 * n + touched * (32 + 16 + 16 * (3 * ncoef + 1))
        refit_bytes = 36 * (3 * ncoef + 1) * n
        predicted = {"spread_bytes": spread_bytes, "spread_ms_at_copy_rate": spread_bytes / (COPY_TB_PER_S * 1e12) * 1e3,
                     "refit_bytes": refit_bytes, "refit_ms_at_copy_rate": refit_bytes / (COPY_TB_PER_S * 1e12) * 1e3,
                     "touched_gaussians_of_one_frame": touched, "copy_TB_per_s": COPY_TB_PER_S}
        spread_ms = med["sh_gradient"] - med["gradient"]
        return {"viewport": [w, h], "gaussians": n, "sh_deg": sh_deg, "launches": dict(MARKS, refit_sh="k_refit_step_sh"), "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["launch_ms_median"] for x in got[arm]])) for arm in arms},
                "predicted": predicted,
                "measured": {"spread_ms": spread_ms, "spread_over_gradient": spread_ms / med["gradient"], "refit_single_ms": med["refit_sh"],
                             "refit_back_to_back_ms": b2b,
                             "spread_GB_per_s_if_predicted_bytes": spread_bytes / (max(spread_ms, 1e-6) * 1e-3) / 1e9,
                             "refit_GB_per_s_if_predicted_bytes": {"single": refit_bytes / (med["refit_sh"] * 1e-3) / 1e9,
                                                                   "back_to_back": refit_bytes / (b2b * 1e-3) / 1e9}},
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sh_refit", "cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.frames, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "predicted", "measured")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
