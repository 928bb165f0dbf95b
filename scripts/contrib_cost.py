"""Cost of the per-Gaussian contribution pass (ws_renderer_accumulate_contrib) beside the plain blend of the same frame, and the payoff of pruning.

Per workload (hd1m, c3 of bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames:
  * arm "plain":   a renderer with contributions off: prepare + render + stream sync
  * arm "contrib": contributions on (K1 keeps the source indices): prepare + render + accumulate_contrib + stream sync
  * per-kernel times (enable_timers(2)): k_contrib beside the k_blend of the same frames in the same run, and K1 of both arms
Then (--prune, default hd1m): the workload's own views are scored into one accumulator, the Gaussians with max_weight == 0 are
dropped (PointCloud.subset), and the full cloud and the subset are rendered alternately: frames/s of both, same run.
Writes profiles/contrib/contrib_cost.json.

    python scripts/contrib_cost.py [--workloads hd1m,c3] [--reps 3] [--frames 60] [--prune hd1m]"""
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


def run_arm(ctx, pc, views, compressed, sh_deg, contrib, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(ctx, pc.num_points()) if contrib else None
    try:
        r.enable_contrib(contrib)
        wall, kernels = [], {}

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            r.render(pc)
            if contrib:
                r.accumulate_contrib(pc, acc)
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
            for name, ms in r.kernel_times():
                kernels.setdefault(name, []).append(ms)
        stats = r.frame_stats()
        assert stats["overflow"] == 0
        return {"frame_ms_median": float(np.median(wall)), "kernel_ms_median": {k: float(np.median(v)) for k, v in kernels.items()},
                "num_visible": stats["num_visible"], "num_tile_entries": stats["num_tile_entries"]}
    finally:
        if acc:
            acc.close()
        r.close()


def frames_per_second(ctx, pc, views, compressed, sh_deg, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    try:
        for i in range(warmup):
            r.prepare(pc, views[i % len(views)])
            r.render(pc)
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(frames):
            r.prepare(pc, views[i % len(views)])
            r.render(pc)
            ctx.sync()
        dt = time.perf_counter() - t0
        assert r.frame_stats()["overflow"] == 0
        return frames / dt
    finally:
        r.close()


def prune(ctx, pc, views, compressed, sh_deg, reps, frames, warmup):
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(ctx, pc.num_points())
    try:
        r.enable_contrib(True)
        t0 = time.perf_counter()
        for v in views:
            r.prepare(pc, v)
            r.accumulate_contrib(pc, acc)
        _, q, mw = acc.download()
        score_ms = (time.perf_counter() - t0) * 1e3
        assert r.errors()[0] == 0
    finally:
        acc.close()
        r.close()
    keep = np.nonzero(mw > 0)[0].astype(np.uint32)
    sub = pc.subset(keep)
    try:
        fps = {"full": [], "subset": []}
        for rep in range(reps):
            for arm in (("full", "subset") if rep % 2 == 0 else ("subset", "full")):
                fps[arm].append(frames_per_second(ctx, pc if arm == "full" else sub, views, compressed, sh_deg, frames, warmup))
    finally:
        sub.close()
    full, subset = float(np.median(fps["full"])), float(np.median(fps["subset"]))
    return {"views_scored": len(views), "score_ms_including_download": score_ms, "points": int(pc.num_points()), "kept": int(len(keep)),
            "dropped_pct": 100.0 * (1.0 - len(keep) / pc.num_points()), "fps_full": full, "fps_subset": subset,
            "speedup_pct": 100.0 * (subset - full) / full, "fps_reps": fps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="hd1m,c3")
    ap.add_argument("--prune", default="hd1m")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib", "contrib_cost.json"))
    a = ap.parse_args()
    ctx = ws.Context(0, ws.config_from_env({}))
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}, "prune": {}}
    try:
        names = [n for n in a.workloads.split(",") if n]
        for name in names + [n for n in a.prune.split(",") if n and n not in names]:
            gpc, views, (w, h), _ = bench.build_workload(ws, name, 16)
            pc = ws.PointCloud(ctx, gpc)
            compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
            try:
                if name in names:
                    reps = {"plain": [], "contrib": []}
                    for rep in range(a.reps):  # alternating arms
                        for arm in (("plain", "contrib") if rep % 2 == 0 else ("contrib", "plain")):
                            reps[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm == "contrib", a.frames, a.warmup))

                    def med(arm, f):
                        return float(np.median([f(x) for x in reps[arm]]))

                    def k1(x):
                        ks = x["kernel_ms_median"]
                        return ks.get("k_preprocess", ks.get("k_preprocess<compressed>"))

                    blend = med("contrib", lambda x: x["kernel_ms_median"]["k_blend"])
                    contrib = med("contrib", lambda x: x["kernel_ms_median"]["k_contrib"])
                    summary = {
                        "k_blend_ms": {"plain": med("plain", lambda x: x["kernel_ms_median"]["k_blend"]), "contrib": blend},
                        "k_contrib_ms": contrib,
                        "k_contrib_over_k_blend": contrib / blend,
                        "k1_ms": {"plain": med("plain", k1), "contrib": med("contrib", k1)},
                        "frame_ms": {"plain": med("plain", lambda x: x["frame_ms_median"]), "contrib": med("contrib", lambda x: x["frame_ms_median"])},
                        "tile_entries": reps["contrib"][0]["num_tile_entries"], "visible": reps["contrib"][0]["num_visible"],
                    }
                    result["workloads"][name] = {"viewport": [w, h], "summary": summary, "reps": reps}
                    print(name, json.dumps(summary), flush=True)
                if name in a.prune.split(","):
                    result["prune"][name] = prune(ctx, pc, views, compressed, sh_deg, a.reps, a.frames, a.warmup)
                    print(name, "prune", json.dumps({k: v for k, v in result["prune"][name].items() if k != "fps_reps"}), flush=True)
            finally:
                pc.close()
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
