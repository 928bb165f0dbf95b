"""Cost of the geometry gradients (ws_renderer_accumulate_geometry_gradient) beside the colour / opacity and the SH gradients.

On hd1m and c1 (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, per-launch times
from stream events (enable_timers(2)), every arm on the SAME views of one renderer set-up (contributions kept by K1 in all), a
signed ramp in all four components of the plane (no quadrant is idle).  One pair of events brackets an arm's launches:
  * "gradient"   k_removal_base + k_gradient
  * "sh"         k_removal_base + k_gradient + k_sh_spread
  * "stage_a"    k_removal_base + k_geometry                       (the test hook: the sums stay in the scratch)
  * "geometry"   k_removal_base + k_geometry + k_geom_spread
so k_sh_spread = sh - gradient and k_geom_spread = geometry - stage_a; stage_a over gradient compares the two walks with the base
image's launch in both.

Predicted from the code, nothing promised and no gate: k_geometry walks the same pairs as k_gradient with eight DPP wave sums per
walked record where that has six and five LDS partials where that has four -- a third more reduction work on a loop the
reductions dominate, so 1.2 to 1.35 times k_gradient's launch; k_geom_spread touches about one visible splat in fourteen per frame
(the rest read 4 B of source index and 40 B of scratch and return), and each touched one costs about 250 f64 operations, a
division chain and eleven read-modify-writes: the order of k_sh_spread at degree 3, well under a tenth of the walk.
Writes profiles/geometry/cost.json.

    python scripts/geometry_cost.py [--reps 3] [--frames 15]"""
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

ARMS = {"gradient": "k_removal_base+k_gradient", "sh": "k_removal_base+k_gradient+k_sh_spread", "stage_a": "k_removal_base+k_geometry",
        "geometry": "k_removal_base+k_geometry+k_geom_spread"}


def run_arm(ctx, pc, views, sh_deg, arm, d_plane, width, frames, warmup):
    """The median over `frames` frames of the arm's launch time (ms) and of the frame's wall time."""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, False)
    n = pc.num_points()
    acc = ws.Grad(ctx, n) if arm == "gradient" else ws.ShGrad(ctx, n, pc.sh_deg()) if arm == "sh" else ws.GeomGrad(ctx, n)
    label = ARMS[arm]
    try:
        r.enable_contrib(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            if arm == "gradient":
                r.accumulate_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            elif arm == "sh":
                r.accumulate_sh_gradient(pc, acc, d_plane, plane_pitch=width * 16, opacity_scale=1.0 / 16)
            else:
                r.accumulate_geometry_gradient(pc, acc, d_plane, plane_pitch=width * 16, geometry_scale=1.0 / 16, _stage_a_only=arm == "stage_a")
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
        out = {"kernel_ms_median": float(np.median(kernel)), "frame_ms_median": float(np.median(wall))}
        if arm == "geometry":
            got = acc.download()
            out["seen_last_frames_mean"] = float(got["seen"].sum()) / acc.frames
            out["visible_last_frame"] = int(r.frame_stats()["num_visible"])
        return out
    finally:
        acc.close()
        r.close()


def run_workload(ctx, workload, reps, frames, warmup):
    gpc, views, (w, h), _ = bench.build_workload(ws, workload, 16)
    assert not gpc.compressed, "geometry gradients need an uncompressed cloud"
    pc = ws.PointCloud(ctx, gpc)
    sh_deg = min(3, gpc.sh_deg)
    d_plane = ctx.malloc(w * h * 16)
    try:
        x, y = np.arange(w, dtype=np.float32)[None, :] / w, np.arange(h, dtype=np.float32)[:, None] / h
        ctx.upload(d_plane, np.stack([0.9 * np.sin(2.3 * x + 1.1 * y + 0.3), 0.8 * np.cos(1.7 * x - 2.9 * y + 0.2), 0.7 * (x - y) + 0.013,
                                      0.6 * np.sin(3.1 * (x + y)) - 0.21], axis=-1).astype(np.float32))
        arms = tuple(ARMS)
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (arms if rep % 2 == 0 else arms[::-1]):
                got[arm].append(run_arm(ctx, pc, views, sh_deg, arm, d_plane, w, frames, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["kernel_ms_median"] for x in got[arm]])) for arm in arms}
        last = got["geometry"][-1]
        return {"viewport": [w, h], "gaussians": pc.num_points(), "launches": ARMS, "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["kernel_ms_median"] for x in got[arm]])) for arm in arms},
                "k_sh_spread_ms": med["sh"] - med["gradient"], "k_geom_spread_ms": med["geometry"] - med["stage_a"],
                "stage_a_over_gradient": med["stage_a"] / med["gradient"], "geometry_over_sh": med["geometry"] / med["sh"],
                "touched_per_visible": last["seen_last_frames_mean"] / max(1, last["visible_last_frame"]), "plane_bytes": w * h * 16, "arm_reps": got}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry", "cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "frames": a.frames, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.frames, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "k_sh_spread_ms", "k_geom_spread_ms", "stage_a_over_gradient", "touched_per_visible")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
