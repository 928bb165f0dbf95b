"""Cost of the weighted contribution pass (ws_renderer_accumulate_weighted) beside the plain one, of the error plane, and the plain pass before and after.

On hd1m (bench.py), one frame in flight, alternating arms for REPS repetitions, medians over the frames, per-kernel times from
enable_timers(2):
  * k_contrib of arm "plain"  (accumulate_contrib), and on the SAME prepared frames
  * k_contrib_weighted of arm "full" (a plane of values in (0, 1] everywhere) and of arm "region" (the same plane, 0 outside one
    64 x 64 region in the middle of the viewport: all but 64 quadrants are idle)
  * k_image_error: wall time per launch of LAUNCHES back-to-back launches on two Rgba16Float frames of the workload's size
  * --parent-lib PATH (a libwebsplat_hip.so built from the parent commit): arm "plain" measured in fresh processes, alternately
    with that library (WEBSPLAT_LIB) and with this tree's, REPS times each.  The verdict compares the two medians with the spread
    (max - min) of the parent's own repetitions.
Writes profiles/attrib/attrib_cost.json.

    python scripts/attrib_cost.py [--reps 3] [--frames 40] [--parent-lib /path/to/parent/libwebsplat_hip.so]"""
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

WORKLOAD = "hd1m"


def planes(w, h):
    y, x = np.mgrid[0:h, 0:w]
    full = (0.05 + 0.95 * ((x * 7 + y * 13) % 101) / 100.0).astype(np.float32)
    region = np.zeros_like(full)
    y0, x0 = (h // 2 - 32) & ~7, (w // 2 - 32) & ~7
    region[y0:y0 + 64, x0:x0 + 64] = full[y0:y0 + 64, x0:x0 + 64]
    return full, region


def run_arm(ctx, pc, views, compressed, sh_deg, arm, d_plane, pitch, frames, warmup):
    """arm: "plain" | "full" | "region": the median over `frames` frames of the arm's kernel time (ms) and of the frame's wall time"""
    r = ws.GaussianRenderer(ctx, "rgba32float", sh_deg, compressed)
    acc = ws.Contrib(ctx, pc.num_points())
    label = "k_contrib" if arm == "plain" else "k_contrib_weighted"
    try:
        r.enable_contrib(True)

        def frame(i):
            r.prepare(pc, views[i % len(views)])
            if arm == "plain":
                r.accumulate_contrib(pc, acc)
            else:
                r.accumulate_weighted(pc, acc, d_plane, pitch=pitch)
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


def image_error_ms(ctx, pc, views, compressed, sh_deg, w, h, launches):
    r = ws.GaussianRenderer(ctx, "rgba16float", sh_deg, compressed)
    bufs = [ctx.malloc(w * h * 8), ctx.malloc(w * h * 8), ctx.malloc(w * h * 4)]
    try:
        for k in range(2):
            r.prepare(pc, views[k])
            r.render(pc, target_ptr=bufs[k])
        va, vb = (ws.ImageView(bufs[k], "rgba16float", w * 8, (0.0, 0.0, 0.0)).to_c() for k in range(2))

        def launch():
            ws.check(ws.lib.ws_image_error_plane(ctx.handle, va, vb, w, h, 0, 0, bufs[2], w * 4, None))

        for _ in range(10):
            launch()
        ctx.sync()
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(launches):
                launch()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3 / launches)
        return {"ms_per_launch_median": float(np.median(out)), "ms_per_launch": out, "launches": launches,
                "bytes_moved": w * h * 20}
    finally:
        ctx.sync()
        for b in bufs:
            ctx.free(b)
        r.close()


def child(frames, warmup):
    """one repetition of arm "plain" with whatever library this process loaded; prints one JSON line"""
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        gpc, views, _, _ = bench.build_workload(ws, WORKLOAD, 16)
        pc = ws.PointCloud(ctx, gpc)
        try:
            out = run_arm(ctx, pc, views, bool(gpc.compressed), min(3, gpc.sh_deg), "plain", None, 0, frames, warmup)
        finally:
            pc.close()
    finally:
        ctx.close()
    print("CHILD " + json.dumps(out), flush=True)


def before_and_after(parent_lib, reps, frames, warmup):
    got = {"parent": [], "this": []}
    for rep in range(reps):
        for side in (("parent", "this") if rep % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            env.pop("WEBSPLAT_LIB", None)
            if side == "parent":
                env["WEBSPLAT_LIB"] = parent_lib
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(frames), "--warmup", str(warmup)],
                                 env=env, capture_output=True, text=True, timeout=300)
            if res.returncode != 0:  # (a fault in a child: nothing more is started on the device)
                raise RuntimeError(f"{side} child exited with {res.returncode}: {res.stderr[-2000:]}")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")][-1]
            got[side].append(json.loads(line[6:])["kernel_ms_median"])
            print(side, got[side][-1], flush=True)
    parent, this = float(np.median(got["parent"])), float(np.median(got["this"]))
    spread = float(max(got["parent"]) - min(got["parent"]))
    return {"k_contrib_ms": {"parent": parent, "this": this}, "reps": got, "parent_spread_ms": spread, "difference_ms": this - parent,
            "within_parent_spread": bool(abs(this - parent) <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attrib", "attrib_cost.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.frames, a.warmup)
    result = {"what": __doc__.splitlines()[0], "workload": WORKLOAD, "reps": a.reps, "frames": a.frames}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        gpc, views, (w, h), _ = bench.build_workload(ws, WORKLOAD, 16)
        pc = ws.PointCloud(ctx, gpc)
        compressed, sh_deg = bool(gpc.compressed), min(3, gpc.sh_deg)
        d_planes = {}
        try:
            for name, p in zip(("full", "region"), planes(w, h)):
                d_planes[name] = ctx.malloc(p.nbytes)
                ctx.upload(d_planes[name], p)
            arms = ("plain", "full", "region")
            reps = {arm: [] for arm in arms}
            for rep in range(a.reps):  # alternating arms
                for arm in (arms if rep % 2 == 0 else arms[::-1]):
                    reps[arm].append(run_arm(ctx, pc, views, compressed, sh_deg, arm, d_planes.get(arm), w * 4, a.frames, a.warmup))
            med = {arm: float(np.median([x["kernel_ms_median"] for x in reps[arm]])) for arm in arms}
            result["viewport"] = [w, h]
            result["k_contrib_ms"] = med
            result["weighted_over_plain"] = {"full": med["full"] / med["plain"], "region": med["region"] / med["plain"]}
            result["arm_reps"] = reps
            print(json.dumps({k: result[k] for k in ("k_contrib_ms", "weighted_over_plain")}), flush=True)
            result["k_image_error"] = image_error_ms(ctx, pc, views, compressed, sh_deg, w, h, a.launches)
            print(json.dumps(result["k_image_error"]), flush=True)
        finally:
            ctx.sync()
            for p in d_planes.values():
                ctx.free(p)
            pc.close()
    finally:
        ctx.close()
    if a.parent_lib:
        result["before_and_after"] = before_and_after(os.path.abspath(a.parent_lib), a.reps, a.frames, a.warmup)
        print(json.dumps(result["before_and_after"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
