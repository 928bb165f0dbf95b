"""The launches over a prepared frame's weights (k_contrib, k_contrib_weighted, k_values, k_removal_base + k_removal) of this tree
against a library built from the parent commit: same bits, same speed?

Fresh child processes, alternately with the parent's library (WEBSPLAT_LIB) and with this tree's; the script stops at the first
child that does not exit with status 0 (a fault in a child: nothing more is started on the device).
  * parity: one child per side.  On c1 (10 000 Gaussians, 320 x 240; default tiles and 2x2) and on the stack of the staging
    boundaries (tests/attrib_frames._stack; k = 513 and 1025 at 32 x 32, faint and opaque), SHA-256 of accumulate_contrib's sums
    and maxima, of accumulate_weighted's with a ramp-checker plane, of render_values' 4 channels + winner, and of
    accumulate_removal's sums and maxima ("sq" and "abs", each without and with the ramp-checker plane as the weight) with its
    base plane.  Integer sums and atomics-free planes are deterministic: every digest has to be equal.
  * speed: REPS children per side on hd1m (bench.py), one frame in flight, per-kernel times from enable_timers(2): the medians
    over the frames of k_contrib, k_contrib_weighted (a plane in (0, 1] everywhere), k_values (4 channels + winner), and the
    arms removal and removal_weighted ("sq"; the same plane), both of the mark k_removal_base+k_removal.  Per arm the verdict
    compares the two medians over the repetitions with the spread (max - min) of the parent's own repetitions (attrib_cost.py's
    rule).
Writes profiles/weight_walk/ab.json.  Exit status 0: every digest equal and no kernel slower beyond the spread; 1: not so;
2: a child failed or ran out of time.

    python scripts/weight_walk_ab.py --parent-lib /path/to/parent/libwebsplat_hip.so [--reps 3] [--frames 30]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "web-splat_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402

WORKLOAD = "hd1m"
ARMS = {"k_contrib": "k_contrib", "k_contrib_weighted": "k_contrib_weighted", "k_values": "k_values",  # arm: its kernel mark
        "removal": "k_removal_base+k_removal", "removal_weighted": "k_removal_base+k_removal"}
KERNELS = tuple(ARMS)
CHILD_TIMEOUT = 300  # seconds


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def child_parity():
    import attrib_frames as A
    import oracle_lib as oracle
    import websplat as ws

    out = {}
    cases = [("c1", {}, None, None), ("c1-2x2", {"tile_qw": 2, "tile_qh": 2}, None, None)]
    cases += [(f"stack-{k}-{name}", {"bin_request": 0}, k, op) for k in (513, 1025) for name, op in (("faint", 0.002), ("opaque", 0.9))]
    for name, cfg, k, opacity in cases:
        c = A._ctx(ws, **cfg)
        try:
            f = A._c1_frame(ws, oracle, c) if k is None else A._stack_frame(ws, c, k, opacity)
            try:
                vals = np.random.default_rng(5).uniform(-1, 1, size=(f.n, 4)).astype(np.float32)
                planes, winner = f.values(vals, winner=True)
                E = A._ramp_checker(*f.view)
                out[name] = {"contrib": _sha(*f.plain()), "weighted": _sha(*f.weighted(E)), "values": _sha(planes, winner)}
                for kind in ("sq", "abs"):
                    out[name][f"removal-{kind}"] = _sha(*f.removal(kind=kind, base=True))
                    out[name][f"removal-{kind}-weighted"] = _sha(*f.removal(kind=kind, weight=E, base=True))
            finally:
                f.close()
        finally:
            c.close()
    print("CHILD " + json.dumps(out), flush=True)


def child_speed(frames, warmup):
    import bench
    import websplat as ws

    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        gpc, views, (w, h), _ = bench.build_workload(ws, WORKLOAD, 16)
        pc = ws.PointCloud(ctx, gpc)
        y, x = np.mgrid[0:h, 0:w]
        plane = (0.05 + 0.95 * ((x * 7 + y * 13) % 101) / 100.0).astype(np.float32)
        vals = np.random.default_rng(0).uniform(-1, 1, size=(pc.num_points(), 4)).astype(np.float32)
        d_plane, d_values = ctx.malloc(plane.nbytes), ctx.malloc(vals.nbytes)
        r = ws.GaussianRenderer(ctx, "rgba32float", min(3, gpc.sh_deg), bool(gpc.compressed))
        acc = ws.Contrib(ctx, pc.num_points())
        try:
            ctx.upload(d_plane, plane)
            ctx.upload(d_values, vals)
            r.enable_contrib(True)
            launch = {"k_contrib": lambda: r.accumulate_contrib(pc, acc),
                      "k_contrib_weighted": lambda: r.accumulate_weighted(pc, acc, d_plane, pitch=w * 4),
                      "k_values": lambda: r.render_values(pc, d_values, winner=True, stride=16, channels=4),
                      "removal": lambda: r.accumulate_removal(pc, acc),
                      "removal_weighted": lambda: r.accumulate_removal(pc, acc, weight=d_plane, weight_pitch=w * 4)}
            out = {}
            for label in KERNELS:
                def frame(i):
                    r.prepare(pc, views[i % len(views)])
                    launch[label]()
                    ctx.sync()

                r.enable_timers(0)
                for i in range(warmup):
                    frame(i)
                r.enable_timers(2)
                times = []
                for i in range(frames):
                    frame(i)
                    times += [ms for name, ms in r.kernel_times() if name == ARMS[label]]
                assert len(times) == frames and r.frame_stats()["overflow"] == 0
                out[label] = float(np.median(times))
        finally:
            ctx.sync()
            acc.close()
            r.close()
            ctx.free(d_plane)
            ctx.free(d_values)
            pc.close()
    finally:
        ctx.close()
    print("CHILD " + json.dumps(out), flush=True)


def run_child(side, parent_lib, args):
    env = dict(os.environ)
    env.pop("WEBSPLAT_LIB", None)
    if side == "parent":
        env["WEBSPLAT_LIB"] = parent_lib
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        print(f"{side} child {args} did not end within {CHILD_TIMEOUT} s; nothing more is started", flush=True)
        sys.exit(2)
    if res.returncode != 0:
        print(f"{side} child {args} exited with {res.returncode}; nothing more is started:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}", flush=True)
        sys.exit(2)
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", choices=["parity", "speed"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_walk", "ab.json"))
    a = ap.parse_args()
    if a.child == "parity":
        return child_parity()
    if a.child == "speed":
        return child_speed(a.frames, a.warmup)
    if not a.parent_lib or a.reps < 3:
        sys.exit(__doc__)
    parent_lib = os.path.abspath(a.parent_lib)
    result = {"what": __doc__.splitlines()[0], "workload": WORKLOAD, "reps": a.reps, "frames": a.frames}

    digests = {side: run_child(side, parent_lib, ["--child", "parity"]) for side in ("parent", "this")}
    differing = [f"{case}/{what}" for case, d in digests["parent"].items() for what in d if digests["this"][case][what] != d[what]]
    result["parity"] = {"digests": digests, "differing": differing, "verdict": "EQUAL" if not differing else "DIFFERENT"}
    print("parity:", result["parity"]["verdict"], differing, flush=True)

    got = {side: {k: [] for k in KERNELS} for side in ("parent", "this")}
    for rep in range(a.reps):
        for side in (("parent", "this") if rep % 2 == 0 else ("this", "parent")):
            t = run_child(side, parent_lib, ["--child", "speed", "--frames", str(a.frames), "--warmup", str(a.warmup)])
            for k in KERNELS:
                got[side][k].append(t[k])
            print(side, t, flush=True)
    speed = {}
    for k in KERNELS:
        parent, this = float(np.median(got["parent"][k])), float(np.median(got["this"][k]))
        spread = float(max(got["parent"][k]) - min(got["parent"][k]))
        speed[k] = {"reps_ms": {"parent": got["parent"][k], "this": got["this"][k]}, "median_ms": {"parent": parent, "this": this},
                    "parent_spread_ms": spread, "difference_ms": this - parent,
                    "verdict": "SLOWER" if this - parent > spread else "FASTER" if parent - this > spread else "WITHIN PARENT SPREAD"}
        print(k, json.dumps(speed[k]), flush=True)
    result["speed"] = speed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)
    return 1 if differing or any(s["verdict"] == "SLOWER" for s in speed.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
