"""Cost of the save kernel (k_ply_encode) beside the load kernel (k_ply_decode) on the same rows.

On hd1m and c1 (bench.py), REPS alternating repetitions, medians over LAUNCHES launches per arm, times from stream events around
one launch each (so every interval holds the dispatch latency of a launch, as every per-launch time of this library does), and
the mean of ten launches enqueued back to back between one pair of events, where that latency overlaps:
  * arm "encode": ws_pointcloud_encode_ply_rows_device -- the resident planes of the workload's cloud -> rows in device memory
  * arm "decode": ws_pointcloud_decode_ply_rows_device -- those rows -> the planes of a second cloud of the size
PREDICTION, written down before the first run, from the code: both kernels move 128 B of planes and 248 B of row per Gaussian at
degree 3, 376 B, once each, coalesced on the plane side and as one contiguous run per block on the row side.  At the 6.3 TB/s a
copy reaches that is 0.060 ms per million Gaussians; the encode adds a few hundred dependent f64 operations per thread (two to
four Jacobi sweeps of three rotations with an f64 division and two square roots each, three logarithms), which at 8 waves per
SIMD should hide partly: expected 0.10 - 0.20 ms per million Gaussians for the encode, 0.07 - 0.10 ms for the decode.  Nothing is
promised and nothing is gated.  Writes profiles/ply_encode/encode_cost.json with the prediction beside the measurement.

    python scripts/ply_encode_cost.py [--reps 3] [--launches 15]"""
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

PLANE_BYTES, BACK_TO_BACK = 128, 10
PREDICTED_MS_PER_MILLION = {"encode": [0.10, 0.20], "decode": [0.07, 0.10], "copy_at_6.3_TB_per_s": 0.060}


def timed(ctx, call, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        call()
    b.record()
    ctx.sync()
    b.synchronize()
    return a.elapsed_time(b) / count


def run_arm(ctx, call, launches, warmup):
    for _ in range(warmup):
        timed(ctx, call, 1)
    one = [timed(ctx, call, 1) for _ in range(launches)]
    many = [timed(ctx, call, BACK_TO_BACK) for _ in range(launches)]
    return {"launch_ms_median": float(np.median(one)), "back_to_back_ms_median": float(np.median(many))}


def run_workload(ctx, workload, reps, launches, warmup):
    gpc, _, _, _ = bench.build_workload(ws, workload, 1)
    assert not gpc.compressed
    pc, other = ws.PointCloud(ctx, gpc), ws.PointCloud(ctx, gpc)
    n, sh_deg = pc.num_points(), pc.sh_deg()
    row_bytes = 4 * (14 + 3 * (sh_deg + 1) ** 2)
    d_rows = ctx.malloc(n * row_bytes)
    try:
        arms = {"encode": lambda: pc.encode_ply_rows_device(d_rows, n * row_bytes),
                "decode": lambda: other.decode_ply_rows_device(d_rows, n * row_bytes)}
        arms["encode"]()      # the rows the decode arm reads
        ctx.sync()
        got = {arm: [] for arm in arms}
        for rep in range(reps):  # alternating arms
            for arm in (tuple(arms) if rep % 2 == 0 else tuple(arms)[::-1]):
                got[arm].append(run_arm(ctx, arms[arm], launches, warmup))
                print(workload, arm, got[arm][-1], flush=True)
        med = {arm: float(np.median([x["launch_ms_median"] for x in got[arm]])) for arm in arms}
        b2b = {arm: float(np.median([x["back_to_back_ms_median"] for x in got[arm]])) for arm in arms}
        expected = n * (PLANE_BYTES + row_bytes)
        predicted = {arm: [lo * n / 1e6, hi * n / 1e6] for arm, (lo, hi) in (("encode", PREDICTED_MS_PER_MILLION["encode"]), ("decode", PREDICTED_MS_PER_MILLION["decode"]))}
        return {"gaussians": n, "sh_deg": sh_deg, "launches": {"encode": "k_ply_encode", "decode": "k_ply_decode"}, "launch_ms": med,
                "launch_ms_spread_over_reps": {arm: float(np.ptp([x["launch_ms_median"] for x in got[arm]])) for arm in arms},
                "back_to_back_ms": b2b, "encode_over_decode": b2b["encode"] / b2b["decode"],
                "expected_bytes": expected, "expected_bytes_per_gaussian": PLANE_BYTES + row_bytes,
                "GB_per_s_if_expected_bytes": {arm: expected / (b2b[arm] * 1e-3) / 1e9 for arm in arms},
                "predicted_ms": predicted,
                "back_to_back_over_predicted_upper": {arm: b2b[arm] / predicted[arm][1] for arm in arms},
                "arm_reps": got}
    finally:
        ctx.sync()
        ctx.free(d_rows)
        other.close()
        pc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="hd1m,c1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_encode", "encode_cost.json"))
    a = ap.parse_args()
    result = {"what": __doc__.splitlines()[0], "reps": a.reps, "launches": a.launches,
              "prediction_ms_per_million_gaussians": PREDICTED_MS_PER_MILLION, "workloads": {}}
    ctx = ws.Context(0, ws.config_from_env({}))
    try:
        for workload in a.workloads.split(","):
            result["workloads"][workload] = run_workload(ctx, workload, a.reps, a.launches, a.warmup)
            print(json.dumps({workload: {k: result["workloads"][workload][k] for k in ("launch_ms", "back_to_back_ms", "predicted_ms", "encode_over_decode",
                                                                                        "GB_per_s_if_expected_bytes")}}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
