#!/usr/bin/env python3
"""Offline check that tests/test_gpu_blend_boundary.py bites: for every device image the test saved
(WS_BLEND_BOUNDARY_SAVE=<dir> python -m pytest tests/test_gpu_blend_boundary.py -m gpu), compare it once more with the float64
reference of its own frame -- with ONE MARKER DROPPED from the reference, and with TWO NEIGHBOURING MARKERS EXCHANGED -- under the
test's gate.  Every such comparison has to FAIL: a kernel that had lost or exchanged that record would have drawn the mutated
reference's image.  Needs no device.  Cases with an occluder are left out (a marker behind the cut is not drawn at all).

usage: python scripts/blend_boundary_recheck.py <dir>      exit status 0 = every mutation failed the gate"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "web-splat_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import blend_ref as B  # noqa: E402


def stack_positions(frame, spec, st):
    """List positions (near end first) of the markers of stack `st`, and of its neighbouring marker pairs: the frame's records
    are told apart by their centre pixel."""
    w, h = spec.viewport
    h16 = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    cx, cy = (h16[:, 4] * 0.5 + 0.5) * w, (0.5 - h16[:, 5] * 0.5) * h
    centres = np.array([s["centre"] for s in spec.stacks if s["k"]])
    mine = np.argmin((cx[:, None] - centres[:, 0]) ** 2 + (cy[:, None] - centres[:, 1]) ** 2, axis=1)
    index = [i for i, s in enumerate(s for s in spec.stacks if s["k"]) if s is st][0]
    order = frame["sorted"].astype(np.int64)[::-1]
    where = np.nonzero(mine[order] == index)[0]
    assert len(where) == st["k"]
    pos = [int(where[m]) for m in st["positions"]]
    pairs = [(p, p1) for (m, p), (m1, p1) in zip(zip(st["positions"], pos), zip(st["positions"][1:], pos[1:])) if m1 == m + 1]
    return pos, pairs


def main(directory):
    specs = {s.name: s for s in B.all_specs()}
    tried = passed_wrongly = 0
    for path in sorted(glob.glob(os.path.join(directory, "*.npz"))):
        d = np.load(path)
        if "occluder" in d.files or str(d["spec"]) not in specs:
            continue
        spec, fmt = specs[str(d["spec"])], str(d["fmt"])
        w, h = spec.viewport
        frame = {"splats": d["splats"], "sorted": d["sorted"]}
        b = B.record_weights(frame, w, h)
        C, T = B.walk(frame, b)
        worst, excess = B.colour_errors(fmt, d["image"], B.over({"C": C, "T": T}, d["target"], fmt))
        assert excess <= 0, f"{path}: the unmutated reference fails the gate ({worst:.3e})"
        n = 0
        for st in spec.stacks:
            if not st["k"]:
                continue
            pos, pairs = stack_positions(frame, spec, st)
            for kw in [dict(drop=p) for p in pos] + [dict(swap=p) for p in pairs]:
                C, T = B.walk(frame, b, **kw)
                _, excess = B.colour_errors(fmt, d["image"], B.over({"C": C, "T": T}, d["target"], fmt))
                tried += 1
                n += 1
                if excess <= 0:
                    passed_wrongly += 1
                    print(f"{os.path.basename(path)}: {kw} still PASSES the gate")
        print(f"{os.path.basename(path)}: {n} mutations, unmutated error {worst:.2e}")
    print(f"{tried} mutated references tried, {passed_wrongly} still passed the gate")
    return 1 if passed_wrongly or not tried else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
