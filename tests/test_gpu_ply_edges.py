"""k_ply_decode (ply_decode.hip) on the edge clouds of tests/ply_rows.py, bit for bit against the numpy restatement with the
kernel's own exp (an f64 exp rounded once to f32): positions, padding and the SH record byte for byte, the opacity and the six
covariance halves exactly on every row, NaN halves compared as a class.  tests/test_ply_rows.py holds the conditions this rests
on: the restatement equals the oracle and the host twin, and no row of any cloud is undecided between two f64 exp
implementations -- so nothing here is a tolerance.

Each cloud is one decode of at most a few thousand rows.  Per cloud the number of halves that differ from the f64-exp reference
(expected: 0) and from the libm oracle goes to ply_decode_report.json in WEBSPLAT_REPORT_DIR (default: test_reports/ under the
repository root, as tests/test_gpu_metrics.py); profiles/ply_decode/report.json is a committed copy of an MI355X run."""
import json
import os

import numpy as np
import pytest

import ply_rows as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREES = (0, 1, 2, 3)
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        total = {k: sum(r[k] for r in REPORT.values()) for k in ("rows", "halves", "differ_from_f64_exp_reference",
                                                                 "differ_from_libm_oracle", "sh_halves_differing")}
        with open(os.path.join(out, "ply_decode_report.json"), "w") as f:
            json.dump({"compared": "opacity + six covariance halves per row, NaN as a class", "total": total, "clouds": REPORT},
                      f, indent=1)


def _decode_and_compare(ws, ctx, oracle, name, d):
    rows = pr.bulk_rows(d) if name == "bulk" else pr.cloud(name, d)
    n = rows.shape[0]
    pc = ws.PointCloud.from_ply_rows(ctx, rows, d)
    try:
        assert pc.num_points() == n and pc.sh_deg() == d and not pc.compressed()
        g, s = pc.download()
    finally:
        pc.close()
    g0, s0 = pr.reference(name, d, "f64")
    bad, bad_sh, fixed = pr.compare(g, s, g0, s0)
    bad_libm = pr.compare(g, s, *oracle.ply_rows_convert(rows, d))[0]
    REPORT[f"{name}/deg{d}"] = {"rows": n, "halves": int(bad.size), "differ_from_f64_exp_reference": int(bad.sum()),
                                "differ_from_libm_oracle": int(bad_libm.sum()), "sh_halves_differing": int(bad_sh.sum())}
    print(name, d, REPORT[f"{name}/deg{d}"])
    return rows, g, g0, bad, bad_sh, fixed


def _first(rows, d, g, g0, bad):
    """the first differing halves by (row, half): the row's tail, what the device gave, what the reference gives"""
    out = []
    for i, k in np.argwhere(bad)[:6].tolist():
        out.append({"row": i, "half": ("opacity", "c00", "c01", "c02", "c11", "c12", "c22")[k],
                    "tail": rows[i, pr.tail_col(d):].tolist(), "device": hex(pr.computed_halves(g)[i, k]),
                    "reference": hex(pr.computed_halves(g0)[i, k])})
    return out


@pytest.mark.parametrize("d", DEGREES)
@pytest.mark.parametrize("name", pr.CLOUDS)
def test_edge_cloud_decodes_bit_for_bit(ws, ctx, oracle, name, d):
    rows, g, g0, bad, bad_sh, fixed = _decode_and_compare(ws, ctx, oracle, name, d)
    assert fixed                                           # positions and padding, byte for byte
    if bad_sh.any():                                       # a slot by name: (row, coefficient, channel)
        i, e = np.argwhere(bad_sh)[0].tolist()
        raise AssertionError(f"SH half of row {i}, coefficient {e // 3}, channel {e % 3} ({int(bad_sh.sum())} differ)")
    assert not bad.any(), (int(bad.sum()), _first(rows, d, g, g0, bad))


@pytest.mark.parametrize("d", DEGREES)
def test_bulk_scene_decodes_bit_for_bit(ws, ctx, oracle, d):
    """the 50 001-row scene of tests/test_gpu_ply_decode.py, which holds it to one ulp against the libm oracle: exact against
    the f64-exp restatement"""
    rows, g, g0, bad, bad_sh, fixed = _decode_and_compare(ws, ctx, oracle, "bulk", d)
    assert fixed and not bad_sh.any()
    assert not bad.any(), (int(bad.sum()), _first(rows, d, g, g0, bad))
