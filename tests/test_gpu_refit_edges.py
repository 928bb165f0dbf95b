"""The refit kernels on edge inputs (refit.hip k_refit_init, k_refit_init_sh, k_refit_step, k_refit_step_sh; include/websplat.h
"Refitting colour and opacity"): every family of tests/refit_edges.py on the device, word for word against refit_ref / sh_refit_ref.
tests/test_refit_edges.py holds what this rests on: each family reaches the denormals, infinities, NaNs and store ties it is named
for, the numpy twin agrees with exact rational arithmetic on denormals, and each defect a kernel could have is caught by a family.

   1. per family, kernel and degree: masters, moments, stored halves and every byte no step may write, at every check
   2. ws_refit_step_sh with lr_sh = 0 leaves what ws_refit_step leaves, on the same inputs
   3. a cloud one Gaussian shorter (256 | 257: the block edge) gives the same per-Gaussian result

THE RULE.  Two words are equal when their bits are equal, or when both are NaN and the value was computed (a master, a moment, a
half some step has stored): the sign and payload of a computed NaN are the hardware's.  A NaN that was only passed through -- a
frozen group's half, padding, the halves past the cloud's degree -- is compared by its bits, and so is +-0, always.  No tolerance,
no element left out.  How often the NaN rule was needed is counted per case; it must be 0 in decay, tiny_g and ties.

A module-scoped fixture writes one row per case to refit_edges.json in WEBSPLAT_REPORT_DIR (default: test_reports/ under the
repository root, as tests/test_gpu_metrics.py); profiles/refit/edges.json is a committed copy of an MI355X run."""
import json
import os

import numpy as np
import pytest

import refit_edges as E
from attrib_frames import _ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
NO_NAN = ("decay", "tiny_g", "ties")
RUNS = [(family, kernel, sh_deg) for family in E.FAMILIES
        for kernel, sh_deg in (("step", 3), ("step_sh0", 3), ("step_sh", 3), ("step_sh", 1), ("step_sh", 2))]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        total = {k: sum(r[k] for r in REPORT) for k in ("words_compared", "words_differing", "nan_class_comparisons")}
        with open(os.path.join(out, "refit_edges.json"), "w") as f:
            json.dump({"rule": "bits equal, or both NaN where the value was computed; +-0 and passed-through NaN by bits; no tolerance",
                       "classes": "per intermediate of refit_ref._adam: [denormal, infinite, NaN] values the reference met over all steps",
                       "total": total, "cases": REPORT}, f, indent=1)


def _nan(bits):
    bits = np.asarray(bits)
    if bits.dtype == np.uint32:
        return (bits & 0x7FFFFFFF) > 0x7F800000
    assert bits.dtype == np.uint16
    return (bits & 0x7FFF) > 0x7C00


class _Tally:
    """words compared, words differing, comparisons the NaN rule decided; the first few differences in words"""

    def __init__(self):
        self.compared = self.differing = self.nan_class = 0
        self.first = []

    def words(self, what, got, want, computed):
        """got, want: uint16 / uint32 / uint8 arrays of one shape; computed: whether a NaN may differ in sign and payload
        (a bool, or an array that broadcasts)"""
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
        same = got == want
        if got.dtype != np.uint8:
            by_class = ~same & _nan(got) & _nan(want) & np.broadcast_to(computed, got.shape)
            self.nan_class += int(by_class.sum())
            same = same | by_class
        self.compared += got.size
        bad = np.argwhere(~same)
        self.differing += len(bad)
        for at in bad[:4]:
            at = tuple(int(v) for v in at)
            self.first.append(f"{what}{list(at)}: device 0x{int(got[at]):x}, reference 0x{int(want[at]):x}")


class _Device:
    """A case's cloud on the device with its Refit and the accumulator its kernel reads."""

    def __init__(self, ws, c, case, kernel):
        self.case, self.kernel = case, kernel
        g, s = case.g.copy(), case.s.copy()
        aabb, center, up = ws.pointcloud_stats(g, 28, ws.Aabb([0, 0, 0], [0, 0, 0]))
        gpc = ws.GenericGaussianPointCloud(g, s, case.sh_deg, case.n, aabb, center, up=up)
        self.pc = ws.PointCloud(c, gpc)
        self.refit = ws.Refit(c, self.pc)
        if kernel == "step":
            self.grad = ws.Grad(c, case.n)
        else:
            self.refit.enable_sh(self.pc)
            self.grad = ws.ShGrad(c, case.n, case.sh_deg)
        self.zeroed = False

    def step(self, st):
        if st["zero"]:
            if not self.zeroed:   # one reset serves every zero-sum step that follows: no upload per step
                self.grad.reset()
                self.zeroed = True
        else:
            self.grad.reset()
            if self.kernel == "step":
                self.grad.add(np.concatenate([st["q_sh"][:, 0, :], st["q_o"][:, None]], axis=1))
            else:
                self.grad.add(sh=st["q_sh"], opacity=st["q_o"])
            self.zeroed = False
        args = dict(E.step_args(st, self.kernel), colour_unit=st["colour_unit"], opacity_unit=st["opacity_unit"])
        if self.kernel == "step":
            self.refit.step(self.pc, self.grad, **args)
        else:
            self.refit.step_sh(self.pc, self.grad, **args)

    def state(self):
        """{"master", "m", "v"[, "sh_master", "sh_m", "sh_v"]} as uint32, the blobs as (N, 14) and (N, 48) uint16"""
        out = {k: np.ascontiguousarray(v).view(np.uint32) for k, v in self.refit.download().items()}
        if self.kernel != "step":
            out.update({"sh_" + k: np.ascontiguousarray(v).view(np.uint32) for k, v in self.refit.download_sh().items()})
        g, s = self.pc.download()
        out["g"] = np.ascontiguousarray(g).view(np.uint16).reshape(self.case.n, 14)
        out["s"] = np.ascontiguousarray(s).view(np.uint16).reshape(self.case.n, 48)
        return out

    def close(self):
        self.grad.close()
        self.refit.close()
        self.pc.close()


def _against_reference(tally, where, got, snap, kernel, n):
    for k in ("master", "m", "v") + (("sh_master", "sh_m", "sh_v") if kernel != "step" else ()):
        tally.words(f"{where} {k}", got[k], np.ascontiguousarray(getattr(snap, k)).view(np.uint32), True)
    want_g = np.ascontiguousarray(snap.g).view(np.uint16).reshape(n, 14)
    want_s = np.ascontiguousarray(snap.s).view(np.uint16).reshape(n, 48)
    computed_g = np.zeros(14, bool)
    computed_g[6] = snap.written[48]   # the opacity half; the halves beside it are x, y, z, the padding and the covariance
    tally.words(f"{where} gaussians (halves)", got["g"], want_g, computed_g[None, :])
    tally.words(f"{where} sh (halves)", got["s"], want_s, snap.written[None, :48])


def _run(ws, c, case, kernel):
    """The case on the device, compared with the reference at every check: (Expected, _Tally, {check: the device's state})."""
    ex = E.expected(case, kernel)
    tally = _Tally()
    states = {}
    d = _Device(ws, c, case, kernel)
    try:
        if 0 in case.checks:
            states[0] = d.state()
            _against_reference(tally, "after create", states[0], ex.snaps[0], kernel, case.n)
        for k, st in enumerate(case.steps, start=1):
            d.step(st)
            if k in case.checks:
                states[k] = d.state()
                assert d.refit.steps == k
                _against_reference(tally, f"step {k}", states[k], ex.snaps[k], kernel, case.n)
    finally:
        d.close()
    assert sorted(states) == sorted(case.checks)
    return ex, tally, states


# ---- 1. every family, kernel and degree -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,kernel,sh_deg", RUNS)
def test_device_equals_the_reference_word_for_word(ws, family, kernel, sh_deg):
    c = _ctx(ws)
    failures = []
    try:
        for case in E.family(family, sh_deg):
            ex, tally, _ = _run(ws, c, case, kernel)
            row = dict(family=family, case=case.name, kernel=kernel, degree=sh_deg, n=case.n, steps=len(case.steps), checks=len(case.checks),
                       words_compared=tally.compared, words_differing=tally.differing, nan_class_comparisons=tally.nan_class,
                       classes={k: v for k, v in ex.classes.items() if any(v)})
            REPORT.append(row)
            print({k: v for k, v in row.items() if k != "classes"})
            if tally.differing:
                failures.append(f"{case.name}: {tally.differing} of {tally.compared} words differ: " + "; ".join(tally.first[:8]))
            if family in NO_NAN and tally.nan_class:
                failures.append(f"{case.name}: {tally.nan_class} comparisons met a NaN in a family that has none")
    finally:
        c.close()
    assert not failures, "\n".join(failures)


# ---- 2. the lr_sh = 0 tie, on edge inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", E.FAMILIES)
def test_frozen_rest_group_is_refit_step_on_edge_inputs(ws, family):
    """Both kernels on the device, bits against bits (the hardware's NaN is the same on both sides): masters, moments and every
    byte of the cloud, at every check."""
    c = _ctx(ws)
    try:
        for case in E.family(family, 3):
            plain, frozen = _run(ws, c, case, "step")[2], _run(ws, c, case, "step_sh0")[2]
            differing = [(k, key) for k in plain for key in ("master", "m", "v", "g", "s") if not np.array_equal(plain[k][key], frozen[k][key])]
            assert not differing, (case.name, differing[:8])
    finally:
        c.close()


# ---- 3. one Gaussian fewer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", E.FAMILIES)
def test_per_gaussian_result_does_not_depend_on_the_size_around_the_block_edge(ws, family):
    """The family at 257 Gaussians (decay: 65) and at one fewer, in two contexts: Gaussian i comes out the same in both."""
    long = E.family(family, 3)
    short = E.family(family, 3, long[0].n - 1)
    ca, cb = _ctx(ws), _ctx(ws)
    try:
        for a, b in zip(long, short):
            assert a.name == b.name and b.n == a.n - 1 and np.array_equal(a.g[:b.n], b.g) and np.array_equal(a.s[:b.n], b.s)
            more, (_, tally, fewer) = _run(ws, ca, a, "step_sh")[2], _run(ws, cb, b, "step_sh")
            differing = [(k, key) for k in fewer for key, v in fewer[k].items() if not np.array_equal(v, more[k][key][:b.n])]
            assert not differing and tally.differing == 0, (a.name, differing[:8], tally.first[:8])
    finally:
        cb.close()
        ca.close()
