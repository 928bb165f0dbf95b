"""What tests/test_gpu_refit_edges.py rests on, without a GPU (tests/refit_edges.py, tests/refit_ref.py, tests/sh_refit_ref.py):

   1. every family reaches the classes it is named for: per intermediate of refit_ref._adam, the exact number of denormal,
      infinite and NaN values the reference meets (REACHED below, degree 3 through ws_refit_step_sh), and the facts behind each
   2. the facts the families were built from: the step at which a decaying moment first goes denormal, the value it sticks at,
      the results of the store on ties
   3. every defect of refit_ref.DEFECTS changes what some family expects -- and which of them the five-step inputs of
      tests/test_gpu_refit.py can tell apart
   4. the numpy twin on denormals: two steps of decay and of tiny_g again in exact rational arithmetic, every operation rounded
      once to float32 (subnormal grid included) by _round32 below

ON 3.  The five-step inputs never meet a denormal, an infinity or a NaN (they assert so), hence cannot see flush_results,
daz_divide_sqrt or clamp_fmin_fmax: 0 words differ.  The two store defects are another matter: a store that truncates differs on
about half of all stored halves, so the five-step tests do catch it.  A store that is wrong ON TIES ONLY (store_ties_toward_zero,
added here for that reason) or that flushes subnormal halves is seen by three and by one of the 27 000 halves those tests store,
where a random master happens to land on such a value (a float32 is a tie of the f16 store once in 2^13): chance, not a check.
The test pins all of this."""
from fractions import Fraction

import numpy as np
import pytest

import refit_edges as E
import refit_ref
import sh_refit_ref as ref

F = np.float32
TINY = float(np.finfo(F).tiny)
SMALLEST = 2.0 ** -149

# family -> case -> intermediate -> [denormal, infinite, NaN], at degree 3 through ws_refit_step_sh; what is not listed is [0, 0, 0]
REACHED = {}   # (filled in below the tests: REACHED.update(...))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _h16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _groups(case, st, kernel="step_sh"):
    """{"colour" | "opacity" | "rest": {name: array}}: the intermediates of one reference step from the case's start"""
    state = ref.ShState(*E.start_halves(case))
    trace = []
    ref.step_sh(state, st["q_sh"], st["q_o"], st["colour_unit"], st["opacity_unit"], trace=trace, **E.step_args(st, kernel))
    out, i = {}, 0
    for name, width in (("colour", 15), ("opacity", 16), ("rest", 15)):
        rate = {"colour": "lr_colour", "opacity": "lr_opacity", "rest": "lr_sh"}[name]
        if F(st["adam"][rate]) == 0 or (name == "rest" and case.sh_deg == 0):
            continue
        out[name] = dict(zip(E.NAMES, trace[i + width - 15:i + width]))
        i += width
    assert i == len(trace)
    return out, state


# ---- 1. what every family reaches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", E.FAMILIES)
def test_family_reaches_its_classes_count_for_count(family):
    got = {}
    for case in E.family(family, 3):
        ex = E.expected(case, "step_sh")
        got[case.name] = {k: v for k, v in ex.classes.items() if any(v)}
        print(family, case.name, got[case.name])
    assert got == REACHED[family]
    if family not in ("overflow", "hostile_halves", "params"):
        assert all(v[1] == 0 and v[2] == 0 for c in got.values() for v in c.values()), "an infinity or a NaN outside the three families that aim at them"


@pytest.mark.parametrize("sh_deg,kernel", [(3, "step"), (3, "step_sh0"), (1, "step_sh"), (2, "step_sh")])
def test_named_classes_are_reached_at_every_degree_and_kernel(sh_deg, kernel):
    """The intermediates each row of the families' table names, wherever the device is compared."""
    def reached(family, name, which):
        case = next(c for c in E.family(family, sh_deg) if c.name == name)
        return {k for k, v in E.expected(case, kernel).classes.items() if v[which]}

    assert {"a", "m1", "mh", "s", "t"} <= reached("decay", "decay", 0)
    assert {"g", "b", "m1", "mh"} <= reached("tiny_g", "2^-140", 0)
    assert {"gg", "d", "v1", "vh"} <= reached("tiny_g", "2^-75", 0) and {"gg", "d", "v1", "vh"} <= reached("tiny_g", "2^-70", 0)
    assert {"gg", "v1", "vh", "r", "den"} <= reached("overflow", "finite_and_gg_inf", 1)
    assert {"g", "m1", "mh"} <= reached("overflow", "gg_inf_and_g_inf", 1) and {"s", "t", "x1"} <= reached("overflow", "gg_inf_and_g_inf", 2)
    assert "x1" in reached("hostile_halves", "ordinary", 1) and "x1" in reached("hostile_halves", "ordinary", 2)
    assert "den" in reached("params", "eps_smallest", 0) and "s" in reached("params", "eps_3e38", 0) and "x1" in reached("params", "lr_3e38", 1)
    for family in ("decay", "tiny_g", "ties"):
        for case in E.family(family, sh_deg):
            assert all(v[1] == 0 and v[2] == 0 for v in E.expected(case, kernel).classes.values()), (family, case.name)


def test_decay_sticks_above_zero():
    case, = E.family("decay", 3)
    ex = E.expected(case, "step_sh")
    first = next(k for k, c in enumerate(ex.per_step, start=1) if c[0])
    print("decay: first step with a denormal intermediate", first)
    assert 580 <= first <= 600 and first in case.checks and not any(c[0] for c in ex.per_step[:first - 1])
    end, before = ex.snaps[1200], ex.snaps[1100]
    for m in (end.m, end.sh_m):
        moved = m[m != 0]
        assert moved.size > m.size // 2 and (np.abs(moved) == F(4 * SMALLEST)).all()   # 4 * 0.9 = 3.6 rounds back to 4
    assert np.array_equal(_u32(end.m), _u32(before.m)) and np.array_equal(_u32(end.sh_m), _u32(before.sh_m))
    assert np.array_equal(_u32(end.master), _u32(before.master)) and np.array_equal(_u32(end.sh_master), _u32(before.sh_master))
    assert np.array_equal(end.g, before.g) and np.array_equal(end.s, before.s)
    assert not np.array_equal(_u32(ex.snaps[580].m), _u32(ex.snaps[600].m))


def test_tiny_g_facts():
    cases = {c.name: c for c in E.family("tiny_g", 3)}
    # 2^-140: g, b, m' denormal, g * g = 0, the denominator is eps
    gr, state = _groups(cases["2^-140"], cases["2^-140"].steps[0])
    q = cases["2^-140"].steps[0]["q_sh"][:, 0, :]
    assert np.array_equal(gr["colour"]["g"].astype(np.float64), q * 2.0 ** -140), "the DC gradients are not exactly q * 2^-140"
    assert not gr["colour"]["gg"].any() and (gr["colour"]["den"] == F(1e-15)).all() and not gr["rest"]["gg"].any()
    assert (np.abs(gr["colour"]["m1"][q != 0]) < TINY).all() and (gr["colour"]["m1"][q != 0] != 0).all()
    # 2^-70: omb2 * g * g rounds at the bottom of the denormal grid: 0.512 q^2 units of 2^-149 -> 1, 5, 13
    gr, state = _groups(cases["2^-70"], cases["2^-70"].steps[0])
    q = cases["2^-70"].steps[0]["q_sh"][:, 0, :]
    for sum_, units in ((1, 1), (3, 5), (-5, 13)):
        assert (q == sum_).any() and (_u32(state.v[:, :3])[q == sum_] == units).all(), (sum_, units)
    # 2^-75: g * g is a tie or inexact on the grid: q^2 / 2 units, to even
    gr, _ = _groups(cases["2^-75"], cases["2^-75"].steps[0])
    q = cases["2^-75"].steps[0]["q_sh"][:, 0, :]
    for sum_, units in ((1, 0), (3, 4), (-5, 12), (7, 24)):
        assert (_u32(gr["colour"]["gg"])[q == sum_] == units).all(), (sum_, units)


def test_overflow_regimes():
    for case in E.family("overflow", 3):
        ex = E.expected(case, "step_sh")
        one, two, three = ex.snaps[1], ex.snaps[2], ex.snaps[3]
        # the exact step to an opacity master of 2^-40, whose half is 0
        assert (one.master[:, 3] == F(2.0 ** -40)).all() and not _h16(one.g[:, 12:14]).any()
        assert np.array_equal(one.s, case.s) and np.array_equal(one.g[:, 14:], case.g[:, 14:]) and np.array_equal(one.g[:, :12], case.g[:, :12])
        state = ref.ShState(*E.start_halves(case))
        ref.step_sh(state, case.steps[0]["q_sh"], case.steps[0]["q_o"], E.UNIT, E.UNIT, **E.step_args(case.steps[0], "step_sh"))
        trace = []
        st = case.steps[1]
        ref.step_sh(state, st["q_sh"], st["q_o"], st["colour_unit"], st["opacity_unit"], trace=trace, **E.step_args(st, "step_sh"))
        seen = set()
        for name, at, x0, x1, v1, x2, v2, halves in (
                ("colour", 0, one.master[:, :3], two.master[:, :3], two.v[:, :3], three.master[:, :3], three.v[:, :3], two.s.view(np.uint16)[:, :3]),
                ("opacity", 16, one.master[:, 3], two.master[:, 3], two.v[:, 3], three.master[:, 3], three.v[:, 3], two.g.view(np.uint16)[:, 6]),
                ("rest", 31, one.sh_master, two.sh_master, two.sh_v, three.sh_master, three.sh_v,
                 two.s.view(np.uint16)[:, 3:].reshape(case.n, 15, 3))):
            g, gg = np.abs(trace[at]), trace[at + 4]
            finite = (g >= 2.0 ** 63) & (g < 2.0 ** 64)
            frozen = np.isinf(gg) & np.isfinite(g)
            poisoned = np.isinf(g)
            if finite.any():
                seen.add("finite")
                assert all(np.isfinite(z[finite]).all() for z in trace[at:at + 15]) and (x1[finite] != x0[finite]).all(), name
            if frozen.any():   # v' = inf, s = 0: the master stays, at once and a step later
                seen.add("frozen")
                assert np.isinf(v1[frozen]).all() and np.isinf(v2[frozen]).all(), name
                assert np.array_equal(_u32(x1[frozen]), _u32(x0[frozen])) and np.array_equal(_u32(x2[frozen]), _u32(x0[frozen])), name
            if poisoned.any():   # m' = inf, s = inf / inf: a NaN master and a NaN half in the scene
                seen.add("poisoned")
                assert np.isnan(x1[poisoned]).all() and np.isnan(x2[poisoned]).all() and ((halves[poisoned] & 0x7FFF) > 0x7C00).all(), name
        assert seen == ({"finite", "frozen"} if case.name == "finite_and_gg_inf" else {"frozen", "poisoned"}), (case.name, seen)


def test_hostile_halves_facts():
    cases = {c.name: c for c in E.family("hostile_halves", 3)}
    case = cases["ordinary"]
    ex = E.expected(case, "step_sh")
    h4, rest = E.start_halves(case)
    for halves, master in ((h4, ex.snaps[0].master), (rest, ex.snaps[0].sh_master)):
        assert set(E.HOSTILE.tolist()) == set(_h16(halves).ravel().tolist())
        nan = np.isnan(halves)
        assert np.array_equal(np.isnan(master), nan) and np.array_equal(master[~nan].astype(np.float64), halves[~nan].astype(np.float64))
        assert np.array_equal(np.signbit(master[~nan]), np.signbit(halves[~nan])) and (master == F(2.0 ** -24)).any()
    one = ex.snaps[1]
    for halves, master in ((h4[:, :3], one.master[:, :3]), (rest, one.sh_master)):   # an infinite master comes back as +-65504
        assert (master[np.isposinf(halves)] == F(65504.0)).all() and (master[np.isneginf(halves)] == F(-65504.0)).all()
        assert np.isnan(master[np.isnan(halves)]).all() and np.isfinite(master[~np.isnan(halves)]).all()
    zero = h4[:, 3] == 0   # +0 and -0: the x == 0 branch, whatever the sum
    q_o = case.steps[0]["q_o"]
    assert (q_o[zero] != 0).any() and np.signbit(h4[zero, 3]).any() and not one.m[zero, 3].any() and not one.v[zero, 3].any()
    assert np.array_equal(_u32(one.master[zero, 3]), _u32(h4[zero, 3].astype(F)))   # (-0 - 0 = -0, and -0 < opacity_min = +0 is false)
    inf_op, nan_op = np.isinf(h4[:, 3]), np.isnan(h4[:, 3])
    assert inf_op.any() and not one.m[inf_op, 3].any() and np.isnan(one.master[nan_op, 3]).all() and nan_op.sum() >= 2
    # frozen groups keep their bits, a signalling NaN among them
    sh0, op0 = _h16(case.s).reshape(case.n, 48), _h16(case.g[:, 12:14])
    for name, cols in (("only_colour", slice(0, 3)), ("only_opacity", None), ("only_sh", slice(3, 48))):
        snap = E.expected(cases[name], "step_sh").snaps[1]
        sh1, op1 = _h16(snap.s).reshape(case.n, 48), _h16(snap.g[:, 12:14])
        moved = np.zeros(48, bool)
        if cols is not None:
            moved[cols] = True
        assert np.array_equal(sh1[:, ~moved], sh0[:, ~moved]) and (sh0[:, ~moved] == 0x7D00).any() and (sh1[:, moved] != sh0[:, moved]).any() == (cols is not None)
        assert np.array_equal(op1, op0) == (name != "only_opacity") and (op0 == 0x7D00).any()
        assert np.array_equal(snap.g[:, 14:], case.g[:, 14:])


def test_ties_steer_the_store_everywhere():
    kinds = {}
    for case in E.family("ties", 3):
        snap = E.expected(case, "step_sh").snaps[1]
        for x in (snap.master, snap.sh_master):
            for k, v in E.rounding_kinds(x).items():
                kinds[k] = kinds.get(k, 0) + v
        assert np.array_equal(_h16(snap.s).reshape(case.n, 48)[:, :3], _h16(refit_ref.store16(snap.master[:, :3])))
    print("ties: how the store rounds", kinds)
    assert all(kinds[k] > 100 for k in ("exact", "down", "up", "tie_to_even_down", "tie_to_even_up", "subnormal_half", "zero_from_nonzero")), kinds
    case = E.family("ties", 3)[0]
    start, end = _h16(case.s).reshape(case.n, 48)[:, :3], _h16(E.expected(case, "step_sh").snaps[1].s).reshape(case.n, 48)[:, :3]
    assert (start == 0x8000).any() and (end[start == 0x8000] == 0x8000).all(), "a -0 half with a zero sum does not stay -0"
    top = next(c for c in E.family("ties", 3) if c.name == "top")
    m = E.expected(top, "step_sh").snaps[1]
    assert (m.master[:, :3] == F(65504.0 - 8.0)).any() and (m.sh_master == F(65472.0 + 16.0)).any() and (np.abs(m.master[:, :3]) <= F(65504.0)).all()
    sub = next(c for c in E.family("ties", 3) if c.name == "subnormal_0")
    m = E.expected(sub, "step_sh").snaps[1]
    assert (m.master[:, :3] == F(2.0 ** -25)).any() and (m.master[:, 3] == F(2.0 ** -26)).any() and (m.sh_master == F(2.0 ** -25 * (1 + 2.0 ** -20))).any()


def test_params_facts():
    cases = {c.name: c for c in E.family("params", 3)}
    for name, power in (("beta1_0", "p1"), ("beta2_0", "p2"), ("lr_3e38", "p1")):   # bc = (float)(1.0 - 0) = 1
        state = ref.ShState(*E.start_halves(cases[name]))
        st = cases[name].steps[0]
        ref.step_sh(state, st["q_sh"], st["q_o"], st["colour_unit"], st["opacity_unit"], **st["adam"])
        assert getattr(state, power) == 0.0 and (state.p1 == 0.0) != (state.p2 == 0.0)
    gr, state = _groups(cases["eps_smallest"], cases["eps_smallest"].steps[0])
    still = np.arange(cases["eps_smallest"].n) % 5 == 2
    assert not cases["eps_smallest"].steps[0]["q_sh"][still].any() and not cases["eps_smallest"].steps[0]["q_o"][still].any()
    assert still.sum() > 40 and (gr["colour"]["den"][still] == F(SMALLEST)).all() and not gr["colour"]["s"][still].any()   # 0 / eps = 0
    assert np.array_equal(_u32(state.master[still]), _u32(E.start_halves(cases["eps_smallest"])[0].astype(F)[still]))
    gr, _ = _groups(cases["eps_3e38"], cases["eps_3e38"].steps[0])
    s = gr["colour"]["s"]
    assert ((s != 0) & (np.abs(s) < TINY)).sum() > 300 and (gr["colour"]["den"] == F(3e38)).all()
    snap = E.expected(cases["opacity_min_1"], "step_sh").snaps[2]
    assert (snap.master[:, 3] == F(1.0)).all() and (_h16(snap.g[:, 12:14]) == 0x3C00).all()
    ex = E.expected(cases["lr_3e38"], "step_sh")
    assert ex.classes["x1"][1] > 1000 and ex.classes["x1"][2] == 0
    snap = ex.snaps[2]
    moved = cases["lr_3e38"].steps[0]["q_sh"][:, 0, :] != 0
    assert (np.abs(snap.master[:, :3][moved]) == F(65504.0)).all() and np.isin(snap.master[:, 3], [F(0.0), F(1.0), *snap.master[~moved.any(axis=1), 3]]).all()


# ---- 2. the facts the families were built from ---------------------------------------------------------------------------------------
def test_quoted_decay():
    """One-shot sums of 2^20, -2^8, 2^40 and 1 under the default betas, units of 2^-32, opacity_min = 2^-7: the first denormal
    intermediate appears at step 586; at step 1200 every first moment is +-4 * 2^-149 and has been for 100 steps."""
    h = np.array([[0.5, -0.25, 1.0, 0.5]] * 4, np.float16)
    st = refit_ref.State(h)
    q = np.repeat(np.array(E.DECAY_QUOTED, np.int64)[:, None], 4, axis=1)
    first, at_1100 = None, None
    for k in range(1, 1201):
        trace = []
        refit_ref.step(st, q if k == 1 else np.zeros_like(q), E.UNIT, E.UNIT, opacity_min=2.0 ** -7, trace=trace)
        if first is None and not refit_ref.all_zero_or_normal(trace):
            first = k
        if k == 1100:
            at_1100 = (st.m.copy(), st.master.copy())
    assert first == 586
    assert (np.abs(st.m) == F(4 * SMALLEST)).all() and np.array_equal(np.signbit(st.m), q < 0)
    assert np.array_equal(_u32(st.m), _u32(at_1100[0])) and np.array_equal(_u32(st.master), _u32(at_1100[1]))
    # the same Gaussians open the decay family
    case, = E.family("decay", 3)
    assert np.array_equal(case.steps[0]["q_sh"][:4, 0, :], q[:, :3]) and np.array_equal(case.steps[0]["q_o"][:4], q[:, 3])
    assert np.array_equal(E.start_halves(case)[0][:4], h)
    assert np.array_equal(_u32(E.expected(case, "step").snaps[1200].m[:4]), _u32(st.m))


def test_quoted_ties():
    cu = E.unit_for(E.UNIT)
    assert cu * refit_ref.C0 == E.UNIT
    st = refit_ref.State(np.array([[1.0, 1.0 + 2.0 ** -10, -(1.0 + 3 * 2.0 ** -10), 0.5]], np.float16))
    trace = []
    refit_ref.step(st, np.array([[2 ** 32, 2 ** 32, -(2 ** 32), 0]], np.int64), cu, E.UNIT, lr_colour=2.0 ** -11, lr_opacity=0.0, beta1=0.0,
                   beta2=0.0, trace=trace)
    assert np.array_equal(trace[0], np.array([[1, 1, -1]], F)) and np.array_equal(trace[12], np.array([[1, 1, -1]], F))
    assert np.array_equal(st.master[0, :3].astype(np.float64), [1 - 2.0 ** -11, 1 + 2.0 ** -11, -(1 + 5 * 2.0 ** -11)])
    assert _h16(st.halves())[0, :3].tolist() == [0x3BFF, 0x3C00, 0xBC02]   # exact; a tie down to even; a tie to even
    sub = np.array([2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, 5 * 2.0 ** -25], F)
    assert _h16(refit_ref.store16(sub)).tolist() == [0x0000, 0x0002, 0x0001, 0x0000, 0x0002]


# ---- 3. the defects ------------------------------------------------------------------------------------------------------------------
CATCHES = {   # defect -> the families that must see it (degree, kernel)
    "flush_results": (("decay", 3, "step"), ("tiny_g", 3, "step_sh"), ("params", 3, "step_sh")),
    "daz_divide_sqrt": (("tiny_g", 3, "step"), ("tiny_g", 3, "step_sh"), ("params", 3, "step")),   # (decay cannot: a flushed m' / bc1 only
                                                                                                   #  turns a step of less than an ulp into 0)
    "clamp_fmin_fmax": (("overflow", 3, "step"), ("overflow", 2, "step_sh"), ("hostile_halves", 3, "step")),
    "store_toward_zero": (("ties", 3, "step"), ("ties", 1, "step_sh")),
    "store_flush_subnormal": (("ties", 3, "step"), ("ties", 2, "step_sh"), ("hostile_halves", 3, "step")),
    "rewiden_unstepped": (("hostile_halves", 3, "step"), ("hostile_halves", 3, "step_sh0"), ("hostile_halves", 1, "step_sh"), ("ties", 2, "step_sh")),
    "store_ties_toward_zero": (("ties", 3, "step"), ("ties", 3, "step_sh")),
}


def _words_differing(a, b):
    """between two Expected: masters, moments and blobs by their bits, over every check"""
    total = 0
    for k in a.snaps:
        for key in ("master", "m", "v", "sh_master", "sh_m", "sh_v"):
            total += int((_u32(getattr(a.snaps[k], key)) != _u32(getattr(b.snaps[k], key))).sum())
        for key in ("g", "s"):
            total += int((_h16(getattr(a.snaps[k], key)) != _h16(getattr(b.snaps[k], key))).sum())
    return total


@pytest.mark.parametrize("defect", refit_ref.DEFECTS)
def test_every_defect_is_caught_by_a_family(defect):
    assert set(CATCHES) == set(refit_ref.DEFECTS)
    for family, sh_deg, kernel in CATCHES[defect]:
        words = sum(_words_differing(E.expected(case, kernel), E.expected(case, kernel, defect)) for case in E.family(family, sh_deg))
        print(f"{defect}: {family} at degree {sh_deg} through {kernel}: {words} expected words differ")
        assert words > 0, (defect, family, sh_deg, kernel)


def test_defect_hook_off_changes_nothing():
    """defect=None is the code path every other test of the reference takes; an unknown name is no defect either."""
    case = E.family("hostile_halves", 3)[0]
    assert _words_differing(E.expected(case, "step_sh"), E.expected(case, "step_sh", "no such defect")) == 0
    x = np.array([1.0 + 2.0 ** -11, 2.0 ** -25, 65519.0, -0.0, np.nan], F)
    assert np.array_equal(_h16(refit_ref.store16(x))[:4], _h16(x.astype(np.float16))[:4])


def _five_step_words(ws, defect):
    """What tests/test_gpu_refit.py test_step_bit_for_bit_at_wave_and_block_edges compares (masters, moments, stored halves), its
    own inputs, sound reference against defective: {(n, step): words differing}, and the stored halves that are ties / subnormal."""
    import test_gpu_refit as old
    out, ties, subnormal, stored = {}, 0, 0, 0
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        gpc = old._cloud(ws, old._rows(n, 100 + n))
        h0 = old._halves(gpc.gaussians, gpc.sh_coefs)
        a, b = refit_ref.State(h0), refit_ref.State(h0)
        rng = np.random.default_rng(n)
        for k in range(1, 6):
            q = old._sums(rng, n)
            trace = []
            refit_ref.step(a, q, old.UNIT, old.UNIT, trace=trace, **old.ADAM)
            refit_ref.step(b, q, old.UNIT, old.UNIT, defect=defect, **old.ADAM)
            assert refit_ref.all_zero_or_normal(trace)
            words = sum(int((_u32(getattr(a, key)) != _u32(getattr(b, key))).sum()) for key in ("master", "m", "v"))
            words += int((_h16(a.halves()) != _h16(b.halves(defect))).sum())
            if words:
                out[(n, k)] = words
            kinds = E.rounding_kinds(a.master)
            ties += kinds["tie_to_even_down"] + kinds["tie_to_even_up"]
            subnormal += kinds["subnormal_half"]
            stored += a.master.size
    return out, ties, subnormal, stored


@pytest.mark.parametrize("defect", ["flush_results", "daz_divide_sqrt", "clamp_fmin_fmax"])
def test_five_step_cases_cannot_tell_the_defect_apart(ws, defect):
    """THE GAP: on the inputs of the five-step test not one compared word changes under these defects."""
    words, ties, _, stored = _five_step_words(ws, defect)
    print(defect, "on the five-step inputs:", words, "; stored halves", stored, "of them ties", ties)
    assert words == {} and stored > 20000


def test_five_step_cases_and_the_store_defects(ws):
    """A truncating store is no gap: about half of all stored halves differ, in every five-step case but the first step of n = 1.
    A store that is wrong on ties only is seen by THREE of the 27 000 stored halves, one that flushes subnormal halves by ONE
    (n = 255, step 2): values that random masters happen to land on (a tie once in 2^13), in three and one of the forty
    (case, step) pairs.  Pinned here so that nobody takes those tests for a check of the store's rounding."""
    words, _, _, stored = _five_step_words(ws, "store_toward_zero")
    print("store_toward_zero on the five-step inputs: halves differing", sum(words.values()), "of", stored)
    assert 0.4 * stored < sum(words.values()) < 0.6 * stored and len(words) >= 38
    words, _, subnormal, stored = _five_step_words(ws, "store_flush_subnormal")
    print("store_flush_subnormal on the five-step inputs:", words, "subnormal halves stored", subnormal, "of", stored)
    assert words == {(255, 2): 1} and subnormal == 1
    words, ties, _, stored = _five_step_words(ws, "store_ties_toward_zero")
    print("store_ties_toward_zero on the five-step inputs:", words, "ties stored", ties, "of", stored)
    assert words == {(63, 2): 1, (65, 3): 1, (1000, 3): 1} and ties <= 8


# ---- 4. the numpy twin on denormals, against exact arithmetic ----------------------------------------------------------------------------
def _round32(x):
    """The float32 nearest to the Fraction x, ties to even, the subnormal grid of 2^-149 included; as a Fraction.  (No value
    here is large enough to overflow.)"""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e < 127
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, quantum)
    if rem * 2 > quantum or (rem * 2 == quantum and n % 2):
        n += 1
    return (n * quantum) * (1 if x > 0 else -1)


def _sqrt32(x):
    """the correctly rounded float32 square root of the Fraction x >= 0, as a Fraction"""
    if x == 0:
        return Fraction(0)
    import math
    e = (x.numerator.bit_length() - x.denominator.bit_length()) // 2
    quantum = Fraction(2) ** (max(e, -126) - 23)
    while True:
        y = x / (quantum * quantum)
        n = math.isqrt(y.numerator // y.denominator)
        if n >= 2 ** 24:
            quantum *= 2
        elif n < 2 ** 23 and quantum > Fraction(2) ** -149:
            quantum /= 2
        else:
            break
    if y > (Fraction(2 * n + 1, 2)) ** 2:   # (a square root is never exactly half way between two floats)
        n += 1
    return n * quantum


def _fr(z):
    return Fraction(float(z))


def _exact_step(x, m, v, g, lr, beta1, beta2, bc1, bc2, eps, lo, hi):
    """refit_ref._adam and the clamp on Fractions, every operation rounded once by _round32"""
    r32 = _round32
    omb1, omb2 = _fr(F(1.0) - F(beta1)), _fr(F(1.0) - F(beta2))
    beta1, beta2, lr, eps = _fr(F(beta1)), _fr(F(beta2)), _fr(F(lr)), _fr(F(eps))
    m1 = r32(r32(beta1 * m) + r32(omb1 * g))
    v1 = r32(r32(beta2 * v) + r32(omb2 * r32(g * g)))
    s = r32(r32(m1 / bc1) / r32(_sqrt32(r32(v1 / bc2)) + eps))
    x1 = r32(x - r32(lr * s))
    return min(max(x1, lo), hi), m1, v1


def _exact_run(case, first, steps, rows):
    """Steps first + 1 .. first + steps of a case on the DC, the opacity and the first rest coefficient of `rows`, from the numpy
    state after step `first`: ({key: (rows, ...) float64} expected from exact arithmetic, the numpy state to compare with)."""
    ex = E.expected(case, "step_sh")
    keys = ("master", "m", "v", "sh_master", "sh_m", "sh_v")
    if first:
        start = {k: getattr(ex.snaps[first], k) for k in keys}
    else:
        h4, rest = E.start_halves(case)
        start = dict(master=h4.astype(F), m=np.zeros(h4.shape, F), v=np.zeros(h4.shape, F),
                     sh_master=rest.astype(F), sh_m=np.zeros(rest.shape, F), sh_v=np.zeros(rest.shape, F))
    width = {k: 3 if k.startswith("sh_") else 4 for k in keys}   # (of the rest elements: coefficient 1 alone)
    state = {k: [[_fr(z) for z in np.ravel(start[k][r])[:width[k]]] for r in rows] for k in keys}
    p1 = p2 = 1.0
    for st in case.steps[:first]:
        p1, p2 = p1 * float(F(st["adam"]["beta1"])), p2 * float(F(st["adam"]["beta2"]))
    for k in range(first + 1, first + steps + 1):
        st = case.steps[k - 1]
        a = st["adam"]
        p1, p2 = p1 * float(F(a["beta1"])), p2 * float(F(a["beta2"]))
        bc1, bc2 = _fr(F(1.0 - p1)), _fr(F(1.0 - p2))
        for j, r in enumerate(rows):
            for ch in range(4):
                u = st["colour_unit"] * E.C0 if ch < 3 else st["opacity_unit"]
                q = int(st["q_sh"][r, 0, ch]) if ch < 3 else int(st["q_o"][r])
                g = _round32(Fraction(float(q) * u))   # (the product is a double, as on the host and the device)
                x = state["master"][j][ch]
                if ch == 3:
                    g = Fraction(0) if x == 0 else _round32(g / x)
                lo, hi = (Fraction(-65504), Fraction(65504)) if ch < 3 else (_fr(F(a["opacity_min"])), Fraction(1))
                lr = a["lr_colour"] if ch < 3 else a["lr_opacity"]
                state["master"][j][ch], state["m"][j][ch], state["v"][j][ch] = _exact_step(
                    x, state["m"][j][ch], state["v"][j][ch], g, lr, a["beta1"], a["beta2"], bc1, bc2, a["eps"], lo, hi)
            for ch in range(3):
                g = _round32(Fraction(float(int(st["q_sh"][r, 1, ch])) * st["colour_unit"]))
                state["sh_master"][j][ch], state["sh_m"][j][ch], state["sh_v"][j][ch] = _exact_step(
                    state["sh_master"][j][ch], state["sh_m"][j][ch], state["sh_v"][j][ch], g, a["lr_sh"], a["beta1"], a["beta2"], bc1, bc2,
                    a["eps"], Fraction(-65504), Fraction(65504))
    want = ex.snaps[first + steps]
    got = {k: np.array([[float(z) for z in row] for row in v]) for k, v in state.items()}
    twin = {k: np.array([np.ravel(getattr(want, k)[r])[:width[k]] for r in rows], np.float64) for k in keys}
    return got, twin


def test_round32_is_float32_rounding():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(200) * 10.0 ** rng.integers(-46, 30, 200), [2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -149 * 1.5, 2.0 ** -126 * (1 - 2.0 ** -25),
                                                                                       1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -151]])
    for x in xs:
        assert float(_round32(Fraction(float(x)))) == float(F(x)), x
    for x in np.abs(xs):
        x32 = F(x)
        assert float(_sqrt32(Fraction(float(x32)))) == float(np.sqrt(x32)), x


@pytest.mark.parametrize("family,name,first", [("decay", "decay", 589), ("decay", "decay", 598), ("tiny_g", "2^-140", 0), ("tiny_g", "2^-75", 0),
                                               ("tiny_g", "2^-70", 0), ("tiny_g", "2^-64", 0)])
def test_numpy_twin_agrees_with_exact_arithmetic_on_denormals(family, name, first):
    case = next(c for c in E.family(family, 3) if c.name == name)
    rows = list(range(12)) + [40, 63, 64]
    got, want = _exact_run(case, first, 2, rows)
    ex = E.expected(case, "step_sh")
    assert sum(ex.per_step[first][j] + ex.per_step[first + 1][j] for j in (1, 2)) == 0 and ex.per_step[first][0] + ex.per_step[first + 1][0] > 0
    denormal = 0
    for k in got:
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4])
        denormal += int(((got[k] != 0) & (np.abs(got[k]) < TINY)).sum())
    print(family, name, "after step", first + 2, "denormal moments among the compared:", denormal)
    assert denormal > 0


REACHED.update({
    "decay": {
        "decay": {"a": [1502345, 0, 0], "m1": [1502345, 0, 0], "mh": [1502345, 0, 0], "s": [669708, 0, 0], "t": [962814, 0, 0]},
    },
    "tiny_g": {
        "2^-140": {"g": [22036, 0, 0], "a": [11018, 0, 0], "b": [22036, 0, 0], "m1": [22036, 0, 0], "mh": [22036, 0, 0], "gu": [448,
                   0, 0]},
        "2^-75": {"gg": [21842, 0, 0], "c": [4594, 0, 0], "d": [9188, 0, 0], "v1": [9188, 0, 0], "vh": [9188, 0, 0]},
        "2^-70": {"gg": [16252, 0, 0], "c": [11018, 0, 0], "d": [22036, 0, 0], "v1": [22036, 0, 0], "vh": [16252, 0, 0]},
        "2^-64": {"gg": [194, 0, 0], "c": [7966, 0, 0], "d": [15932, 0, 0], "v1": [14390, 0, 0], "vh": [226, 0, 0]},
    },
    "overflow": {
        "finite_and_gg_inf": {"gg": [0, 5038, 0], "c": [0, 5038, 0], "d": [0, 5038, 0], "v1": [0, 10076, 0], "vh": [0, 10076, 0],
                              "r": [0, 10076, 0], "den": [0, 10076, 0]},
        "gg_inf_and_g_inf": {"g": [0, 5038, 103], "a": [0, 5038, 0], "b": [0, 5038, 103], "m1": [0, 9973, 103], "gg": [0, 10075,
                             103], "c": [0, 10075, 0], "d": [0, 10075, 103], "v1": [0, 20047, 103], "mh": [0, 9973, 103], "vh": [0,
                             20047, 103], "r": [0, 20047, 103], "den": [0, 20047, 103], "s": [0, 0, 10076], "t": [0, 0, 10076],
                             "x1": [0, 0, 10076]},
    },
    "hostile_halves": {
        "ordinary": {"g": [0, 0, 46], "b": [0, 0, 46], "m1": [0, 0, 46], "gg": [0, 0, 46], "d": [0, 0, 46], "v1": [0, 0, 46], "mh":
                     [0, 0, 46], "vh": [0, 0, 46], "r": [0, 0, 46], "den": [0, 0, 46], "s": [0, 0, 46], "t": [0, 0, 46], "x1": [0,
                     2287, 2286]},
        "only_colour": {"g": [0, 0, 46], "b": [0, 0, 46], "m1": [0, 0, 46], "gg": [0, 0, 46], "d": [0, 0, 46], "v1": [0, 0, 46],
                        "mh": [0, 0, 46], "vh": [0, 0, 46], "r": [0, 0, 46], "den": [0, 0, 46], "s": [0, 0, 46], "t": [0, 0, 46],
                        "x1": [0, 2287, 2424]},
        "only_opacity": {"g": [0, 0, 92], "a": [0, 0, 46], "b": [0, 0, 92], "m1": [0, 0, 92], "gg": [0, 0, 92], "c": [0, 0, 46],
                         "d": [0, 0, 92], "v1": [0, 0, 92], "mh": [0, 0, 92], "vh": [0, 0, 92], "r": [0, 0, 92], "den": [0, 0, 92],
                         "s": [0, 0, 92], "t": [0, 0, 92], "x1": [0, 2287, 2332]},
        "only_sh": {"g": [0, 0, 46], "b": [0, 0, 46], "m1": [0, 0, 46], "gg": [0, 0, 46], "d": [0, 0, 46], "v1": [0, 0, 46], "mh":
                    [0, 0, 46], "vh": [0, 0, 46], "r": [0, 0, 46], "den": [0, 0, 46], "s": [0, 0, 46], "t": [0, 0, 46], "x1": [0,
                    2287, 4388]},
    },
    "ties": {
        "near_one_0": {},
        "near_one_1": {},
        "near_one_2": {},
        "top": {},
        "subnormal_0": {},
        "subnormal_1": {},
        "subnormal_2": {},
    },
    "params": {
        "beta1_0": {},
        "beta2_0": {},
        "eps_smallest": {"den": [7104, 0, 0]},
        "eps_3e38": {"s": [9704, 0, 0], "t": [18078, 0, 0]},
        "opacity_min_1": {},
        "lr_3e38": {"t": [0, 8940, 0], "x1": [0, 8940, 0]},
    },
})
