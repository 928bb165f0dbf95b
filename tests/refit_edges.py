"""Edge inputs for the refit steps (include/websplat.h "Refitting colour and opacity"; refit.hip k_refit_init, k_refit_init_sh,
k_refit_step, k_refit_step_sh): six families of clouds and step lists that take tests/refit_ref.py and tests/sh_refit_ref.py, used
as they are, into denormal intermediates, overflow to infinity and NaN, non-finite and subnormal halves as masters, and ties of
the f16 store.  Plain numpy, no GPU: tests/test_refit_edges.py shows what each family reaches and which defect it catches,
tests/test_gpu_refit_edges.py compares the device with expected() word for word.

   decay           one step of sums, then zero sums to step 1200: the moments decay into the denormal range and stick there
   tiny_g          gradients of 2^-140, 2^-75, 2^-70 and 2^-64: denormal g, g * g, v'
   overflow        |g| in [2^63, 2^64), g * g = inf, g = inf; the opacity through a master of 2^-40
   hostile_halves  +-0, subnormal, largest finite, infinite and NaN halves as DC, opacity and rest masters; frozen groups
   ties            beta1 = beta2 = 0, s = +-1: x' on and beside ties of the f16 store, at the top and in the subnormal halves
   params          beta1 = 0, beta2 = 0, eps = 2^-149, eps = 3e38, opacity_min = 1, lr = 3e38

A family is a list of Case (one cloud and its steps each); family(name, sh_deg, n) builds it, the patterns in rotation over the
Gaussians so that wave and block edges see every one of them.  A case runs through one of KERNELS: "step" (ws_refit_step on the DC
sums and the opacity sum), "step_sh0" (ws_refit_step_sh with lr_sh = 0) and "step_sh" (ws_refit_step_sh as the case says)."""
import dataclasses
import functools

import numpy as np

import ply_encode_ref
import refit_ref
import sh_refit_ref as ref

F = np.float32
C0 = refit_ref.C0

# A reference that flushed denormals would agree with a kernel that flushes them.
assert np.float32(np.finfo(np.float32).tiny) * np.float32(0.5) != 0, "this host flushes float32 denormals: the reference cannot be trusted"

NAMES = tuple("g a b m1 gg c d v1 mh vh r den s t x1".split())   # refit_ref._adam's intermediates, in the order it traces them
FAMILIES = ("decay", "tiny_g", "overflow", "hostile_halves", "ties", "params")
KERNELS = ("step", "step_sh0", "step_sh")
N_DEFAULT = {"decay": 65}
UNIT = 2.0 ** -32

HOSTILE = np.array([0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7D00], np.uint16)
# what the halves no step may write hold: NaN (quiet, signalling, negative with a payload), both infinities, noise, a subnormal, -0
FILL = np.array([0x7E00, 0x7C00, 0xFC00, 0x7D00, 0xFE01, 0x3555, 0xB8E1, 0x0001, 0x8000], np.uint16)


def ncoef(sh_deg):
    return ref.ncoef(sh_deg)


def h16(x):
    """float16 bit patterns of x (exact values expected)"""
    h = np.asarray(x, np.float64).astype(np.float16)
    assert np.array_equal(h.astype(np.float64), np.asarray(x, np.float64)), "not a half"
    return h.view(np.uint16)


def unit_for(u_c):
    """a colour_unit whose product with C0, in double, is exactly u_c when a neighbour of u_c / C0 gives that, else u_c / C0"""
    c = u_c / C0
    for cand in [c] + [np.nextafter(c, s * np.inf) for s in (1, -1)]:
        if float(cand) * C0 == u_c:
            return float(cand)
    for s in (1, -1):
        cand = c
        for _ in range(8):
            cand = np.nextafter(cand, s * np.inf)
            if float(cand) * C0 == u_c:
                return float(cand)
    return float(c)


@dataclasses.dataclass
class Case:
    family: str
    name: str
    sh_deg: int
    g: np.ndarray        # (N, 28) uint8
    s: np.ndarray        # (N, 96) uint8
    steps: list          # dicts: q_sh (N, ncoef, 3) int64, q_o (N,) int64, zero (all sums 0), colour_unit, opacity_unit, adam
    checks: tuple        # the steps after which the device is compared; 0: after create and enable_sh

    @property
    def n(self):
        return self.g.shape[0]


def _rot(values, n, slots, stride=1):
    """values[(i + stride * slot) % len]: (n, slots)"""
    v = np.asarray(values)
    return v[(np.arange(n)[:, None] + stride * np.arange(slots)[None, :]) % len(v)]


def _blobs(n, sh_deg, dc, op, rest, seed=0):
    """Blobs as ply_encode_ref.edges() builds them: dc (n, 3), op (n,), rest (n, 3 (ncoef - 1)) uint16 halves; every SH half past
    3 ncoef and the two bytes beside the opacity hold FILL patterns in rotation."""
    nc = ncoef(sh_deg)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, size=(N_MAX, 3)).astype(F)[:n]
    cov = np.broadcast_to(h16([2.0 ** -7, 0.0, 0.0, 2.0 ** -7, 0.0, 2.0 ** -7]), (n, 6))
    sh = _rot(FILL, n, 48, stride=4).astype(np.uint16)
    sh[:, :3] = dc
    if nc > 1:
        sh[:, 3:3 * nc] = rest
    g, s = ply_encode_ref.join(pos, np.asarray(op, np.uint16), cov, sh)
    g[:, 14:16] = np.ascontiguousarray(_rot(FILL, n, 1, stride=2).astype(np.uint16)).view(np.uint8).reshape(n, 2)
    return g, s


def _quiet(n, sh_deg):
    """normal halves for every parameter"""
    nr = 3 * (ncoef(sh_deg) - 1)
    return (_rot(h16([0.5, -0.25, 1.0, -1.5, 0.75]), n, 3), _rot(h16([0.5, 0.25, 1.0, 0.125]), n, 1)[:, 0],
            _rot(h16([0.125, -0.0625, 0.03125, -0.25]), n, nr, stride=3))


def _adam(**kw):
    return dict(dict(lr_colour=0.0025, lr_opacity=0.01, lr_sh=0.000125, beta1=0.9, beta2=0.999, eps=1e-15, opacity_min=0.0), **kw)


def _step(q_sh, q_o, adam, colour_unit=UNIT, opacity_unit=UNIT):
    q_sh, q_o = np.ascontiguousarray(q_sh, np.int64), np.ascontiguousarray(q_o, np.int64)
    return dict(q_sh=q_sh, q_o=q_o, zero=not (q_sh.any() or q_o.any()), colour_unit=float(colour_unit), opacity_unit=float(opacity_unit),
                adam=adam)


def _zeros(n, nc):
    return np.zeros((n, nc, 3), np.int64), np.zeros(n, np.int64)


N_MAX = 1024


def _well_scaled(rng, shape):
    """int64 sums of 2^24 .. 2^41 in magnitude with random low bits, both signs, one in ten exactly 0.  Drawn for N_MAX Gaussians
    and cut: Gaussian i gets the same sums in a cloud of any size."""
    n, shape = shape[0], (N_MAX,) + tuple(shape[1:])
    assert n <= N_MAX
    v = rng.integers(2 ** 40, 2 ** 41, size=shape, dtype=np.int64) >> rng.integers(0, 17, size=shape, dtype=np.int64)
    v *= rng.choice(np.array([-1, 1], np.int64), size=shape)
    v[rng.uniform(size=shape) < 0.1] = 0
    return v[:n].copy()


# ---- the families ----------------------------------------------------------------------------------------------------------------
DECAY_QUOTED = (2 ** 20, -(2 ** 8), 2 ** 40, 1)   # the one-shot sums of Gaussians 0 .. 3, on all their channels
DECAY_STEPS = 1200
DECAY_CHECKS = tuple(range(580, 601)) + (900, 1100, 1200)   # (1100: the last hundred steps change nothing)


def _decay(sh_deg, n):
    nc = ncoef(sh_deg)
    dc = np.broadcast_to(h16([0.5, -0.25, 1.0]), (n, 3))
    op = np.full(n, h16(0.5))
    rest = _quiet(n, sh_deg)[2]
    i = np.arange(n)
    expo = (i[:, None, None] + 7 * np.arange(nc)[None, :, None] + 3 * np.arange(3)[None, None, :]) % 41
    sign = np.where((i[:, None, None] + np.arange(nc)[None, :, None] + np.arange(3)[None, None, :]) % 2 == 0, 1, -1)
    q_sh = sign * (np.int64(1) << expo.astype(np.int64))
    q_o = np.where(i % 2 == 0, -1, 1) * (np.int64(1) << ((5 * i) % 41).astype(np.int64))
    for j, v in enumerate(DECAY_QUOTED[:min(n, 4)]):
        q_sh[j], q_o[j] = v, v
    adam = _adam(opacity_min=2.0 ** -7)
    first = _step(q_sh, q_o, adam)
    rest_step = _step(*_zeros(n, nc), adam)
    g, s = _blobs(n, sh_deg, dc, op, rest)
    return [Case("decay", "decay", sh_deg, g, s, [first] + [rest_step] * (DECAY_STEPS - 1), DECAY_CHECKS)]


TINY_Q = (1, 3, -5, 7, -45, 91, -13, 0)
TINY_EXPONENTS = (140, 75, 70, 64)


def _tiny_g(sh_deg, n):
    nc = ncoef(sh_deg)
    dc, _, rest = _quiet(n, sh_deg)
    op = _rot(h16([1.0, 0.5]), n, 1)[:, 0]   # (g / x is g or 2 g, exactly)
    q_sh = _rot(np.array(TINY_Q, np.int64), n, 3 * nc).reshape(n, nc, 3)
    q_o = _rot(np.array(TINY_Q[::-1], np.int64), n, 1)[:, 0]
    out = []
    for e in TINY_EXPONENTS:
        g, s = _blobs(n, sh_deg, dc, op, rest, seed=e)
        st = _step(q_sh, q_o, _adam(), colour_unit=unit_for(2.0 ** -e), opacity_unit=2.0 ** -e)
        out.append(Case("tiny_g", f"2^-{e}", sh_deg, g, s, [st, st], (1, 2)))
    return out


INF = float("inf")
OVERFLOW = {   # per case: u_c = colour_unit * C0, the opacity's unit (its master is 2^-40), the gradients aimed at, in rotation
    "finite_and_gg_inf": (2.0 ** 40, 2.0 ** 20, (1.5 * 2.0 ** 63, -1.25 * 2.0 ** 63, 2.0 ** 70, -(2.0 ** 90), 0.0)),
    "gg_inf_and_g_inf": (2.0 ** 70, 2.0 ** 30, (3.0 * 2.0 ** 70, -(2.0 ** 100), INF, -INF, 0.0)),
}
OVERFLOW_LR1 = 2.0 ** -24 - 2.0 ** -40   # exact in f32: the step from the half 2^-24 to the master 2^-40


def _sums_for(targets, u):
    """int64 sums q with q * u near the targets; +-2^62 for an infinite one"""
    t = np.asarray(targets, np.float64)
    with np.errstate(all="ignore"):
        q = np.where(np.isinf(t), np.sign(t) * 2.0 ** 62, np.rint(t / u))
    assert (np.abs(q) <= 2.0 ** 62).all()
    return q.astype(np.int64)


def _overflow(sh_deg, n):
    nc = ncoef(sh_deg)
    dc, _, rest = _quiet(n, sh_deg)
    op = np.full(n, h16(2.0 ** -24))
    out = []
    for name, (u_c, u_o, targets) in OVERFLOW.items():
        cu = unit_for(u_c)
        g, s = _blobs(n, sh_deg, dc, op, rest, seed=len(name))
        # 1: betas 0, s = 1 exactly, the opacity alone: 2^-24 - (2^-24 - 2^-40) = 2^-40
        q_sh, q_o = _zeros(n, nc)
        q_o[:] = 2 ** 20
        one = _step(q_sh, q_o, _adam(lr_colour=0.0, lr_sh=0.0, lr_opacity=OVERFLOW_LR1, beta1=0.0, beta2=0.0))
        # 2: the regimes, in rotation over Gaussians and slots
        q_sh = np.empty((n, nc, 3), np.int64)
        q_sh[:, 0, :] = _rot(_sums_for(targets, u_c), n, 3)
        if nc > 1:
            q_sh[:, 1:, :] = _rot(_sums_for(targets, cu), n, 3 * (nc - 1), stride=2).reshape(n, nc - 1, 3)
        q_o = _rot(_sums_for(targets[::-1], u_o * 2.0 ** 40), n, 1)[:, 0]
        big = _adam(lr_colour=0.01, lr_opacity=0.01, lr_sh=0.01)
        two = _step(q_sh, q_o, big, colour_unit=cu, opacity_unit=u_o)
        # 3: zero sums
        three = _step(*_zeros(n, nc), big, colour_unit=cu, opacity_unit=u_o)
        out.append(Case("overflow", name, sh_deg, g, s, [one, two, three], (1, 2, 3)))
    return out


HOSTILE_RATES = dict(lr_colour=0.0025, lr_opacity=0.05, lr_sh=0.002)


def _hostile_halves(sh_deg, n):
    nc = ncoef(sh_deg)
    allh = _rot(HOSTILE, n, 49)
    dc, rest, op = allh[:, :3], allh[:, 3:3 * nc], allh[:, 48]
    rng = np.random.default_rng(11)
    out = []
    for name in ("ordinary", "only_colour", "only_opacity", "only_sh"):
        g, s = _blobs(n, sh_deg, dc, op, rest, seed=3)
        ordinary = _step(_well_scaled(rng, (n, nc, 3)), _well_scaled(rng, (n,)), _adam(**HOSTILE_RATES))
        steps = [ordinary]
        if name != "ordinary":
            live = {"only_colour": "lr_colour", "only_opacity": "lr_opacity", "only_sh": "lr_sh"}[name]
            frozen = _adam(lr_colour=0.0, lr_opacity=0.0, lr_sh=0.0)
            frozen[live] = HOSTILE_RATES[live]
            steps = [_step(_well_scaled(rng, (n, nc, 3)), _well_scaled(rng, (n,)), frozen), ordinary]
        out.append(Case("hostile_halves", name, sh_deg, g, s, steps, tuple(range(len(steps) + 1))))
    return out


def _signed_rot(masters, n, slots, q, stride=1):
    """masters in rotation and, per turn of the rotation, sums of +q and -q; a master of -0 gets the sum 0"""
    m = np.asarray(masters, np.float64)
    k = np.arange(n)[:, None] + stride * np.arange(slots)[None, :]
    x = m[k % len(m)]
    sums = np.where((k // len(m)) % 2 == 0, q, -q).astype(np.int64)
    sums[(x == 0) & np.signbit(x)] = 0
    return h16(x), sums


TIES_NEAR_ONE = (1.0, 1.0 + 2.0 ** -10, -(1.0 + 3 * 2.0 ** -10), -1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), -0.0)
TIES_OPACITY = (0.5, 0.5 + 2.0 ** -11, 0.75, 1.0 - 2.0 ** -11, 0.5 + 3 * 2.0 ** -11)
TIES_TOP = (65504.0, 65472.0, -65504.0, -65472.0, 65440.0, -0.0)
TIES_SUB = tuple(k * 2.0 ** -24 for k in (1, 2, 3, 4, 5, 1023, 1024)) + tuple(-k * 2.0 ** -24 for k in (1, 2, 3, 1023)) + (-0.0,)
TIES_SUB_OPACITY = tuple(k * 2.0 ** -24 for k in (1, 2, 3, 4, 5, 1023, 1024))
# rates that are a tie distance, and one f32 ulp of x' more and less: halves in [1, 2) step by 2^-10, in [0.5, 1) by 2^-11
TIES_LR = (2.0 ** -11, 2.0 ** -11 + 2.0 ** -23, 2.0 ** -11 - 2.0 ** -23)
TIES_LR_OPACITY = (2.0 ** -12, 2.0 ** -12 + 2.0 ** -24, 2.0 ** -12 - 2.0 ** -24)
# subnormal halves step by 2^-24: onto a tie, beside it, and from 2^-24 down to 2^-26
TIES_LR_SUB = (2.0 ** -25, 2.0 ** -25 * (1.0 - 2.0 ** -20), 3 * 2.0 ** -26)


def _ties(sh_deg, n):
    nc = ncoef(sh_deg)
    nr = 3 * (nc - 1)
    cu = unit_for(UNIT)   # colour_unit * C0 = 2^-32 exactly: g = +-1 on the DC, +-1 / C0 on the rest, +-1 / x on the opacity
    out = []

    def case(name, masters, op_masters, lr_colour, lr_sh, lr_opacity):
        dc, q_dc = _signed_rot(masters, n, 3, 2 ** 32)
        rest, q_rest = _signed_rot(masters, n, nr, 2 ** 32, stride=2) if nr else (None, None)
        op, q_o = _signed_rot(op_masters, n, 1, 2 ** 32)
        g, s = _blobs(n, sh_deg, dc, op[:, 0], rest, seed=len(out))
        q_sh = np.zeros((n, nc, 3), np.int64)
        q_sh[:, 0, :] = q_dc
        if nr:
            q_sh[:, 1:, :] = q_rest.reshape(n, nc - 1, 3)
        st = _step(q_sh, q_o[:, 0], _adam(lr_colour=lr_colour, lr_sh=lr_sh, lr_opacity=lr_opacity, beta1=0.0, beta2=0.0), colour_unit=cu)
        out.append(Case("ties", name, sh_deg, g, s, [st], (1,)))

    for j in range(3):
        case(f"near_one_{j}", TIES_NEAR_ONE, TIES_OPACITY, TIES_LR[j], TIES_LR[(j + 1) % 3], TIES_LR_OPACITY[(j + 2) % 3])
    case("top", TIES_TOP, TIES_OPACITY, 8.0, 16.0, TIES_LR_OPACITY[0])
    for j in range(3):
        case(f"subnormal_{j}", TIES_SUB, TIES_SUB_OPACITY, TIES_LR_SUB[j], TIES_LR_SUB[(j + 1) % 3], TIES_LR_SUB[(j + 2) % 3])
    return out


PARAMS = {
    "beta1_0": dict(beta1=0.0),
    "beta2_0": dict(beta2=0.0),
    "eps_smallest": dict(eps=2.0 ** -149),
    "eps_3e38": dict(eps=3e38),
    "opacity_min_1": dict(opacity_min=1.0),
    "lr_3e38": dict(lr_colour=3e38, lr_opacity=3e38, lr_sh=3e38, beta1=0.0),
}


def _params(sh_deg, n):
    nc = ncoef(sh_deg)
    dc, op, rest = _quiet(n, sh_deg)
    out = []
    for k, (name, kw) in enumerate(PARAMS.items()):
        rng = np.random.default_rng(50 + k)
        g, s = _blobs(n, sh_deg, dc, op, rest, seed=k)
        q_sh, q_o = _well_scaled(rng, (n, nc, 3)), _well_scaled(rng, (n,))
        q_sh[np.arange(n) % 5 == 2], q_o[np.arange(n) % 5 == 2] = 0, 0   # (whole Gaussians of zero sums: 0 / eps)
        adam = _adam(**dict(HOSTILE_RATES, **kw))
        out.append(Case("params", name, sh_deg, g, s, [_step(q_sh, q_o, adam), _step(4 * q_sh, 4 * q_o, adam)], (1, 2)))
    return out


_BUILD = dict(decay=_decay, tiny_g=_tiny_g, overflow=_overflow, hostile_halves=_hostile_halves, ties=_ties, params=_params)


@functools.lru_cache(maxsize=None)
def _family(name, sh_deg, n):
    cases = _BUILD[name](sh_deg, n)
    for c in cases:
        c.g.setflags(write=False)
        c.s.setflags(write=False)
    return cases


def family(name, sh_deg=3, n=None):
    """the list of Case of a family at a degree; n: 257 (65 for decay) unless given"""
    return _family(name, int(sh_deg), int(n or N_DEFAULT.get(name, 257)))


# ---- what the reference makes of a case ----------------------------------------------------------------------------------------------
def start_halves(case):
    """(N, 4) float16 DC and opacity, (N, ncoef - 1, 3) float16 rest: what create and enable_sh widen"""
    sh16 = np.ascontiguousarray(case.s).view(np.uint16).reshape(case.n, 48)
    op16 = np.ascontiguousarray(case.g[:, 12:14]).view(np.uint16).reshape(case.n, 1)
    nc = ncoef(case.sh_deg)
    return (np.concatenate([sh16[:, :3], op16], axis=1).view(np.float16),
            np.ascontiguousarray(sh16[:, 3:3 * nc]).view(np.float16).reshape(case.n, nc - 1, 3))


def classes(trace):
    """{name: [denormal, infinite, NaN]}: how many values of each of refit_ref._adam's intermediates, over every group a trace
    holds, are denormal, infinite or NaN.  (The opacity's gradient before its division by the master, which refit_ref.step traces
    ahead of the fifteen, is counted as "gu".)"""
    out = {k: [0, 0, 0] for k in NAMES + ("gu",)}
    tiny = np.finfo(F).tiny
    i = 0
    while i < len(trace):
        j = i
        while j < len(trace) and np.shape(trace[j]) == np.shape(trace[i]):
            j += 1
        run = trace[i:j]
        assert len(run) in (15, 16), "a trace is made of refit_ref._adam's fifteen, the opacity's of sixteen"
        for name, z in zip((("gu",) if len(run) == 16 else ()) + NAMES, run):
            z = np.asarray(z)
            out[name][0] += int(((z != 0) & np.isfinite(z) & (np.abs(z) < tiny)).sum())
            out[name][1] += int(np.isinf(z).sum())
            out[name][2] += int(np.isnan(z).sum())
        i = j
    return out


def _add(total, part):
    for k, v in part.items():
        for j in range(3):
            total[k][j] += v[j]


def requantised(bits):
    """uint16 halves through f16 -> f32 -> f16 as the hardware converts: a signalling NaN comes back quiet"""
    bits = np.asarray(bits, np.uint16)
    nan = ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)
    return np.where(nan, bits | 0x0200, bits).astype(np.uint16)


@dataclasses.dataclass
class Snapshot:
    master: np.ndarray
    m: np.ndarray
    v: np.ndarray
    sh_master: np.ndarray
    sh_m: np.ndarray
    sh_v: np.ndarray
    g: np.ndarray          # the expected blobs
    s: np.ndarray
    written: np.ndarray    # (49,) bool: SH halves 0 .. 47 and the opacity half that some step so far has stored (computed values)


@dataclasses.dataclass
class Expected:
    snaps: dict            # check -> Snapshot
    classes: dict          # classes() over every step
    per_step: list         # [denormal, infinite, NaN] over all intermediates, per step


def step_args(st, kernel):
    """the Adam arguments of a step as `kernel` takes them"""
    a = dict(st["adam"])
    if kernel == "step":
        a.pop("lr_sh")
    elif kernel == "step_sh0":
        a["lr_sh"] = 0.0
    return a


def _store(g, s, state, adam, kernel, sh_deg, written, defect):
    """the bytes one step writes, into the expected blobs"""
    n, nc = g.shape[0], ncoef(sh_deg)
    sh16 = s.view(np.uint16).reshape(n, 48)
    g16 = g.view(np.uint16).reshape(n, 14)
    colour, opacity = F(adam["lr_colour"]) != 0, F(adam["lr_opacity"]) != 0
    rest = kernel != "step" and F(adam["lr_sh"]) != 0 and nc > 1
    stepped = np.zeros(49, bool)
    if colour:
        sh16[:, :3] = state.halves(defect)[:, :3].view(np.uint16)
        stepped[:3] = True
    if opacity:
        g16[:, 6] = state.halves(defect)[:, 3].view(np.uint16)
        stepped[48] = True
    if rest:
        sh16[:, 3:3 * nc] = state.rest_halves(defect).reshape(n, -1).view(np.uint16)
        stepped[3:3 * nc] = True
    written |= stepped
    if defect == "rewiden_unstepped":
        stored = np.zeros(48, bool)   # the halves of the chunks (words, under ws_refit_step) the step stores
        if kernel == "step":
            stored[:4] = colour
        else:
            planes = (3 * nc + 7) // 8 if (kernel == "step_sh" and F(adam["lr_sh"]) != 0) else int(colour)
            stored[:8 * planes] = True
        again = stored & ~stepped[:48]
        sh16[:, again] = requantised(sh16[:, again])
        if opacity:
            g16[:, 7] = requantised(g16[:, 7])


@functools.lru_cache(maxsize=None)
def _expected(name, sh_deg, n, index, kernel, defect):
    case = family(name, sh_deg, n)[index]
    state = ref.ShState(*start_halves(case))
    g, s = case.g.copy(), case.s.copy()
    written = np.zeros(49, bool)
    snaps, total, per_step = {}, {k: [0, 0, 0] for k in NAMES + ("gu",)}, []

    def snap():
        return Snapshot(*(getattr(state, k).copy() for k in ("master", "m", "v", "sh_master", "sh_m", "sh_v")), g.copy(), s.copy(), written.copy())

    if 0 in case.checks:
        snaps[0] = snap()
    for k, st in enumerate(case.steps, start=1):
        adam = step_args(st, kernel)
        trace = []
        if kernel == "step":
            refit_ref.step(state, np.concatenate([st["q_sh"][:, 0, :], st["q_o"][:, None]], axis=1), st["colour_unit"], st["opacity_unit"],
                           trace=trace, defect=defect, **adam)
        else:
            ref.step_sh(state, st["q_sh"], st["q_o"], st["colour_unit"], st["opacity_unit"], trace=trace, defect=defect, **adam)
        _store(g, s, state, adam, kernel, sh_deg, written, defect)
        c = classes(trace)
        _add(total, c)
        per_step.append([sum(v[j] for v in c.values()) for j in range(3)])
        if k in case.checks:
            snaps[k] = snap()
    return Expected(snaps, total, per_step)


def expected(case, kernel, defect=None):
    """What refit_ref / sh_refit_ref make of a case under a kernel: the state and the blobs at every check, the classes met."""
    cases = family(case.family, case.sh_deg, case.n)
    index = [c.name for c in cases].index(case.name)
    assert cases[index] is case
    return _expected(case.family, case.sh_deg, case.n, index, kernel, defect)


def rounding_kinds(x):
    """How the f16 store rounds each finite value of x (float32): counts of exact, down and up (in magnitude), tie_to_even_down,
    tie_to_even_up, and of results that are subnormal halves or a zero from a value that is not."""
    x = np.asarray(x, F).ravel()
    x = x[np.isfinite(x)]
    with np.errstate(all="ignore"):
        h = x.astype(np.float16)
    ax, ah = np.abs(x.astype(np.float64)), np.abs(h.astype(np.float64))
    bits = h.view(np.uint16) & 0x7FFF
    with np.errstate(all="ignore"):
        lo = np.where(ah <= ax, bits, bits - 1).astype(np.uint16).view(np.float16).astype(np.float64)
        hi = np.where(ah >= ax, bits, bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    tie = (ah != ax) & np.isfinite(hi) & (ax - lo == hi - ax)
    return dict(exact=int((ah == ax).sum()), down=int(((ah < ax) & ~tie).sum()), up=int(((ah > ax) & ~tie).sum()),
                tie_to_even_down=int(((ah < ax) & tie).sum()), tie_to_even_up=int(((ah > ax) & tie).sum()),
                subnormal_half=int(((bits & 0x7C00) == 0).sum() - (bits == 0).sum()), zero_from_nonzero=int(((bits == 0) & (ax != 0)).sum()))
