"""The refit step (include/websplat.h "Refitting colour and opacity") restated in numpy: np.float32 arrays, one rounded operation
per line, the running beta powers Python floats multiplied once per step.  What the device is compared with bit for bit."""
import numpy as np

F = np.float32
C0 = 0.28209479177387814
DC_MAX = F(65504.0)
DEFAULTS = dict(lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999, eps=1e-15, opacity_min=0.0)


class State:
    """master, m, v: (N, 4) float32 -- DC r, g, b and the opacity; steps; p1, p2 = beta^steps as Python floats."""

    def __init__(self, halves):
        h = np.asarray(halves)
        assert h.dtype == np.float16 and h.ndim == 2 and h.shape[1] == 4
        self.master = h.astype(F)
        self.m = np.zeros_like(self.master)
        self.v = np.zeros_like(self.master)
        self.steps = 0
        self.p1 = 1.0
        self.p2 = 1.0

    def halves(self, defect=None):
        """what the step stores in the cloud: the masters to f16, round to nearest even"""
        return store16(self.master, defect)


# What a kernel could get wrong without today's well-scaled inputs noticing (tests/test_refit_edges.py shows that each one is
# caught by a family of tests/refit_edges.py).  defect=None is the step; nothing below changes a result then.
DEFECTS = ("flush_results",          # every f32 result flushed to signed zero (a build without denormals)
           "daz_divide_sqrt",        # denormal inputs read as zero in the divide and the square root only (their expansions)
           "clamp_fmin_fmax",        # the clamp by fmin / fmax: a NaN becomes the bound
           "store_toward_zero",      # the f16 store truncates
           "store_flush_subnormal",  # the f16 store flushes subnormal halves to signed zero
           "rewiden_unstepped",      # unstepped halves of a stored chunk go f16 -> f32 -> f16 (tests/refit_edges.py `requantised`)
           "store_ties_toward_zero") # the f16 store rounds to nearest but takes a tie toward zero instead of to even


def _flushed(z):
    """z with every denormal replaced by a zero of its sign"""
    z = np.asarray(z, F)
    return np.where((z != 0) & (np.abs(z) < np.finfo(F).tiny), np.copysign(F(0), z), z).astype(F)


def _same(z):
    return z


def store16(x, defect=None):
    """f16(x), round to nearest even, subnormal halves honoured"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        h = x.astype(np.float16)
        if defect == "store_toward_zero":
            bits = h.view(np.uint16).copy()
            bits[np.abs(h.astype(F)) > np.abs(x)] -= 1   # (rounded away from zero: one half back; inf from a finite x -> 0x7BFF)
            h = bits.view(np.float16)
        elif defect == "store_ties_toward_zero":
            bits = h.view(np.uint16).copy()
            x64, h64 = x.astype(np.float64), h.astype(np.float64)
            below = (bits - 1).astype(np.uint16).view(np.float16).astype(np.float64)   # one half nearer zero
            tie = (np.abs(h64) > np.abs(x64)) & np.isfinite(h64) & (np.abs(h64 - x64) == np.abs(x64 - below))   # (exact in double)
            bits[tie] -= 1
            h = bits.view(np.float16)
        elif defect == "store_flush_subnormal":
            bits = h.view(np.uint16)
            sub = ((bits & 0x7C00) == 0) & ((bits & 0x03FF) != 0)
            h = np.where(sub, bits & 0x8000, bits).astype(np.uint16).view(np.float16)
    return h


def _adam(g, lr, x, m, v, beta1, beta2, omb1, omb2, bc1, bc2, eps, trace, defect=None):
    out = _flushed if defect == "flush_results" else _same      # on every result
    arg = _flushed if defect == "daz_divide_sqrt" else _same    # on what the divide and the square root read
    g = out(g)
    a = out(beta1 * m)
    b = out(omb1 * g)
    m1 = out(a + b)
    gg = out(g * g)
    c = out(beta2 * v)
    d = out(omb2 * gg)
    v1 = out(c + d)
    mh = out(arg(m1) / arg(bc1))
    vh = out(arg(v1) / arg(bc2))
    r = out(np.sqrt(arg(vh)))
    den = out(r + eps)
    s = out(arg(mh) / arg(den))
    t = out(lr * s)
    x1 = out(x - t)
    if trace is not None:
        trace += [g, a, b, m1, gg, c, d, v1, mh, vh, r, den, s, t, x1]
    for z in (m1, v1, x1):
        assert z.dtype == F
    return x1, m1, v1


def _clamp(x, lo, hi, defect=None):
    if defect == "clamp_fmin_fmax":
        return np.fmin(np.fmax(x, lo), hi).astype(F)
    x = np.where(x < lo, lo, x)
    return np.where(x > hi, hi, x).astype(F)


def step(st, q, colour_unit, opacity_unit, lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999, eps=1e-15, opacity_min=0.0,
         trace=None, defect=None):
    """One step of State st along the (N, 4) int64 sums q, in place.  trace: a list that receives every f32 intermediate.
    defect: one of DEFECTS, for tests that show what the suite would catch."""
    q = np.asarray(q)
    assert q.dtype == np.int64 and q.shape == st.master.shape
    lr_colour, lr_opacity, beta1, beta2, eps, opacity_min = (F(z) for z in (lr_colour, lr_opacity, beta1, beta2, eps, opacity_min))
    st.p1 = st.p1 * float(beta1)
    st.p2 = st.p2 * float(beta2)
    bc1 = F(1.0 - st.p1)
    bc2 = F(1.0 - st.p2)
    omb1 = F(1.0) - beta1
    omb2 = F(1.0) - beta2
    u_c = float(colour_unit) * C0
    u_o = float(opacity_unit)
    with np.errstate(all="ignore"):
        if lr_colour != 0:
            g = (q[:, :3].astype(np.float64) * u_c).astype(F)
            x1, m1, v1 = _adam(g, lr_colour, st.master[:, :3], st.m[:, :3], st.v[:, :3], beta1, beta2, omb1, omb2, bc1, bc2, eps, trace,
                                defect)
            st.master[:, :3] = _clamp(x1, -DC_MAX, DC_MAX, defect)
            st.m[:, :3] = m1
            st.v[:, :3] = v1
        if lr_opacity != 0:
            x = st.master[:, 3]
            g = (q[:, 3].astype(np.float64) * u_o).astype(F)
            if trace is not None:
                trace.append(g)
            if defect == "daz_divide_sqrt":
                g = np.where(x == 0, F(0), _flushed(g) / np.where(x == 0, F(1), _flushed(x))).astype(F)
            else:
                g = np.where(x == 0, F(0), g / np.where(x == 0, F(1), x)).astype(F)
            x1, m1, v1 = _adam(g, lr_opacity, x, st.m[:, 3], st.v[:, 3], beta1, beta2, omb1, omb2, bc1, bc2, eps, trace, defect)
            st.master[:, 3] = _clamp(x1, opacity_min, F(1.0), defect)
            st.m[:, 3] = m1
            st.v[:, 3] = v1
    st.steps += 1
    return st


def all_zero_or_normal(trace):
    """every value of every traced intermediate is 0 or a normal float32 (no denormal, infinity or NaN)"""
    tiny = np.finfo(F).tiny
    return all(bool(np.all((z == 0) | (np.isfinite(z) & (np.abs(z) >= tiny)))) for z in trace)


def adam_f64(x0, grads, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """Plain float64 Adam over a list of gradient arrays (no clamps): what the f32 step approximates."""
    x = np.asarray(x0, np.float64).copy()
    m = np.zeros_like(x)
    v = np.zeros_like(x)
    beta1, beta2, eps, lr = (float(F(z)) for z in (beta1, beta2, eps, lr))
    p1 = p2 = 1.0
    for g in grads:
        p1 *= beta1
        p2 *= beta2
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        x = x - lr * (m / (1.0 - p1)) / (np.sqrt(v / (1.0 - p2)) + eps)
    return x
