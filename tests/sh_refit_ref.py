"""The SH spread and the SH refit step (include/websplat.h "SH gradients"; ws_refit_step_sh) restated in numpy: np.float32 arrays,
one rounded operation per line, int64 sums.  What the device and the host twin are compared with bit for bit; float64 versions of
the direction, the basis and the spread beside them."""
import numpy as np

import refit_ref

F = np.float32
C1 = F(0.4886025119029199)
C2 = [F(v) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
C3 = [F(v) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                     1.445305721320277, -0.5900435899266435)]
SH_MAX = F(65504.0)


def ncoef(deg):
    return (int(deg) + 1) ** 2


def direction(xyz32, cam32):
    """(N, 3) float32: d = xyz - cam, dl = sqrt((dx dx + dy dy) + dz dz), d / dl -- NaN where dl is 0 or xyz is not finite."""
    xyz32, cam32 = np.asarray(xyz32), np.asarray(cam32)
    assert xyz32.dtype == F and cam32.dtype == F
    with np.errstate(all="ignore"):
        d = xyz32 - cam32[None, :]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        dl = np.sqrt((dx * dx + dy * dy) + dz * dz)
        out = d / dl[:, None]
    assert out.dtype == F
    return out


def _basis(x, y, z, two, three, four, c1, c2, c3):
    """columns 1..15 by K1's expressions, left to right; column 3 negated (K1 subtracts that term); column 0 is not used (0)"""
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    b = [np.zeros_like(x),
         (-c1) * y, c1 * z, -(c1 * x),
         c2[0] * xy, c2[1] * yz, c2[2] * ((two * zz - xx) - yy), c2[3] * xz, c2[4] * (xx - yy),
         (c3[0] * y) * (three * xx - yy), (c3[1] * xy) * z, (c3[2] * y) * ((four * zz - xx) - yy),
         (c3[3] * z) * ((two * zz - three * xx) - three * yy), (c3[4] * x) * ((four * zz - xx) - yy), (c3[5] * z) * (xx - yy),
         (c3[6] * x) * (xx - three * yy)]
    return np.stack(b, axis=1)


def basis(dir32):
    """(N, 16) float32: the effective basis of every coefficient at the unit directions dir32 (column 0: unused, 0)."""
    d = np.asarray(dir32)
    assert d.dtype == F
    with np.errstate(all="ignore"):
        out = _basis(d[:, 0], d[:, 1], d[:, 2], F(2), F(3), F(4), C1, C2, C3)
    assert out.dtype == F
    return out


def spread(q4, xyz32, cam32, active_deg, sh_deg=None):
    """One frame's (N, 4) int64 sums spread over the coefficients, to the bit: ((N, ncoef, 3) int64, (N,) int64).  Coefficients
    above active_deg stay 0; a sum of 0 and a basis that is not finite add nothing."""
    q4 = np.asarray(q4)
    assert q4.dtype == np.int64 and q4.ndim == 2 and q4.shape[1] == 4
    sh_deg = active_deg if sh_deg is None else sh_deg
    nact = ncoef(min(active_deg, sh_deg))
    sh = np.zeros((q4.shape[0], ncoef(sh_deg), 3), np.int64)
    sh[:, 0, :] = q4[:, :3]
    if nact > 1:
        bas = basis(direction(xyz32, cam32))[:, :nact].astype(np.float64)
        with np.errstate(all="ignore"):
            prod = q4[:, None, :3].astype(np.float64) * bas[:, :, None]
        ok = np.isfinite(bas)[:, :, None] & (q4[:, None, :3] != 0)
        sh[:, 1:nact, :] = np.where(ok, np.rint(np.where(ok, prod, 0.0)), 0.0).astype(np.int64)[:, 1:, :]
    return sh, q4[:, 3].copy()


def direction64(xyz32, cam32):
    d = np.asarray(xyz32, np.float64) - np.asarray(cam32, np.float64)[None, :]
    with np.errstate(all="ignore"):
        return d / np.sqrt((d * d).sum(axis=1))[:, None]


def basis64(dir64):
    d = np.asarray(dir64, np.float64)
    return _basis(d[:, 0], d[:, 1], d[:, 2], 2.0, 3.0, 4.0, float(C1), [float(c) for c in C2], [float(c) for c in C3])


def spread64(q4, xyz32, cam32, active_deg):
    """The spread in float64 throughout, not rounded to integers: (N, ncoef, 3) float64."""
    bas = basis64(direction64(xyz32, cam32))[:, :ncoef(active_deg)]
    out = np.asarray(q4)[:, None, :3].astype(np.float64) * bas[:, :, None]
    out[:, 0, :] = np.asarray(q4)[:, :3]
    return out


class ShState(refit_ref.State):
    """refit_ref.State and the rest coefficients: sh_master, sh_m, sh_v (N, ncoef - 1, 3) float32."""

    def __init__(self, halves, rest_halves):
        super().__init__(halves)
        r = np.asarray(rest_halves)
        assert r.dtype == np.float16 and r.ndim == 3 and r.shape[2] == 3 and r.shape[0] == self.master.shape[0]
        self.sh_master = r.astype(F)
        self.sh_m = np.zeros_like(self.sh_master)
        self.sh_v = np.zeros_like(self.sh_master)

    def rest_halves(self, defect=None):
        return refit_ref.store16(self.sh_master, defect)


def step_sh(st, q_sh, q_o, colour_unit, opacity_unit, lr_sh=0.000125, lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999, eps=1e-15,
            opacity_min=0.0, trace=None, defect=None):
    """One ws_refit_step_sh of ShState st along q_sh (N, ncoef, 3) and q_o (N,), in place: refit_ref.step on the DC triple and the
    opacity, then the rest elements with g = (float)((double)q * colour_unit), the rate lr_sh and the clamp at +-65504, under the
    same powers."""
    q_sh, q_o = np.asarray(q_sh), np.asarray(q_o)
    assert q_sh.dtype == np.int64 and q_o.dtype == np.int64 and q_sh.shape[1:] == (st.sh_master.shape[1] + 1, 3)
    refit_ref.step(st, np.concatenate([q_sh[:, 0, :], q_o[:, None]], axis=1), colour_unit, opacity_unit, lr_colour=lr_colour,
                   lr_opacity=lr_opacity, beta1=beta1, beta2=beta2, eps=eps, opacity_min=opacity_min, trace=trace, defect=defect)
    lr_sh, beta1, beta2, eps = (F(z) for z in (lr_sh, beta1, beta2, eps))
    if lr_sh != 0 and st.sh_master.shape[1]:
        bc1, bc2 = F(1.0 - st.p1), F(1.0 - st.p2)   # (the powers refit_ref.step has just advanced)
        omb1, omb2 = F(1.0) - beta1, F(1.0) - beta2
        with np.errstate(all="ignore"):
            g = (q_sh[:, 1:, :].astype(np.float64) * float(colour_unit)).astype(F)
            x1, m1, v1 = refit_ref._adam(g, lr_sh, st.sh_master, st.sh_m, st.sh_v, beta1, beta2, omb1, omb2, bc1, bc2, eps, trace,
                                           defect)
        st.sh_master = refit_ref._clamp(x1, -SH_MAX, SH_MAX, defect)
        st.sh_m, st.sh_v = m1, v1
    return st
