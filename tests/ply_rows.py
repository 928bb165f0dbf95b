"""The PLY row decode (k_ply_decode of ply_decode.hip, its host twin ws_ply_rows_convert and the oracle's
wso_ply_rows_convert) restated in numpy, and the small clouds that put one edge each in front of it.  Plain numpy, no GPU;
tests/test_ply_rows.py pins this module against the oracle and the host twin, tests/test_gpu_ply_edges.py pins the kernel to it.

decode_ref      every operation a separately rounded f32 numpy operation in the order of the three implementations; exp either
                as the kernel takes it ("f64": an f64 exp rounded once to f32) or as the host twin and the oracle take it ("libm":
                the C library's expf).  The covariance is build_cov of oracle/ws_oracle_io.py.
same_halves     bit equality of f16 halves, NaN compared as a class: no implementation defines a NaN's sign or payload.
undecided       the rows with an exp argument whose f64 result lies within two f64 ulps of an f32 rounding boundary: only there may
                two f64 exp implementations that differ in the last bit give different f32 values.
CLOUDS / cloud  the named edge clouds, each for every SH degree: rows of 14 + 3 (deg + 1)^2 floats
                x y z | nx ny nz | f_dc[3] | f_rest[3][C-1] | opacity | scale[3] | rot[4], normals NaN (the decode ignores them),
                positions finite.
"""
import ctypes
import ctypes.util
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ws_oracle_io as oio  # noqa: E402

F = np.float32
INF, NAN = np.inf, np.nan

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def row_len(sh_deg):
    return 14 + 3 * (sh_deg + 1) ** 2


def tail_col(sh_deg):
    """column of the opacity logit: the eight tail floats are opacity | scale[3] | rot[4]"""
    return row_len(sh_deg) - 8


def exp_f64(x):
    """what k_ply_decode does: (float)exp((double)x)"""
    with np.errstate(all="ignore"):
        return np.exp(x.astype(np.float64)).astype(F)


def exp_libm(x):
    """what the host twin and the oracle do: the C library's expf, one call per element"""
    x = np.ascontiguousarray(x, dtype=F)
    return np.array([_libm.expf(float(v)) for v in x.ravel()], dtype=F).reshape(x.shape)


def _defective_inverse(q, defect):
    """1 / magnitude of the quaternion normalisation gone wrong; `defect` ("flush", "fused" or "approx_rcp") restates one way a build can go wrong, for
    tests/test_ply_rows.py to show that the clouds tell it from the real thing: f32 subnormals flushed to zero, the sum of
    squares contracted into fused multiply-adds, a reciprocal one ulp off"""
    sq = q * q
    if defect == "flush":
        sq = np.where(np.abs(sq) < np.finfo(F).tiny, F(0) * sq, sq)
    mag2 = sq[:, 0] + (sq[:, 1] + sq[:, 2] + sq[:, 3])
    if defect == "fused":
        d = q.astype(np.float64)
        acc = sq[:, 3].astype(np.float64)
        for k in (2, 1):
            acc = (d[:, k] * d[:, k] + acc).astype(F).astype(np.float64)
        mag2 = (d[:, 0] * d[:, 0] + acc).astype(F)
    inv = F(1) / np.sqrt(mag2)
    if defect == "approx_rcp":
        inv = np.nextafter(inv, F(np.inf))
    return inv


def _parts(rows, sh_deg, exp, defect=None):
    ex = {"f64": exp_f64, "libm": exp_libm}[exp]
    rows = np.ascontiguousarray(rows, dtype=F)
    n, nc = rows.shape[0], (sh_deg + 1) ** 2
    assert rows.shape[1] == row_len(sh_deg)
    tail = rows[:, tail_col(sh_deg):]
    x = tail[:, 0]
    with np.errstate(all="ignore"):
        # utils.rs sigmoid, two branches on x >= 0 (NaN takes the second)
        pos = F(1) / (F(1) + ex(-x))
        e = ex(x)
        neg = e / (F(1) + e)
        opacity = np.where(x >= 0, pos, neg).astype(F)
        scale = ex(tail[:, 1:4])
        q = tail[:, 4:8]
        if defect is None:
            mag = np.sqrt(q[:, 0] * q[:, 0] + (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
            q = q * (F(1) / mag)[:, None]
        else:
            q = q * _defective_inverse(q, defect)[:, None]
        cov = oio.build_cov(q, scale)
        sh = np.zeros((n, 16, 3), F)                     # coefficient-major; zero above the degree
        sh[:, 0] = rows[:, 6:9]
        if nc > 1:                                       # f_rest is channel-major [3][C-1]
            sh[:, 1:nc] = rows[:, 9:9 + 3 * (nc - 1)].reshape(n, 3, nc - 1).transpose(0, 2, 1)
        return opacity.astype(np.float16), cov.astype(np.float16), sh.astype(np.float16)


def decode_ref(rows, sh_deg, exp="f64", defect=None):
    """(gaussians N x 28 uint8, sh N x 96 uint8) in the layout ws_pointcloud_download returns:
    x y z f32 | opacity f16 | 2 B zero | cov f16 x 6, and [[f16; 3]; 16].  `defect`: see _defective_inverse (never the reference)."""
    rows = np.ascontiguousarray(rows, dtype=F)
    n = rows.shape[0]
    opacity, cov, sh = _parts(rows, sh_deg, exp, defect)
    g = np.zeros((n, 28), np.uint8)
    g[:, 0:12] = np.ascontiguousarray(rows[:, 0:3]).view(np.uint8).reshape(n, 12)
    g[:, 12:14] = np.ascontiguousarray(opacity).view(np.uint8).reshape(n, 2)
    g[:, 16:28] = np.ascontiguousarray(cov).view(np.uint8).reshape(n, 12)
    s = np.ascontiguousarray(sh).view(np.uint8).reshape(n, 96).copy()
    return g, s


def halves(a):
    """any array of f16 / uint8 / uint16 as its binary16 bit patterns"""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint16 else a.view(np.uint16)


def is_nan_half(h):
    return (halves(h) & 0x7FFF) > 0x7C00


def same_halves(a, b):
    a, b = halves(a), halves(b)
    return (a == b) | (is_nan_half(a) & is_nan_half(b))


def computed_halves(g):
    """N x 7 uint16: the opacity and the six covariance halves of N x 28 Gaussian records"""
    n = g.shape[0]
    return np.ascontiguousarray(g[:, 12:28]).view(np.uint16).reshape(n, 8)[:, [0, 2, 3, 4, 5, 6, 7]]


def exp_arguments(rows, sh_deg):
    """N x 4: the arguments the decode hands to exp -- the sigmoid's (x or -x by its branch) and the three log-scales"""
    tail = np.ascontiguousarray(rows, dtype=F)[:, tail_col(sh_deg):]
    x = tail[:, 0]
    return np.concatenate([np.where(x >= 0, -x, x)[:, None], tail[:, 1:4]], axis=1).astype(F)


def undecided(rows, sh_deg):
    """bool per row: some exp argument's f64 result, moved two f64 ulps either way, rounds to two different f32 values"""
    with np.errstate(all="ignore"):
        y = np.exp(exp_arguments(rows, sh_deg).astype(np.float64))
        lo = hi = y
        for _ in range(2):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        decided = (lo.astype(F) == hi.astype(F)) | np.isnan(y)
    return ~decided.all(axis=1)


# ---- the clouds -------------------------------------------------------------------------------------------------------------------
BLOCK_NS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385)      # k_ply_decode: 128 rows per block
GENERIC_Q = (0.5, -0.3, 0.7, 0.2)

OPACITY_SUBNORMAL = (-9.71, -12.0, -14.5, -16.6)                     # sigmoid in (2^-24, 2^-14): an f16 subnormal
OPACITY_LOGITS = (0.0, -0.0, -9.70, *OPACITY_SUBNORMAL, -16.64, -17.33, -17.4, 9.70, 16.64, 17.33, 30.0, -30.0, 87.3, -87.3,
                  88.8, -88.8, -103.97, -104.0, 745.0, -745.0, INF, -INF, NAN)
LOG_SCALES = (-INF, -104.0, -20.0, -12.5, -8.664, -8.5, -4.85, 0.0, 5.5449, 5.55, 44.4, 88.8, INF, NAN)
QUATERNIONS = (
    (1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1),
    GENERIC_Q, tuple(-v for v in GENERIC_Q), tuple(v * 1e-3 for v in GENERIC_Q), tuple(v * 1e3 for v in GENERIC_Q),
    (1e-20, 0, 0, 0), (0, 0, 1e-20, 0), (1e-20, 1e-20, 1e-20, 1e-20), (1e-20, -1e-20, 2e-20, 1e-20),   # squares: f32 subnormals
    (1e-23, 0, 0, 0), (1e-23, 1e-23, 1e-23, 1e-23),                  # squares 0, magnitude 0, NaN through 0 * inf
    (1e19, 1e19, 1e19, 1e19), (1e20, 0, 0, 0), (-1e20, 1e20, 0, 1e20),   # magnitude inf, inverse 0, R = I
    (0, 0, 0, 0), (NAN, 0, 0, 0), (0.5, NAN, 0.5, 0.5), (1, 0, 0, NAN))
Q_SUBNORMAL_SQUARES = (12, 13, 14, 15)
Q_OVERFLOW = (18, 19, 20)
QUATERNION_LOG_SCALES = (-1.0, -2.5, 0.5)
SH_VALUES = (65504.0, 65519.99, 65520.0, 1e5, INF, -INF, NAN, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -14,
             1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -0.0, 1e-40, -65504.0, -65519.99, -65520.0, -1e5, -(2.0 ** -24), -(2.0 ** -25),
             -(2.0 ** -25) * (1 + 2.0 ** -23), -(2.0 ** -14), -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11), -1e-40)
# what SH_VALUES[k] becomes in f16 (round to nearest, ties to even); None: NaN
SH_HALVES = (0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0x7C00, 0xFC00, None, 0x0001, 0x0000, 0x0001, 0x0400, 0x3C00, 0x3C02, 0x8000, 0x0000,
             0xFBFF, 0xFBFF, 0xFC00, 0xFC00, 0x8001, 0x8000, 0x8001, 0x8400, 0xBC00, 0xBC02, 0x8000)
SH_TIES = (2, 8, 11, 12, 17, 20, 23, 24)                             # exact ties in f32, landing on the even neighbour
POSITIONS = (-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 3e38, -3e38, 1.0, -2.5)
MIXED_TAIL = (0, -0.0, 1e-30, -1e-30, 9.7, -9.7, -16.6, -16.64, -17.33, 30, -30, 87.3, -87.3, 88.8, -88.8, -103.97, -104, 745,
              -745, INF, -INF, NAN, -20, -12.5, -8.5, -8.664, -4.85, 5.5449, 5.55, 44.4, 1e-20, 1e-23, 1e19, 1e20, 1e-45)
MIXED_N, MIXED_SEED = 3000, 1
BULK_N = 50_001

CLOUDS = tuple(f"block_{n}" for n in BLOCK_NS) + ("opacity", "scales_identity", "scales_generic", "quaternions", "sh_values",
                                                   "positions", "mixed")


def ordinary(n, sh_deg, seed):
    """n plain rows: a cube of small Gaussians with NaN normals"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, row_len(sh_deg)), F)
    t = tail_col(sh_deg)
    rows[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    rows[:, 3:6] = NAN
    rows[:, 6:9] = rng.uniform(-1.5, 1.5, (n, 3))
    rows[:, 9:t] = rng.standard_normal((n, t - 9)) * 0.1
    rows[:, t] = rng.uniform(-2, 4, n)
    rows[:, t + 1:t + 4] = rng.uniform(np.log(0.005), np.log(0.05), (n, 3))
    rows[:, t + 4:t + 8] = rng.standard_normal((n, 4))
    return rows


def slot_code(row, coef, channel):
    """the f16 bit pattern that names (row, coefficient, channel): a distinct positive normal half for rows < 568"""
    return 0x0400 + row * 48 + coef * 3 + channel


def _block(n, sh_deg):
    rows = ordinary(n, sh_deg, 100 + n)
    nc = (sh_deg + 1) ** 2
    i = np.arange(n)
    rows[:, 0], rows[:, 1], rows[:, 2] = i, -i, i + 0.5
    for c in range(nc):
        for j in range(3):
            col = 6 + j if c == 0 else 9 + j * (nc - 1) + (c - 1)
            rows[:, col] = slot_code(i, c, j).astype(np.uint16).view(np.float16).astype(F)
    return rows


def _scales(sh_deg, q):
    """every log-scale in all three axes, then in one axis at a time beside scales of 1"""
    per = []
    for v in LOG_SCALES:
        per.append((v, v, v))
        per += [tuple(v if k == a else 0.0 for k in range(3)) for a in range(3)]
    rows = ordinary(len(per), sh_deg, 7)
    t = tail_col(sh_deg)
    rows[:, t + 1:t + 4] = np.array(per, F)
    rows[:, t + 4:t + 8] = np.array(q, F)
    return rows


def _mixed(sh_deg):
    """random draws from the hostile list in the eight tail floats of two rows in three, hostile SH values in every slot of one
    row in six, among ordinary rows"""
    rng = np.random.default_rng(MIXED_SEED)
    rows = ordinary(MIXED_N, sh_deg, MIXED_SEED + 1)
    t = tail_col(sh_deg)
    vals = np.array(MIXED_TAIL, F)
    for i in range(0, MIXED_N * 2 // 3):
        k = rng.integers(1, 9)
        cols = t + rng.choice(8, k, replace=False)
        rows[i, cols] = rng.choice(vals, k) * rng.choice(np.array([1, -1, 1], F), k)
    first = MIXED_N * 2 // 3
    count = MIXED_N // 6
    rows[first:first + count, 6:t] = rng.choice(np.array(SH_VALUES, F), (count, t - 6))
    return rows


@functools.lru_cache(maxsize=None)
def cloud(name, sh_deg):
    """the named cloud's rows (read-only, shared between tests)"""
    t = tail_col(sh_deg)
    if name.startswith("block_"):
        rows = _block(int(name[6:]), sh_deg)
    elif name == "opacity":
        rows = ordinary(len(OPACITY_LOGITS), sh_deg, 3)
        rows[:, t] = np.array(OPACITY_LOGITS, F)
    elif name == "scales_identity":
        rows = _scales(sh_deg, (1, 0, 0, 0))
    elif name == "scales_generic":
        rows = _scales(sh_deg, GENERIC_Q)
    elif name == "quaternions":
        rows = ordinary(len(QUATERNIONS), sh_deg, 4)
        rows[:, t + 1:t + 4] = np.array(QUATERNION_LOG_SCALES, F)
        rows[:, t + 4:t + 8] = np.array(QUATERNIONS, F)
    elif name == "sh_values":                            # row i, slot s holds SH_VALUES[(i + s) % len]: every value in every slot
        k = len(SH_VALUES)
        rows = ordinary(k, sh_deg, 5)
        rows[:, 6:t] = np.array(SH_VALUES, F)[(np.arange(k)[:, None] + np.arange(t - 6)[None, :]) % k]
    elif name == "positions":                            # row i holds POSITIONS[i + a] in axis a
        k = len(POSITIONS)
        rows = ordinary(k, sh_deg, 6)
        rows[:, 0:3] = np.array(POSITIONS, F)[(np.arange(k)[:, None] + np.arange(3)[None, :]) % k]
    elif name == "mixed":
        rows = _mixed(sh_deg)
    else:
        raise KeyError(name)
    assert np.isnan(rows[:, 3:6]).all() and np.isfinite(rows[:, 0:3]).all()
    rows.setflags(write=False)
    return rows


def sh_slot_of_column(col, sh_deg):
    """(coefficient, channel) of row column col in 6 .. tail_col"""
    nc = (sh_deg + 1) ** 2
    if col < 9:
        return 0, col - 6
    j, c = divmod(col - 9, nc - 1)
    return c + 1, j


@functools.lru_cache(maxsize=None)
def bulk_rows(sh_deg):
    """the 50 001-row scene of tests/test_gpu_ply_decode.py: synth.scene_c1 with wide logits, wide log-scales and tiny quaternions
    in its first rows"""
    from websplat import synth
    rows = synth.scene_c1(n=BULK_N, seed=70 + sh_deg, sh_deg=sh_deg)
    rng = np.random.default_rng(5)
    t = tail_col(sh_deg)
    rows[:200, t] = rng.uniform(-30, 30, 200)           # opacity logits far out on both sigmoid branches
    rows[200:400, t + 1:t + 4] = rng.uniform(-14, 3, (200, 3))   # log-scales from 1e-6 to 20
    rows[400:410, t + 4:t + 8] *= 1e-3                  # tiny (still normalisable) quaternions
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def reference(name, sh_deg, exp="f64"):
    """decode_ref of a named cloud ("bulk": bulk_rows), computed once"""
    rows = bulk_rows(sh_deg) if name == "bulk" else cloud(name, sh_deg)
    g, s = decode_ref(rows, sh_deg, exp)
    g.setflags(write=False)
    s.setflags(write=False)
    return g, s


def compare(g, s, g0, s0):
    """The comparison of the tests: positions, padding byte for byte; every half under same_halves.  Returns
    (number of differing computed halves [opacity + covariance], number of differing SH halves, positions and padding equal)."""
    n = g.shape[0]
    fixed = np.array_equal(g[:, :12], g0[:, :12]) and np.array_equal(g[:, 14:16], g0[:, 14:16])
    bad = ~same_halves(computed_halves(g), computed_halves(g0))
    bad_sh = ~same_halves(np.ascontiguousarray(s).view(np.uint16).reshape(n, 48), np.ascontiguousarray(s0).view(np.uint16).reshape(n, 48))
    return bad, bad_sh, fixed
