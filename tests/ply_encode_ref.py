"""The PLY row encode (k_ply_encode of ply_encode.hip and its host twin ws_ply_rows_encode; include/websplat.h "Saving a point
cloud") restated in float64 numpy, the bound a saved and reloaded covariance obeys, and the clouds the tests put in front of it.
Plain numpy, no GPU.

encode_ref      the float64 definition with numpy.linalg.eigh for the eigen-decomposition.  Its eigenvectors may differ from the
                Jacobi's (sign, and any basis of a repeated eigenvalue), so the rotation is never compared row against row; the
                log-scales and logits are.
cov_bound       |C' - C| <= sum |l_neg| + ulp16(max(|C|, |C'|)) per element: writing a negative eigenvalue as a zero extent moves
                an element by at most sum |l_neg| (the clamped matrix differs by sum |l_neg| v v^T, |v_i v_j| <= 1); the
                re-rounding to f16 and the f32 decode arithmetic move it by under one f16 ulp.  Derived, not fitted.  (The f32
                decode's error is of the size of l_max 2^-24, so an element far below l_max 2^-12 can exceed the bound whatever the
                encoder writes -- DESIGN.md 3.4l; the clouds below have no such element under the library's encoder.)
psd_margin      l_min > 2^-10 l_max in float64: the rows whose six halves are expected back identical.
CLOUDS / blobs  the four clouds of 20 000 rows the bound was checked on, as resident blobs (ply_rows.decode_ref of their rows),
                and `edges`: hostile opacities, covariances, SH halves and positions, built as blobs directly.
round_trip      the four checks of a blob -> rows -> blob round trip, shared by the CPU and the GPU test.
"""
import functools

import numpy as np

import ply_rows

F = np.float32
FLOOR, CEIL, HALF_MAX = -20.0, 20.0, 65504.0
N_CLOUD = 20_000
CLOUDS = ("ordinary", "aniso", "flat", "opacity_wide")
MISMATCH_CAP = 1e-3        # share of psd_margin rows whose six halves may differ; float64 measured at most 2.5e-4


# ---- the blobs ----------------------------------------------------------------------------------------------------------------------
def split(g, s):
    """(positions N x 3 f32, opacity halves N uint16, covariance halves N x 6 uint16, SH halves N x 48 uint16)"""
    g = np.ascontiguousarray(g, dtype=np.uint8).reshape(-1, 28)
    n = g.shape[0]
    pos = np.ascontiguousarray(g[:, 0:12]).view(F).reshape(n, 3)
    op = np.ascontiguousarray(g[:, 12:14]).view(np.uint16).reshape(n)
    cov = np.ascontiguousarray(g[:, 16:28]).view(np.uint16).reshape(n, 6)
    sh = np.ascontiguousarray(s, dtype=np.uint8).reshape(n, 96).view(np.uint16).reshape(n, 48)
    return pos, op, cov, sh


def join(pos, op, cov, sh):
    n = len(op)
    g = np.zeros((n, 28), np.uint8)
    g[:, 0:12] = np.ascontiguousarray(pos, dtype=F).view(np.uint8).reshape(n, 12)
    g[:, 12:14] = np.ascontiguousarray(op, dtype=np.uint16).view(np.uint8).reshape(n, 2)
    g[:, 16:28] = np.ascontiguousarray(cov, dtype=np.uint16).view(np.uint8).reshape(n, 12)
    s = np.ascontiguousarray(sh, dtype=np.uint16).view(np.uint8).reshape(n, 96).copy()
    return g, s


def h2d(h):
    """binary16 bit patterns as float64"""
    return np.ascontiguousarray(h, dtype=np.uint16).view(np.float16).astype(np.float64)


def sym(c6):
    """N x 6 (c00 c01 c02 c11 c12 c22) as N x 3 x 3"""
    c6 = np.asarray(c6, np.float64)
    m = np.empty(c6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        m[..., i, j] = m[..., j, i] = c6[..., k]
    return m


def finite_cov(cov_halves):
    return ((np.asarray(cov_halves) & 0x7C00) != 0x7C00).all(axis=-1)


def eigenvalues(cov_halves):
    """float64 eigenvalues, descending, of the rows with finite halves (NaN rows elsewhere)"""
    c = h2d(cov_halves)
    ok = finite_cov(cov_halves)
    lam = np.full((c.shape[0], 3), np.nan)
    if ok.any():
        lam[ok] = np.linalg.eigvalsh(sym(c[ok]))[:, ::-1]
    return lam


def psd_margin(cov_halves):
    lam = eigenvalues(cov_halves)
    with np.errstate(invalid="ignore"):
        return lam[:, 2] > 2.0 ** -10 * lam[:, 0]


def separated(cov_halves):
    """psd_margin and pairwise eigenvalue gaps above 2^-10 l_max: there the Jacobi's eigenvalues and eigh's agree far inside an f32 ulp
    of their logarithms"""
    lam = eigenvalues(cov_halves)
    with np.errstate(invalid="ignore"):
        gap = 2.0 ** -10 * lam[:, 0]
        return psd_margin(cov_halves) & (lam[:, 0] - lam[:, 1] > gap) & (lam[:, 1] - lam[:, 2] > gap)


def ulp16(x):
    """the spacing of binary16 at magnitude x (2^-24 below the smallest normal); inf at and above 65520, where f16 has no finite neighbour"""
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return np.where(x >= 65520.0, np.inf, 2.0 ** (e - 10))


def cov_bound(cov_halves, cov_halves_2):
    """(|C' - C|, bound) per element, N x 6, for rows with finite C; rows with a half that is not finite get (0, 0)"""
    c, c2 = h2d(cov_halves), h2d(cov_halves_2)
    ok = finite_cov(cov_halves)
    lam = eigenvalues(cov_halves)
    neg = np.where(ok[:, None], np.where(lam < 0, -lam, 0.0), 0.0).sum(axis=1)
    with np.errstate(invalid="ignore"):
        diff = np.where(ok[:, None], np.abs(c2 - c), 0.0)
        bound = np.where(ok[:, None], neg[:, None] + ulp16(np.maximum(np.abs(c), np.abs(c2))), 0.0)
    return diff, bound


# ---- the float64 definition ---------------------------------------------------------------------------------------------------------
def _shepperd(r):
    """N x 3 x 3 proper rotations -> unit quaternions (scalar first, scalar part >= 0), float64"""
    r00, r11, r22 = r[:, 0, 0], r[:, 1, 1], r[:, 2, 2]
    tr = r00 + r11 + r22
    cand = np.stack([
        np.stack([1 + tr, r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], 1),
        np.stack([r[:, 2, 1] - r[:, 1, 2], 1 + r00 - r11 - r22, r[:, 0, 1] + r[:, 1, 0], r[:, 0, 2] + r[:, 2, 0]], 1),
        np.stack([r[:, 0, 2] - r[:, 2, 0], r[:, 0, 1] + r[:, 1, 0], 1 - r00 + r11 - r22, r[:, 1, 2] + r[:, 2, 1]], 1),
        np.stack([r[:, 1, 0] - r[:, 0, 1], r[:, 0, 2] + r[:, 2, 0], r[:, 1, 2] + r[:, 2, 1], 1 - r00 - r11 + r22], 1)], 1)
    pick = np.argmax(np.stack([tr, r00, r11, r22], 1), axis=1)
    q = cand[np.arange(len(pick)), pick]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1
    q[:, 0] += 0.0
    return q


def log_scale(lam):
    lam = np.asarray(lam, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lam > 0, 0.5 * np.log(np.where(lam > 0, lam, 1.0)), FLOOR)


def logit(op_halves):
    o = h2d(op_halves)
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.log(o / (1 - o))
    return np.where(np.isnan(o), np.nan, np.where(o <= 0, FLOOR, np.where(o >= 1, CEIL, mid)))


def nonfinite_extents(cov_halves):
    """the stated extents of a covariance with a half that is not finite: the diagonal, +inf as 65504, NaN and -inf (and negatives) as 0"""
    d = h2d(np.asarray(cov_halves)[:, [0, 3, 5]])
    return np.where(np.isnan(d), 0.0, np.clip(d, 0.0, HALF_MAX))


def encode_ref(gaussians, sh, sh_deg):
    """N x (14 + 3 (sh_deg + 1)^2) float32 rows: the definition of websplat.h "Saving a point cloud" in float64, eigh for the Jacobi"""
    pos, op, cov, shh = split(gaussians, sh)
    n, nc = len(op), (sh_deg + 1) ** 2
    rows = np.zeros((n, ply_rows.row_len(sh_deg)), F)
    t = ply_rows.tail_col(sh_deg)
    rows[:, 0:3] = pos
    sh32 = shh.view(np.float16).astype(F).reshape(n, 16, 3)
    rows[:, 6:9] = sh32[:, 0]
    if nc > 1:
        rows[:, 9:t] = sh32[:, 1:nc].transpose(0, 2, 1).reshape(n, 3 * (nc - 1))
    rows[:, t] = logit(op).astype(F)
    ok = finite_cov(cov)
    lam = np.zeros((n, 3))
    q = np.zeros((n, 4))
    q[:, 0] = 1.0
    lam[~ok] = nonfinite_extents(cov[~ok])
    if ok.any():
        w, v = np.linalg.eigh(sym(h2d(cov[ok])))
        w, v = w[:, ::-1], v[:, :, ::-1].copy()              # (descending; the library does not sort: compare as sorted triples)
        v[:, :, 2] *= np.sign(np.linalg.det(v))[:, None]
        lam[ok], q[ok] = w, _shepperd(v)
    rows[:, t + 1:t + 4] = log_scale(lam).astype(F)
    rows[:, t + 4:t + 8] = q.astype(F)
    return rows


# ---- the clouds ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud_rows(name, sh_deg, n=N_CLOUD):
    """the source rows of a named cloud: ply_rows.ordinary(n, sh_deg, 1) with the tail columns of its name redrawn from
    default_rng(1) -- seed 1 is the one seed the clouds are defined with"""
    rows = ply_rows.ordinary(n, sh_deg, 1)
    t = ply_rows.tail_col(sh_deg)
    rng = np.random.default_rng(1)
    if name == "aniso":
        rows[:, t + 1:t + 4] = rng.uniform(-9, 1, (n, 3))
        rows[:, t + 4:t + 8] = rng.standard_normal((n, 4))
    elif name == "flat":
        rows[:, t + 1:t + 3] = rng.uniform(-3, 0, (n, 2))
        rows[:, t + 3] = -12.0
    elif name == "opacity_wide":
        rows[:, t] = rng.uniform(-18, 18, n)
        rows[:, t + 1:t + 4] = rng.uniform(-3, 0, (n, 3))
    elif name != "ordinary":
        raise KeyError(name)
    rows.setflags(write=False)
    return rows


OPACITY_HALVES = (0x0000, 0x8000, 0x3C00, 0x0001, 0x3BFF, 0x3E00, 0x7BFF, 0x7E00, 0xFE00, 0x3800, 0xB800)
_H = lambda *v: tuple(int(np.float16(x).view(np.uint16)) for x in v)  # noqa: E731
INF16, NAN16 = 0x7C00, 0x7E00
COVARIANCES = (
    _H(0, 0, 0, 0, 0, 0),                        # zero
    _H(0.25, 0, 0, 0.25, 0, 0.25),               # isotropic: a triple eigenvalue
    _H(1, 0, 0, 1, 0, 0.0625),                   # doubly degenerate, diagonal
    _H(0.5, 0.25, 0.25, 0.5, 0.25, 0.5),         # doubly degenerate, not diagonal: eigenvalues 1, 0.25, 0.25
    _H(1, 0, 0, -0.5, 0, 0.25),                  # diagonal with a negative entry
    _H(0, 1, 0, 0, 0, 0),                        # zero diagonal, indefinite: eigenvalues 1, 0, -1
    _H(2, 0.5, -0.25, 1, 0.125, 0.5),            # generic, definite
    _H(HALF_MAX, 0, 0, HALF_MAX, 0, HALF_MAX),   # the largest finite half on the diagonal
    _H(HALF_MAX, 0, 0, 2.0 ** -24, 0, 1),        # the largest and the smallest half together
    (INF16, 0, 0, 0x3C00, 0, 0x3800),            # +inf on the diagonal
    (0x3C00, 0xFC00, 0, 0x3C00, 0, 0x3C00),      # -inf off the diagonal
    (0x3C00, 0, 0, 0xFC00, 0, 0x3C00),           # -inf on the diagonal
    (0x3C00, 0, 0, 0x3C00, NAN16, 0x3C00),       # a NaN half off the diagonal
    (NAN16, 0, 0, 0xB800, 0, 0x3400),            # a NaN half and a negative one on the diagonal
)
N_FINITE_COV = 9


@functools.lru_cache(maxsize=None)
def edges():
    """(gaussians, sh) of the edge cloud: every covariance beside every opacity half; row i holds SH_HALVES[(i + slot) % len] in
    SH slot `slot` and POSITIONS[(i + axis) % len] in axis `axis`.  The same blobs serve every SH degree."""
    pairs = [(o, c) for c in COVARIANCES for o in OPACITY_HALVES]
    n = len(pairs)
    op = np.array([p[0] for p in pairs], np.uint16)
    cov = np.array([p[1] for p in pairs], np.uint16)
    shv = np.array([NAN16 if h is None else h for h in ply_rows.SH_HALVES], np.uint16)
    sh = shv[(np.arange(n)[:, None] + np.arange(48)[None, :]) % len(shv)]
    posv = np.array(ply_rows.POSITIONS, F)
    pos = posv[(np.arange(n)[:, None] + np.arange(3)[None, :]) % len(posv)]
    g, s = join(pos, op, cov, sh)
    g.setflags(write=False)
    s.setflags(write=False)
    return g, s


@functools.lru_cache(maxsize=None)
def blobs(name, sh_deg, n=N_CLOUD):
    """(gaussians N x 28, sh N x 96) of a named cloud as it is resident: decode_ref of its rows; `edges` as built (SH coefficients
    above the degree zeroed, as every loader leaves them)"""
    if name == "edges":
        g, s = edges()
        s = s.copy()
        s[:, 6 * (sh_deg + 1) ** 2:] = 0
    else:
        g, s = ply_rows.decode_ref(cloud_rows(name, sh_deg, n), sh_deg, "f64")
    g.setflags(write=False)
    s.setflags(write=False)
    return g, s


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def round_trip(g0, s0, g1, s1, label=""):
    """The four checks of blobs -> rows -> blobs.  Prints every figure before it asserts."""
    pos0, op0, cov0, sh0 = split(g0, s0)
    pos1, op1, cov1, sh1 = split(g1, s1)
    same_pos = np.array_equal(pos0.view(np.uint32), pos1.view(np.uint32)) and np.array_equal(np.asarray(g0)[:, 14:16], np.asarray(g1)[:, 14:16])
    bad_sh = int((~ply_rows.same_halves(sh0, sh1)).sum())
    # opacity: exact, NaN as a class, a half above 1 comes back as 1
    want_op = np.where((h2d(op0) > 1.0), np.uint16(0x3C00), op0).astype(np.uint16)
    want_op = np.where(op0 == 0x8000, np.uint16(0), want_op).astype(np.uint16)     # -0 is written as logit -20, whose sigmoid rounds to +0
    neg = (h2d(op0) < 0)                                                           # (a negative opacity is no opacity: written as 0)
    want_op = np.where(neg, np.uint16(0), want_op).astype(np.uint16)
    bad_op = int((~ply_rows.same_halves(want_op, op1)).sum())
    diff, bound = cov_bound(cov0, cov1)
    with np.errstate(invalid="ignore"):
        over = diff > bound
    margin = psd_margin(cov0)
    zero_sign = (cov0 | 0x8000) == (cov1 | 0x8000)
    equal = ((cov0 == cov1) | (zero_sign & ((cov0 & 0x7FFF) == 0))).all(axis=1)
    mism = int((margin & ~equal).sum())
    share = mism / max(1, int(margin.sum()))
    print(f"{label}: rows {len(op0)}, positions equal {same_pos}, SH halves differing {bad_sh}, opacity halves differing {bad_op}, "
          f"covariance elements over the bound {int(over.sum())} (largest |C'-C|/bound {np.nanmax(np.where(bound > 0, diff / np.where(bound > 0, bound, 1), 0)):.3f}), "
          f"psd_margin rows {int(margin.sum())}, of them not identical {mism} (share {share:.2e}, cap {MISMATCH_CAP:.0e})")
    assert same_pos and bad_sh == 0
    assert bad_op == 0
    assert not over.any()
    assert share <= MISMATCH_CAP
    return dict(margin_rows=int(margin.sum()), mismatches=mism, equal=equal)


def tail_is_sound(rows, g0, s0, sh_deg):
    """quaternion norm within 2^-22 of 1, rot_0 >= 0, its rotation proper, every value finite unless its input half was NaN,
    normals +0"""
    rows = np.ascontiguousarray(rows, dtype=F)
    _, op, _, sh = split(g0, s0)
    t = ply_rows.tail_col(sh_deg)
    q = rows[:, t + 4:t + 8].astype(np.float64)
    norm = np.linalg.norm(q, axis=1)
    assert np.abs(norm - 1).max() <= 2.0 ** -22, np.abs(norm - 1).max()
    assert (rows[:, t + 4] >= 0).all() and not np.signbit(rows[:, t + 4]).any()
    s_, x, y, z = q.T
    r = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s_ * z), 2 * (x * z + s_ * y)], 1),
                  np.stack([2 * (x * y + s_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s_ * x)], 1),
                  np.stack([2 * (x * z - s_ * y), 2 * (y * z + s_ * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    assert (np.linalg.det(r) > 0).all()
    assert np.array_equal(rows[:, 3:6].view(np.uint32), np.zeros((rows.shape[0], 3), np.uint32))
    nan_in = np.zeros(rows.shape, bool)
    nan_in[:, t] = ply_rows.is_nan_half(op)
    nc = (sh_deg + 1) ** 2
    for c in range(nc):
        for j in range(3):
            col = 6 + j if c == 0 else 9 + j * (nc - 1) + (c - 1)
            nan_in[:, col] = ply_rows.is_nan_half(sh[:, 3 * c + j])
    inf_in = np.zeros(rows.shape, bool)                   # an infinite SH half stays infinite: it is widened, not computed
    for c in range(nc):
        for j in range(3):
            col = 6 + j if c == 0 else 9 + j * (nc - 1) + (c - 1)
            inf_in[:, col] = (sh[:, 3 * c + j] & 0x7FFF) == 0x7C00
    assert np.array_equal(np.isnan(rows), nan_in)
    assert np.array_equal(np.isinf(rows), inf_in)


def ulps_f32(a, b):
    """|a - b| in units of the f32 spacing at the larger magnitude (0 where both are equal, NaN pairs included)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F)).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp
    return np.where(same, 0.0, d)
