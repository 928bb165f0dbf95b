"""k_blend_strict (csrc/raster.hip: the blend of WS_BLEND_TARGET_PRECISION) restated in numpy, with an interval for the one
operation numpy cannot reproduce, and the frames that put the kernel's launch geometry in front of it.  Plain numpy, no GPU;
tests/test_strict_ref.py pins this module against the oracle (oracle/ws_oracle.c wso_render) and shows which wrong blends it
tells from the right one, tests/test_gpu_blend_strict.py holds the kernel to it.

The kernel and its decode_splat are compiled with contraction off, and division and square root are correctly rounded, so every
operation of a (record, pixel) pair is an IEEE binary32 operation that numpy's float32 repeats bit for bit -- but one: expf.  The
HIP math API documents device expf with a maximum error of 1 ulp (HIP documentation, "HIP math API", single-precision
mathematical functions); the walk allows EXP_ULPS = 2, one more.

strict_walk     the walk of a frame, far to near, per record and pixel in the kernel's operation order:
                  m00 = v1x W, m01 = v2x W, m10 = -v1y H, m11 = -v2y H, det = (m00 m11) - (m01 m10), inv = 1 / det,
                  i00 = m11 inv, i01 = -m01 inv, i10 = -m10 inv, i11 = m00 inv, cx = ((x 0.5) + 0.5) W, cy = (0.5 - (y 0.5)) H;
                  dx = fx - cx, dy = fy - cy, p0 = (i00 dx) + (i01 dy), p1 = (i10 dx) + (i11 dy), a = (p0 p0) + (p1 p1);
                  kept = a <= CUT_A (and z < D under an occluder); bb = min(0.99, exp(-a) alpha), om = 1 - bb;
                  d = q((c bb) + (d om)) per channel, c = 1 for alpha; q = the target's rounding (quantize).
                exp(-a) is taken in float64 and rounded once to f32: the CENTRE e.  The device's value is one of the 2 E + 1
                binary32 values e - E ulp .. e + E ulp.  The step is monotone in d for a fixed bb (om >= 0.01, every f32 rounding
                and q are monotone), so an interval (lo, hi) per pixel and channel is carried through d by its two ends.  In bb
                the EXACT step is monotone as well, but the rounded one is a rising term plus a falling one, (c bb) + (d om), and
                between the two ends of bb it can leave their images by an f32 ulp; so the step is evaluated at every one of
                the 2 E + 1 values of bb, not only at its ends: new lo = the least, new hi = the largest of
                {bb_-E .. bb_+E} x {lo, hi}.  (The four corners are among them: the interval is never narrower than theirs.)
                Returns lo, hi, the walk with e itself (centre), and per pixel whether some channel's interval is open
                (lo != hi) at the end, or was at any time (ever_open).
                A pair counts wherever it lies (gaussian.wgsl draws every fragment of the quad): the kernel's own quadrant test,
                the padded bounding box of decode_splat, is NOT restated, so a record the kernel fails to broadcast to a quadrant
                it reaches is an error.  Pairs are evaluated over a box that holds the kept ellipse with a pixel and one per cent
                to spare (|d.x| <= sqrt(CUT_A) |row_x(M)| where a <= CUT_A).
libm_walk       the same walk with the C library's expf, which is what the oracle calls: no interval, one image.
check           a device (or oracle) image against the interval: lo <= v <= hi on the decoded values, and equal stored words
                where lo == hi; counts for the report.
defect=         deliberately wrong walks (DEFECTS), for tests/test_strict_ref.py to show that `check` tells them apart.
FRAMES / frame  the named frames: rows and a viewport each, built once.
random_target, occluder_plane
                what the composite cases load and hide behind, shared by the CPU test (the cap on open pixels) and the device test.
"""
import ctypes
import ctypes.util
import hashlib

import numpy as np

import blend_ref as B
from websplat import synth

F = np.float32
CUTOFF = F(2.3539888583335364)   # ws_internal.h
CUT_A = F(2.0) * CUTOFF
CLAMP = F(0.99)
EXP_ULPS = 2
FORMATS = ("rgba16float", "rgba8unorm", "rgba32float")
ORACLE_MODE = {"rgba32float": 0, "rgba16float": 1, "rgba8unorm": 2}
MAX_OPEN = 0.01                  # the cap on the share of pixels whose interval is open at the end: a condition on the frames
DEFECTS = ("f16_rtz", "u8_trunc", "near_to_far", "round_once", "no_clamp", "tail_twice", "alpha_unrounded")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


# ---- the target's rounding ---------------------------------------------------------------------------------------------------
def _f16_toward_zero(v):
    h = v.astype(np.float16)
    with np.errstate(invalid="ignore"):
        past = np.abs(h.astype(F)) > np.abs(v)
    return np.where(past, np.nextafter(h, np.float16(0.0)), h).astype(F)


def quantize(v, fmt, defect=None):
    """quantize_target of raster.hip on f32 values: f16 round to nearest even; unorm8 rint(clamp(v, 0, 1) 255) / 255 (fmaxf and
    fminf: a NaN clamps to 0); f32 the identity."""
    if fmt == "rgba16float":
        with np.errstate(over="ignore"):
            return _f16_toward_zero(v) if defect == "f16_rtz" else v.astype(np.float16).astype(F)
    if fmt == "rgba8unorm":
        scaled = np.fmin(np.fmax(v, F(0.0)), F(1.0)) * F(255.0)
        return (np.floor(scaled) if defect == "u8_trunc" else np.rint(scaled)) / F(255.0)
    return v


def decode(fmt, image):
    """A stored image as the f32 values the kernel loads (load_pixel): unorm8 code / 255 in f32, f16 and f32 as they are."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image.astype(F) / F(255.0)
    return image.astype(F)


def words(fmt, values):
    """The words the kernel stores for f32 `values` already of the target's precision (store_pixel), as unsigned integers."""
    values = np.ascontiguousarray(values, dtype=F)
    if fmt == "rgba8unorm":
        return np.rint(np.fmin(np.fmax(values, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)
    if fmt == "rgba16float":
        with np.errstate(over="ignore"):
            return values.astype(np.float16).view(np.uint16)
    return values.view(np.uint32)


def _image_words(fmt, image):
    image = np.ascontiguousarray(image)
    if image.dtype == np.uint8:
        return image
    if image.dtype == np.float16:
        return image.view(np.uint16)
    return words(fmt, image)  # (an f32 image: the oracle's, or an rgba32float target)


def _ordered(w):
    """Stored float words as integers in the order of the values they encode (-0 and +0 one apart)."""
    bits = 8 * w.dtype.itemsize
    w = w.astype(np.int64)
    sign = np.int64(1) << (bits - 1)
    return np.where(w & sign, sign - 1 - (w & (sign - 1)), w | sign) - sign


def units_apart(fmt, wa, wb):
    """Distance between stored words in units of the target's last place."""
    if fmt == "rgba8unorm":
        return np.abs(wa.astype(np.int64) - wb.astype(np.int64))
    return np.abs(_ordered(wa) - _ordered(wb))


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def _exp_f64(x):
    return np.exp(x.astype(np.float64)).astype(F)


def _exp_libm(x):
    flat = np.ascontiguousarray(x, dtype=F).ravel()
    return np.array([_libm.expf(float(v)) for v in flat], dtype=F).reshape(x.shape)


def _decode_splats(frame, W, H):
    """decode_splat of raster.hip over every record of the frame at once (without its quadrant test)."""
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(F)
    v1x, v1y, v2x, v2y, pcx, pcy = (h[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        m00, m01 = v1x * W, v2x * W
        m10, m11 = (-v1y) * H, (-v2y) * H
        det = (m00 * m11) - (m01 * m10)
        inv = F(1.0) / det
        s = dict(i00=m11 * inv, i01=(-m01) * inv, i10=(-m10) * inv, i11=m00 * inv,
                 cx=((pcx * F(0.5)) + F(0.5)) * W, cy=(F(0.5) - (pcy * F(0.5))) * H)
        rad = np.sqrt(np.float64(CUT_A)) * 1.01
        s["ex"] = rad * np.hypot(m00.astype(np.float64), m01.astype(np.float64)) + 1.0
        s["ey"] = rad * np.hypot(m10.astype(np.float64), m11.astype(np.float64)) + 1.0
    s["colour"] = np.concatenate([h[:, 6:9], np.ones((len(h), 1), dtype=F)], axis=1)
    s["alpha"] = h[:, 9]
    return s


def _box(s, i, width, height):
    """Rows and columns that hold every kept pixel of record i, or None: a record with a NaN or infinite centre or extent keeps
    no pair (its a is NaN or infinite at every pixel)."""
    cx, cy, ex, ey = float(s["cx"][i]), float(s["cy"][i]), float(s["ex"][i]), float(s["ey"][i])
    if not all(np.isfinite(v) for v in (cx, cy, ex, ey)) or not all(np.isfinite(s[k][i]) for k in ("i00", "i01", "i10", "i11")):
        return None
    x0, x1 = max(int(np.floor(cx - ex)), 0), min(int(np.ceil(cx + ex)), width - 1)
    y0, y1 = max(int(np.floor(cy - ey)), 0), min(int(np.ceil(cy + ey)), height - 1)
    if x1 < x0 or y1 < y0:
        return None
    return slice(y0, y1 + 1), slice(x0, x1 + 1)


def _step(c, bb, d, fmt, defect, rounding):
    """d' = q((c bb) + (d om)); c [4], bb [..., 1], d [..., 4]"""
    om = F(1.0) - bb
    v = (c * bb) + (d * om)
    if not rounding:
        return v
    out = quantize(v, fmt, defect)
    if defect == "alpha_unrounded":
        out[..., 3] = v[..., 3]
    return out


def _walk(frame, width, height, fmt, background, target, occluder, z, exp_ulps, defect, exp, interval):
    assert fmt in FORMATS and (defect is None or defect in DEFECTS)
    W, H = F(width), F(height)
    s = _decode_splats(frame, W, H)
    order = frame["sorted"].astype(np.int64)
    if defect == "near_to_far":
        order = order[::-1]
    if defect == "tail_twice" and len(order) % 64:
        order = np.concatenate([order, order[-1:]])
    rounding = defect != "round_once"
    if target is not None:
        start = decode(fmt, target)
    else:
        start = np.broadcast_to(quantize(np.asarray(background, dtype=F), fmt), (height, width, 4))
    centre = np.array(start, dtype=F)
    lo, hi = (centre.copy(), centre.copy()) if interval else (None, None)
    ever_open = np.zeros((height, width), dtype=bool)
    fy_all, fx_all = F(np.arange(height)) + F(0.5), F(np.arange(width)) + F(0.5)
    for i in order:
        box = _box(s, i, width, height)
        if box is None:
            continue
        with np.errstate(all="ignore"):
            dx, dy = (fx_all[box[1]] - s["cx"][i])[None, :], (fy_all[box[0]] - s["cy"][i])[:, None]
            p0 = (s["i00"][i] * dx) + (s["i01"][i] * dy)
            p1 = (s["i10"][i] * dx) + (s["i11"][i] * dy)
            a = (p0 * p0) + (p1 * p1)
            kept = a <= CUT_A
            if occluder is not None:
                kept &= z[i] < occluder[box]
            if not kept.any():
                continue
            a, alpha, c = a[kept], s["alpha"][i], s["colour"][i]
            e = exp(-a)
            limit = (lambda b: b) if defect == "no_clamp" else (lambda b: np.minimum(CLAMP, b))
            sub = centre[box]
            sub[kept] = _step(c, limit(e * alpha)[:, None], sub[kept], fmt, defect, rounding)
            if interval:
                below, above, bbs = e, e, [e]
                for _ in range(exp_ulps):
                    below, above = np.nextafter(below, F(-np.inf)), np.nextafter(above, F(np.inf))
                    bbs += [below, above]
                bb = limit(np.stack(bbs) * alpha)[:, None, :, None]                  # [2 E + 1, 1, pairs, 1]
                ends = np.stack([lo[box][kept], hi[box][kept]])[None]                 # [1, 2, pairs, 4]
                image = _step(c, bb, ends, fmt, defect, rounding).reshape(-1, a.size, 4)
                for plane, value in ((lo, image.min(axis=0)), (hi, image.max(axis=0))):
                    sub = plane[box]
                    sub[kept] = value
                ever = ever_open[box]
                ever[kept] |= (image.min(axis=0) != image.max(axis=0)).any(axis=1)
    if not rounding or defect == "alpha_unrounded":  # (the store rounds whatever the walk did not)
        centre = quantize(centre, fmt)
    out = {"fmt": fmt, "centre": centre, "lo": lo, "hi": hi}
    if interval:
        out["open"] = (lo != hi).any(axis=2)
        out["ever_open"] = ever_open
    return out


def strict_walk(frame, width, height, fmt, background=(0.0, 0.0, 0.0, 0.0), target=None, occluder=None, z=None, exp_ulps=EXP_ULPS,
                defect=None):
    """The walk of `frame` (download_frame() or blend_ref.oracle_frame(): splats, sorted) into a width x height target of `fmt`:
    dict(fmt, centre, lo, hi, open, ever_open), images [H, W, 4] f32 of the target's precision.  background: the clear colour;
    target: the stored image the walk starts from instead (render_composite(load=True)); occluder [H, W] f32 with z [store slot]
    (download_depths()): a pair is kept only where z < occluder.  defect: one of DEFECTS; a defective walk has no interval
    (lo = hi = None), only its centre image."""
    return _walk(frame, width, height, fmt, background, target, occluder, z, exp_ulps, defect, _exp_f64, interval=defect is None)


def libm_walk(frame, width, height, fmt, background=(0.0, 0.0, 0.0, 0.0), target=None, occluder=None, z=None):
    """The image of the walk with the C library's expf: [H, W, 4] f32."""
    return _walk(frame, width, height, fmt, background, target, occluder, z, 0, None, _exp_libm, interval=False)["centre"]


def check(image, ref, fmt):
    """`image` (a downloaded target of fmt's dtype, or an f32 image of the target's precision) against strict_walk's `ref`.
    A value is OUTSIDE when its decode is not in [lo, hi], or -- where lo == hi -- its stored word is not the word of lo.
    Returns dict(pixels, open_pixels, ever_open_pixels, off_centre, max_units, outside, first): off_centre = values whose word is
    not the centre image's, max_units = the largest such distance in units of the last place, first = (y, x, channel, device
    value, lo, hi) of the first value outside or None."""
    v = decode(fmt, image)
    lo, hi = ref["lo"], ref["hi"]
    assert v.shape == lo.shape, (v.shape, lo.shape)
    got = _image_words(fmt, image)
    with np.errstate(invalid="ignore"):
        outside = ~((lo <= v) & (v <= hi))
    outside |= (lo == hi) & (got != words(fmt, lo))
    apart = units_apart(fmt, got, words(fmt, ref["centre"]))
    first = None
    if outside.any():
        y, x, ch = (int(t) for t in np.argwhere(outside)[0])
        first = (y, x, ch, float(v[y, x, ch]), float(lo[y, x, ch]), float(hi[y, x, ch]))
    return {"pixels": int(v.shape[0] * v.shape[1]), "open_pixels": int(ref["open"].sum()), "ever_open_pixels": int(ref["ever_open"].sum()),
            "off_centre": int((apart > 0).sum()), "max_units": int(apart.max()), "outside": int(outside.sum()), "first": first}


# ---- cached walks ------------------------------------------------------------------------------------------------------------
_CACHE = {}  # K1 and the depth sort do not depend on the launch form: one walk per frame, format and start serves every launch


def _digest(*arrays):
    d = hashlib.sha1()
    for a in arrays:
        d.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


def reference(frame, width, height, fmt, background=(0.0, 0.0, 0.0, 0.0), target=None, occluder=None, z=None):
    """strict_walk, remembered by the frame's bytes; the result is shared: leave it unchanged."""
    key = (_digest(frame["splats"], frame["sorted"], np.asarray(background, dtype=F), target, occluder, z if occluder is not None else None),
           width, height, fmt)
    if key not in _CACHE:
        _CACHE[key] = strict_walk(frame, width, height, fmt, background, target=target, occluder=occluder, z=z)
    return _CACHE[key]


# ---- the named frames ----------------------------------------------------------------------------------------------------------
STACK_K = (1, 63, 64, 65, 128, 129, 193)   # k_blend_strict walks a list in chunks of 64 entries, the last one clamped


def _cloud(rng, viewport, n, sigma_major, sigma_minor, opacity, colour, margin=3.0):
    """n Gaussians flat against the image plane of blend_ref's camera, at distinct depths in [-0.5, 0.5]: centres uniform over
    the viewport and `margin` px beyond, standard deviations (px) log-uniform in the two ranges along a random direction and
    across it, opacity log-uniform and colour uniform in theirs."""
    w, h = viewport

    def log_uniform(r, size):
        return np.exp(rng.uniform(np.log(r[0]), np.log(r[1]), size))

    zs = rng.permutation(np.linspace(-0.5, 0.5, n))
    depth = B.CAM_DIST + zs
    px, py = rng.uniform(-margin, w + margin, n), rng.uniform(-margin, h + margin, n)
    xyz = np.stack([(px - 0.5 * w) * depth / B.FOCAL, (py - 0.5 * h) * depth / B.FOCAL, zs], axis=1).astype(F)
    sig = np.stack([log_uniform(sigma_major, n), log_uniform(sigma_minor, n), np.full(n, 0.5)], axis=1)
    log_scale = np.log(sig * depth[:, None] / B.FOCAL).astype(F)
    theta = rng.uniform(0.0, np.pi, n)
    rot = np.stack([np.cos(0.5 * theta), np.zeros(n), np.zeros(n), np.sin(0.5 * theta)], axis=1).astype(F)  # about the optical axis
    op = log_uniform(opacity, n)
    logit = np.log(op / (1.0 - op)).astype(F)
    f_dc = ((rng.uniform(colour[0], colour[1], (n, 3)) - 0.5) / B.SH_C0).astype(F)
    return synth._rows(xyz, f_dc, np.zeros((n, 45), F), logit, log_scale, rot)


def _general():
    return _cloud(np.random.default_rng(11), (96, 64), 3000, (0.5, 2.0), (0.4, 1.2), (0.002, 0.9), (0.0, 1.0)), (96, 64)


def _needles():
    return _cloud(np.random.default_rng(12), (96, 64), 160, (10.0, 30.0), (0.3, 0.6), (0.02, 0.7), (0.0, 1.0)), (96, 64)


def _saturated():
    """Wide Gaussians whose f16 opacity is 1 or just below -- exp(-a) alpha passes 0.99 within 0.14 standard deviations of a
    centre -- with colours up to 3, between translucent ones that let the layers behind show through."""
    rng = np.random.default_rng(13)
    rows = np.concatenate([_cloud(rng, (64, 48), 100, (6.0, 24.0), (5.0, 16.0), (0.99, 0.99995), (0.0, 3.0)),
                           _cloud(rng, (64, 48), 50, (2.0, 8.0), (1.5, 5.0), (0.2, 0.8), (0.0, 3.0))])
    return rows, (64, 48)


def _edges(viewport, n, seed):
    """Small and middling Gaussians over a viewport with partial quadrants, a good share of them across its borders."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([_cloud(rng, viewport, n, (0.5, 2.0), (0.4, 1.2), (0.002, 0.9), (0.0, 1.0)),
                           _cloud(rng, viewport, n // 8, (3.0, 9.0), (1.0, 3.0), (0.01, 0.6), (0.0, 1.0), margin=6.0)])
    # (the two clouds' depths interleave; equal depths would leave the order to the sort's stability, which is fine too)
    return rows, viewport


STACK_CENTRE = (15.3, 16.6)


def stack_spec(k):
    """blend_ref's full stack (faint base records, markers around the chunk boundaries of 64) over a 32 x 32 viewport, but centred
    off the pixel grid's axes of symmetry: around (16, 16) eight pixels share every a, and one undecided rounding opens eight."""
    return B._spec(f"strict-stack-k{k}", lambda n: B._one(n, k, 64, B.FULL_SIGMA, STACK_CENTRE))


def _stack(k):
    spec = stack_spec(k)
    return spec.rows, spec.viewport


FRAMES = {"general": _general, "needles": _needles, "saturated": _saturated, "edges-33x17": lambda: _edges((33, 17), 200, 14),
          "edges-72x40": lambda: _edges((72, 40), 900, 15)}
FRAMES.update({f"stacks-k{k}": (lambda k=k: _stack(k)) for k in STACK_K})
EDGES = ("edges-33x17", "edges-72x40")
STACKS = tuple(f"stacks-k{k}" for k in STACK_K)
_BUILT = {}


def frame(name):
    """(rows, viewport) of a named frame, built once."""
    if name not in _BUILT:
        _BUILT[name] = FRAMES[name]()
    return _BUILT[name]


def exact_background(fmt):
    """A clear colour that the format holds exactly: quantising it is the identity."""
    if fmt == "rgba8unorm":
        return tuple(float(F(k) / F(255.0)) for k in (32, 64, 96, 128))
    return (0.125, 0.25, 0.375, 0.5)


# ---- what the composite cases start from -----------------------------------------------------------------------------------
OCCLUDERS = ("none", "constant", "by-quadrant")


def random_target(fmt, width, height, seed=7):
    """A random premultiplied target (colour <= alpha) of a narrow format's dtype, for render_composite(load=True)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (height, width, 1))
    img = np.concatenate([rng.uniform(0.0, 1.0, (height, width, 3)) * a, a], axis=2)
    return np.rint(img * 255.0).astype(np.uint8) if fmt == "rgba8unorm" else img.astype(np.float16)


def occluder_plane(kind, frame, z, width, height):
    """None, a constant view-space depth that leaves the nearest two thirds of the draw order, or one cut per 8 x 8 quadrant:
    around the 64-entry chunk boundaries of the order (counted from either end), through its middle and next to its ends.  z per
    store slot (download_depths() or oracle_frame's); every cut lies half way between two neighbouring depths."""
    if kind == "none":
        return None
    z_of = z[frame["sorted"].astype(np.int64)[::-1]]  # near to far
    n = len(z_of)
    assert np.all(np.diff(z_of) > 0)

    def between(m):  # records 0 .. m - 1, counted from the near end, pass z < D
        d = np.float32((np.float64(z_of[m - 1]) + np.float64(z_of[m])) / 2)
        assert z_of[m - 1] < d < z_of[m]
        return d

    if kind == "constant":
        return np.full((height, width), between((2 * n) // 3), dtype=np.float32)
    ms = sorted({m for m in (1, 2, 63, 64, 65, n - 65, n - 64, n - 63, n // 2, n // 3, n - 1) if 1 <= m < n})
    qy, qx = np.mgrid[0:height, 0:width] // 8
    return np.array([between(m) for m in ms], dtype=np.float32)[(qx + -(-width // 8) * qy) % len(ms)]
