"""Hostile images for the two streaming entry points behind the frame -- ws_display_composite (k_display of raster.hip) and
ws_download_texture_rgba8 (drivers.cpp) -- and the references they are held to.  Plain numpy, no GPU;
tests/test_gpu_display_edges.py runs them, tests/test_display_images.py checks the builder.

The display computes, per channel, out = c + background * (1 - a), clamps to [0, 1] with NaN -> 0, multiplies by 255 and rounds
half to even.  raster.hip is compiled with contraction on, so background * k + c may or may not be one fused operation.  Two
classes of input keep that freedom out of the comparison:

EXACT class (exact_image, EXACT_BACKGROUNDS).  Backgrounds from {0, 0.5, 1}; colour and alpha multiples of 2^-8 in
  [-0.25, 1.25] (exact in f16 too), beside NaN, +-inf, -0 and alpha in {-0.5, 0, 1, 1.5, NaN}.  Then k = 1 - a, background * k and
  c + background * k are all exactly representable in f32 wherever they are finite, so a fused and an unfused evaluation give the
  same value, and the non-finite cases (inf - inf, 0 * inf, NaN) are the same in both.  An rgba8unorm source decodes to
  fl(code / 255); background * k is still exact for these backgrounds, so the sum is rounded once either way.  The f32
  restatement (display_composite of oracle/ws_oracle_io.py) must be met byte for byte.  rgba32float images also hold, under
  alpha 1, the f32 values v_m = fl((m + 0.5) / 255) for which fl(v_m * 255) is m + 0.5 exactly -- the rounding rule (half to
  even, not half up) is visible on them; the dyadic 0.5 (127.5 -> 128) is in every float image.

GENERAL class (general_image, general_background).  Colour and alpha uniform in [-0.25, 1.25], backgrounds uniform in [0, 1],
  against float64.  Bound on the device's f32 value, whatever the contraction: |c| <= 1.25, |k| <= 1.25 < 2, |t| = |background * k|
  < 2, |c + t| < 4.  An rgba8unorm texel decodes with one rounding below 1: 2^-25 for c and for a.  k = fl(1 - a): half an ulp
  below 2, 2^-24, plus a's 2^-25.  t = fl(background * k): background (<= 1) times k's error, plus half an ulp below 2, 2^-24 (a
  fused evaluation does not round t: smaller).  out = fl(c + t): half an ulp below 4, 2^-23.  Sum:
      E = 2^-25 + (2^-24 + 2^-25) + 2^-24 + 2^-23 = 5 * 2^-24 ~ 3.0e-7.
  The clamp does not increase an error; fl(clamp * 255) adds half an ulp below 256, 2^-17.  So a value is DECIDED when
  255 * clamp(v) is further than MARGIN = 255 * E + 2^-17 ~ 8.4e-5 from every m + 0.5: there the device must give
  rint(255 * clamp(v)) exactly; elsewhere it may give either neighbour.  About 2 * MARGIN of the unclamped values are undecided;
  tests/test_display_images.py asserts the share below 1 % on every committed image, from the reference alone.

The read-back is clamp (NaN -> 0), * 255, truncation (download_texture_u8); rgba8unorm is copied.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ws_oracle_io as oio  # noqa: E402

F = np.float32
SIZES = ((1, 1), (63, 3), (64, 4), (65, 5), (129, 9))            # width x height; k_display: 64 x 4 pixels per workgroup
SOURCES = ("rgba32float", "rgba16float", "rgba8unorm")
SURFACES = ("rgba8unorm", "bgra8unorm")
DTYPES = {"rgba32float": np.float32, "rgba16float": np.float16, "rgba8unorm": np.uint8}
SRC_PAD, DST_PAD = 48, 12                                        # bytes behind every row; 48 keeps any texel size aligned
SRC_FILL, DST_FILL = 0xFF, 0xA5
EXACT_BACKGROUNDS = ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.0, 0.5, 1.0, 1.0), (1.0, 0.0, 0.5, 0.0))
E_BOUND = 5 * 2.0 ** -24
MARGIN = 255 * E_BOUND + 2.0 ** -17
MAX_UNDECIDED = 0.01


def half_landings():
    """[(m, v)]: the f32 values v = fl((m + 0.5) / 255) whose f32 product with 255 is m + 0.5 exactly"""
    m = np.arange(255)
    v = ((m + 0.5) / 255.0).astype(F)
    hit = (v * F(255.0)).astype(np.float64) == m + 0.5
    return list(zip(m[hit].tolist(), v[hit].tolist()))


def decode(img):
    """the texel as the kernel decodes it: f32 as stored, f16 -> f32, unorm8 as (float)k / 255.0f"""
    return img.astype(F) / F(255.0) if img.dtype == np.uint8 else img.astype(F)


@functools.lru_cache(maxsize=None)
def exact_image(w, h, fmt, seed=0):
    """H x W x 4 of the format's dtype, read-only"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h + 100 * SOURCES.index(fmt))
    n = w * h
    if fmt == "rgba8unorm":
        img = rng.integers(0, 256, (n, 4))
        if n >= 256:                                            # every code in every channel, in another order in each
            for ch in range(4):
                img[:256, ch] = rng.permutation(256)
        img = img.astype(np.uint8)
    else:
        img = (rng.integers(-64, 321, (n, 4)) / 256.0).astype(F)
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 1.0, 0.0, -0.25], F)
        pick = rng.random((n, 3)) < 0.2
        img[:, :3][pick] = rng.choice(special, int(pick.sum()))
        alphas = np.array([-0.5, 0.0, 1.0, 1.5, np.nan, 0.5, np.inf, -np.inf], F)
        pick = rng.random(n) < 0.5
        img[pick, 3] = rng.choice(alphas, int(pick.sum()), p=[0.15, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05])
        if n >= 16:                                             # the edges that must be there whatever the draw
            img[0] = (0.5, np.nan, np.inf, 1.0)
            img[1] = (-np.inf, -0.25, 0.5, 0.0)
            img[2] = (0.25, 0.5, 0.75, np.nan)
            img[3] = (0.5, 0.5, 0.5, 1.5)
            img[4] = (1.0, 0.0, 0.5, -0.5)
            img[5] = (np.inf, 0.5, -np.inf, np.inf)
        else:
            img[0] = (0.5, np.nan, np.inf, 1.0)
        if fmt == "rgba32float" and n >= 256:                   # m + 0.5 after the multiply, under alpha 1: out = c exactly
            lands = half_landings()
            for i, (m, v) in enumerate(lands[:n - 16]):
                img[16 + i] = (v, lands[(i + 1) % len(lands)][1], lands[(i + 2) % len(lands)][1], 1.0)
        img = img.astype(DTYPES[fmt])
    img = img.reshape(h, w, 4)
    img.setflags(write=False)
    return img


def general_background(seed):
    rng = np.random.default_rng(77 + seed)
    return tuple(float(F(v)) for v in rng.uniform(0, 1, 4))


@functools.lru_cache(maxsize=None)
def general_image(w, h, fmt, seed=0):
    rng = np.random.default_rng(5000 + 1000 * seed + 7 * w + h + 100 * SOURCES.index(fmt))
    if fmt == "rgba8unorm":
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    else:
        img = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(DTYPES[fmt])
    img.setflags(write=False)
    return img


def composite_f32(img, background, surface):
    """the f32 restatement, unfused: what the EXACT class must meet byte for byte"""
    return oio.display_composite(decode(img), background, bgra=surface == "bgra8unorm")


def composite_f64(img, background, surface):
    """(want H x W x 4 uint8, decided H x W x 4 bool) from float64: want = rint(255 * clamp(v)); decided where that is
    further than MARGIN from every m + 0.5"""
    src = img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)
    bg = np.array([F(b) for b in background], F).astype(np.float64)
    v = src + bg * (1.0 - src[..., 3:4])
    s = 255.0 * np.clip(v, 0.0, 1.0)
    want = np.rint(s).astype(np.uint8)
    decided = np.abs(s - np.floor(s) - 0.5) > MARGIN
    if surface == "bgra8unorm":
        want, decided = want[..., [2, 1, 0, 3]], decided[..., [2, 1, 0, 3]]
    return want, decided


def readback(img):
    """ws_download_texture_rgba8: clamp with NaN -> 0, * 255, truncation; unorm8 copied"""
    return img.copy() if img.dtype == np.uint8 else oio.download_texture_u8(img)


def padded(img, pad=SRC_PAD, fill=SRC_FILL):
    """the image's rows with `pad` bytes of `fill` behind each: (H, row + pad) uint8"""
    h, w = img.shape[:2]
    row = w * 4 * img.itemsize
    host = np.full((h, row + pad), fill, dtype=np.uint8)
    host[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    return host
