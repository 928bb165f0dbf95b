"""k_blend (csrc/raster.hip) at its batch boundaries, in every launch form, against float64 -- on marker stacks (tests/blend_ref.py).

The siblings' boundary tests (test_gpu_contrib, test_gpu_attrib, test_gpu_values) run k_contrib and k_values; k_blend writes its
staging store, its compaction loop and its quadrant set-up out, and has machinery of its own: the two-deep prefetch of the next
batch's records and of the indices of the batch after it, the separately prefetched z of the depth forms, the next tile's first
batch in the several-tiles-per-workgroup forms, the piece rule of the compaction, the pad-to-four of a wave's list, the split
halves, the longest-first table, the list that 2 x 2 tiles share, the occluder's Dmax drop.  A frame here is a stack of faint
records with a few MARKER records at the list positions where that arithmetic changes; tests/test_blend_boundary_ref.py shows
from the reference alone that losing one marker, or exchanging two neighbours, moves some pixel of every covered quadrant by at
least ten times the gate below.

The gate (the tolerances the project states against float64: test_gpu_composite._check_f64, test_gpu_aux._check_against_f64):
|device - float64| <= 2e-4 per colour channel and for alpha on an rgba32float target, plus half a unit in the last place of the
target format on rgba16float / rgba8unorm; expected depth within 1e-4 max|z|; the median the exact f32 z unless the reference's
crossing lies within 1e-4 of T = 0.5.  EVERY pixel is compared: the test asserts that the device's own frame has no fragment
within f32 rounding of the cut-off.  Every case also asserts the exact tile list lengths, overflow == 0 and errors()[0] == 0.

  a. length sweep, plain FAST blend: four launches (whole 32 x 32 tiles, their halves, 32 x 16 and 16 x 16 tiles), three formats
  b. sparse quadrant masks: narrow stacks; one stack in a single quadrant beside a short one (list lengths 1, 2, 3, 5)
  c. the depth forms: expected depth, median, alpha; the median crossing on the first record of the second batch
  d. the composite: load over a random target; constant occluders that cut the list around the batch boundary; one by quadrant
  e. how lists are shared: several tiles per workgroup, split halves, the order table, 2 x 2 tiles on one list
  f. saturation across the boundary: one quadrant ends inside batch one, another needs batch two
  g. the exact-cut FAST mode; the strict kernel (stages 64 at a time) against the oracle's target modes
  h. the experimental variants (k_blend2, k_blend_q, LDS-DMA staging) on a and e: skipped against the product library

  h runs the 4x4 sweep of a and the 4x4 settings of e that each variant accepts (see VARIANTS below); c, d, f and g need the FAST
  production launch, which the variants are not.

A module-scoped fixture writes one row per case (form, k, largest |device - float64| per plane) to blend_boundary_report.json in
WEBSPLAT_REPORT_DIR (default: test_reports/ under the repository root, as tests/test_gpu_metrics.py).  With WS_BLEND_BOUNDARY_SAVE=<directory> every case also leaves its device image and frame
there (npz), for scripts/blend_boundary_recheck.py: the same comparison against a reference with one marker dropped or two
exchanged, which has to FAIL."""
import contextlib
import json
import os

import numpy as np
import pytest

import blend_ref as B
import scenes
from variants import exp_param

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAVE_DIR = os.environ.get("WS_BLEND_BOUNDARY_SAVE")
REPORT = []

F32_BG = (0.125, 0.25, 0.375, 0.5)  # exact in f16; for unorm8 the backgrounds are k / 255 (the format's decode)
U8_K = (32, 64, 96, 128)
# The launches.  A context of 4x4 tiles composites a 32 x 32 tile with ONE 1024-thread workgroup (k_blend<4, 4>: sixteen waves over
# a 512-entry batch that half of the threads stage -- the form bench.py measures) only when the halves are off: left to itself
# (blend_split = -1) a frame with fewer tiles than twice the CUs -- every frame here -- is composited by two 512-thread workgroups
# per tile (k_blend<4, 2> on 32 x 16 halves of the tile's list).  So "4x4" pins blend_split = 0, "split" pins 1 (the frames and
# lists of 4x4), and "auto" is the context's default, used only as the image the settings of e are compared with.  The API does
# not report which form a launch took (the kernel timers label every form "k_blend"); the pinning follows api_renderer.cpp
# render_frame / blend_form.h blend_frame_choice.
CFG = {"4x4": {"blend_split": 0}, "split": {"blend_split": 1}, "auto": {}, "4x2": {"tile_qw": 4, "tile_qh": 2}, "2x2": {"tile_qw": 2, "tile_qh": 2}}
FRAMES_OF = {"4x4": "4x4", "split": "4x4", "auto": "4x4", "4x2": "4x2", "2x2": "2x2"}  # launch -> the shape whose frames and lists it has
LAUNCHES = ("4x4", "split", "4x2", "2x2")
# The experimental variants (blend_form.h blend_form_of).  k_blend2 exists for one 32 x 32 tile per workgroup, no halves: under any
# other setting the library stages with barriers (k_blend) WITHOUT saying so, so its cases pin blend_split = 0 and
# blend_tpw_log2 = 0 and run only the settings that keep both.  k_blend_q has no tile shape, halves or tiles-per-workgroup of its
# own (every quadrant is a workgroup): it runs under every setting of the 4x4 context.  LDS-DMA staging is a flag of k_blend's
# forms and takes every setting.
VARIANTS = {"async": {"blend_async": 1, "blend_split": 0, "blend_tpw_log2": 0}, "q": {"exp_blend_variant": 1}, "dma": {"exp_blend_dma": 1}}
VARIANT_SETTINGS = {"async": ("tpw0", "order0", "order1", "bin2"), "q": None, "dma": None}  # None = all


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "blend_boundary_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _background(fmt):
    return tuple(float(np.float32(k) / np.float32(255.0)) for k in U8_K) if fmt == "rgba8unorm" else F32_BG


def _random_target(fmt, w, h, seed):
    """A random premultiplied target (colour <= alpha) of the target's dtype, and its decode (test_gpu_composite._random_target)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (h, w, 1))
    img = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)) * a, a], axis=2)
    if fmt == "rgba8unorm":
        enc = np.rint(img * 255.0).astype(np.uint8)
        return enc, enc.astype(np.float64) / 255.0
    enc = img.astype(np.float16 if fmt == "rgba16float" else np.float32)
    return enc, enc.astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@contextlib.contextmanager
def _open(ws, spec, fmt="rgba32float", depth=False, mode="fast", lengths=None, **cfg):
    """A context of `cfg`, the frame's cloud and a renderer with the frame prepared: (renderer, cloud).  `lengths`: what
    tile_stats()["list_len"] has to be.  On the way out: no overflow, no error bit."""
    c = ws.Context(0, ws.config_from_env({}, **cfg))
    try:
        gpc, args = B.device_scene(ws, spec.rows, spec.viewport)
        pc = ws.PointCloud(c, gpc)
        r = ws.GaussianRenderer(c, fmt, 3, False)
        try:
            if mode != "fast":
                r.set_blend_mode(mode)
            if depth:
                r.enable_depth(True)
            r.prepare(pc, args)
            if lengths is not None:
                got = r.tile_stats()["list_len"]
                assert np.array_equal(got, lengths), f"tile list lengths {got.tolist()}, intended {lengths.tolist()}"
            yield r, pc
            assert r.frame_stats()["overflow"] == 0
            assert r.errors()[0] == 0
        finally:
            r.close()
            pc.close()
    finally:
        c.close()


def _reference(spec, r, depth=False, occluder=None):
    """(frame, z, reference) of the renderer's own prepared frame; asserts that no pixel has an undecided fragment."""
    w, h = spec.viewport
    frame = r.download_frame()
    assert frame["num_visible"] == len(spec.rows)
    z = r.download_depths() if depth else None
    ref = B.reference(frame, z, w, h, occluder=occluder)
    assert not ref["undecided"].any()
    return frame, z, ref


def _row(case, spec, form, **more):
    row = dict(case=case, frame=spec.name, form=form, k=[st["k"] for st in spec.stacks])
    row.update(more)
    REPORT.append(row)
    return row


def _check_colour(row, fmt, image, want, name="colour"):
    worst, excess = B.colour_errors(fmt, image, want)
    row[name] = worst
    print(f"{row['case']} {row['frame']} {row['form']}: largest |device - float64| {name} {worst:.3e} (excess over the gate {excess:.3e})")
    assert excess <= 0.0, f"{name}: {worst:.3e} is {excess:.3e} over the gate"


def _check_planes(row, planes, ref, z):
    res = B.plane_errors(planes, ref, float(np.abs(z).max()) if z is not None else 0.0)
    for name, (worst, ok) in res.items():
        row[name] = worst
    print(f"{row['case']} {row['frame']} {row['form']}: " + ", ".join(f"{n} {w:.3e}" for n, (w, _) in res.items()))
    for name, (worst, ok) in res.items():
        assert ok, f"{name}: {worst:.3e}"


def _save(row, spec, fmt, image, frame, z=None, target=None, occluder=None, planes=None):
    if not SAVE_DIR:
        return
    os.makedirs(SAVE_DIR, exist_ok=True)
    name = "_".join(str(row[k]) for k in ("case", "frame", "form")).replace(" ", "").replace("/", "-")
    extra = {k: v for k, v in dict(z=z, target=target, occluder=occluder).items() if v is not None}
    extra.update({"plane_" + k: v for k, v in (planes or {}).items()})
    np.savez_compressed(os.path.join(SAVE_DIR, name + ".npz"), image=image, splats=frame["splats"], sorted=frame["sorted"],
                        fmt=fmt, spec=spec.name, viewport=np.array(spec.viewport), **extra)


def _plain(ws, case, spec, shape, fmt, bg, form, mode="fast", lengths="tile", **cfg):
    """render() of the frame under `cfg` against float64 over `bg`; returns the image.  lengths: "tile" / "coarse" = the frame
    has to have binned at the blend's tile / at 2 x 2 of them, with exactly the intended list lengths; None = as the device decides."""
    want = spec.list_lengths(FRAMES_OF[shape], coarse=lengths == "coarse") if lengths else None
    with _open(ws, spec, fmt, mode=mode, lengths=want, **dict(CFG[shape], **cfg)) as (r, pc):
        if lengths:
            tile = B.tile_px(FRAMES_OF[shape])
            assert r.binning_tile() == ((2 * tile[0], 2 * tile[1]) if lengths == "coarse" else tile)
        r.render(pc, background=bg)
        image = r.download_target().copy()
        frame, _, ref = _reference(spec, r)
        row = _row(case, spec, form)
        _save(row, spec, fmt, image, frame, target=np.array(bg))
        _check_colour(row, fmt, image, B.over(ref, bg, fmt))
    return image


def _variant_params(base, also):
    """`base` (a list of value tuples) as it is, and those `also(variant)` picks of it once more under each experimental variant."""
    out = [v + (None,) for v in base]
    for name in VARIANTS:
        out += [exp_param(*(v + (name,))) for v in base if also(name, v)]
    return out


def _variant_cfg(variant):
    return VARIANTS[variant] if variant else {}


# ---- a. length sweep --------------------------------------------------------------------------------------------------------
SWEEP = [(shape, k) for shape in LAUNCHES for k in B.SWEEP[FRAMES_OF[shape]]]


def _stage(shape):
    return B.STAGE[B.SHAPES[FRAMES_OF[shape]]]


# (the experimental variants: the sweep of the 4x4 context, see VARIANTS)
@pytest.mark.parametrize("shape,k,variant", _variant_params(SWEEP, lambda variant, v: v[0] == "4x4"))
def test_length_sweep(ws, shape, k, variant):
    spec = B.full(k, _stage(shape))
    _plain(ws, "a" if not variant else "h-a", spec, shape, "rgba32float", (0.0, 0.0, 0.0, 0.0), f"{shape}-f32" + (f"-{variant}" if variant else ""),
           bin_request=0, **_variant_cfg(variant))


LONGEST = [(shape, k, fmt) for shape in LAUNCHES for k in sorted(B.SWEEP[FRAMES_OF[shape]])[-3:] for fmt in ("rgba16float", "rgba8unorm")]


@pytest.mark.parametrize("shape,k,fmt", LONGEST)
def test_length_sweep_narrow_targets(ws, shape, k, fmt):
    spec = B.full(k, _stage(shape))
    _plain(ws, "a", spec, shape, fmt, _background(fmt), f"{shape}-{fmt[4:]}-bg", bin_request=0)


# ---- b. sparse masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", B.SPARSE_SIGMAS)
@pytest.mark.parametrize("shape,k", SWEEP)
def test_sparse_masks(ws, shape, k, sigma):
    _plain(ws, "b", B.sparse(k, FRAMES_OF[shape], sigma), shape, "rgba32float", F32_BG, f"{shape}-f32-bg", bin_request=0)


@pytest.mark.parametrize("short", B.SHORT)
@pytest.mark.parametrize("shape", LAUNCHES)
def test_single_quadrant_beside_a_short_stack(ws, shape, short):
    _plain(ws, "b", B.single(FRAMES_OF[shape], short), shape, "rgba32float", F32_BG, f"{shape}-f32-bg", bin_request=0)


# ---- c. the depth forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", B.MEDIAN_CASES + [("split", k) for s, k in B.MEDIAN_CASES if s == "4x4"])
def test_depth_forms(ws, shape, k):
    spec = B.median(FRAMES_OF[shape], k)
    with _open(ws, spec, depth=True, lengths=spec.list_lengths(FRAMES_OF[shape]), bin_request=0, **CFG[shape]) as (r, pc):
        r.render(pc, background=F32_BG)
        plain = r.download_target().copy()
        r.render_aux(pc, depth=True, median_depth=True, alpha=True, background=F32_BG)
        image, planes = r.download_target().copy(), r.download_aux()
        frame, z, ref = _reference(spec, r, depth=True)
        row = _row("c", spec, f"{shape}-f32-aux")
        _save(row, spec, "rgba32float", image, frame, z=z, target=np.array(F32_BG), planes=planes)
        assert np.array_equal(_bits(plain), _bits(image)), "the colour of the aux launch is not the plain launch's"
        _check_colour(row, "rgba32float", image, B.over(ref, F32_BG))
        _check_planes(row, planes, ref, z)
        # the frame is what the CPU test says it is: the centre pixels' crossing lies on the first record of the second batch
        z_of = z[frame["sorted"].astype(np.int64)[::-1]]
        centre = (slice(15, 17), slice(15, 17))
        assert np.all(ref["median"][centre] == z_of[spec.stage]) and ref["tcross"][centre].min() > 100 * B.NEAR_HALF
        assert np.all(planes["median_depth"][centre] == z_of[spec.stage])


# ---- d. the composite ---------------------------------------------------------------------------------------------------------
COMPOSITE = [("4x4", 1025), ("split", 1025), ("4x2", 1025), ("2x2", 513)]


def _between(z_of, m):
    """A depth between list positions m - 1 and m (m = len: behind the last): records 0 .. m - 1 pass z < D."""
    if m == len(z_of):
        return np.float32(z_of[-1] + np.float32(0.01))
    d = np.float32((np.float64(z_of[m - 1]) + np.float64(z_of[m])) / 2)
    assert z_of[m - 1] < d < z_of[m]
    return d


def _cuts(stage, k):
    return [1, stage - 1, stage, stage + 1, k]


@pytest.mark.parametrize("cut", range(7), ids=["load", "m1", "mS-1", "mS", "mS+1", "mk", "by-quadrant"])
@pytest.mark.parametrize("shape,k", COMPOSITE)
def test_composite(ws, shape, k, cut):
    spec = B.full(k, _stage(shape))
    w, h = spec.viewport
    with _open(ws, spec, depth=True, lengths=spec.list_lengths(FRAMES_OF[shape]), bin_request=0, **CFG[shape]) as (r, pc):
        z = r.download_depths()
        z_of = z[r.download_frame()["sorted"].astype(np.int64)[::-1]]
        assert np.all(np.diff(z_of) > 0)
        if cut == 0:
            occ = None
        elif cut <= 5:
            occ = np.full((h, w), _between(z_of, _cuts(spec.stage, k)[cut - 1]), dtype=np.float32)
        else:  # one cut per 8 x 8 quadrant, cycling through the boundary cuts and a few inside the batches
            ms = _cuts(spec.stage, k) + [2, 255, 256, 257, spec.stage + 255, spec.stage + 256, 64, 5]
            ms = [m for m in ms if 1 <= m <= k]
            qy, qx = np.mgrid[0:h, 0:w] // 8
            occ = np.array([_between(z_of, m) for m in ms], dtype=np.float32)[(qx + (w // 8) * qy) % len(ms)]
        enc, dst = _random_target("rgba32float", w, h, seed=100 + cut)
        r.upload_target(enc)
        r.render_composite(pc, load=True, occluder=occ, alpha=True)
        image, planes = r.download_target().copy(), r.download_aux()
        frame, z, ref = _reference(spec, r, depth=True, occluder=occ)
        row = _row("d", spec, f"{shape}-f32-load-" + ("none" if cut == 0 else "quadrants" if cut == 6 else f"m{_cuts(spec.stage, k)[cut - 1]}"))
        _save(row, spec, "rgba32float", image, frame, z=z, target=dst, occluder=occ, planes=planes)
        _check_colour(row, "rgba32float", image, B.over(ref, dst))
        _check_planes(row, planes, ref, z)
        if 1 <= cut <= 5:  # (the cut is where it was meant to be: the pixels at the centre hold exactly the first m records' coverage)
            m = _cuts(spec.stage, k)[cut - 1]
            assert (ref["T"] < 1.0).any() and np.array_equal(z_of < occ[0, 0], np.arange(k) < m)


# ---- e. how lists are shared --------------------------------------------------------------------------------------------------
# (on top of CFG[shape]: every 4x4 setting but split1 composites whole 32 x 32 tiles, blend_split = 0)
SHARED_SETTINGS = {
    "4x4": [("tpw0", "tile", dict(bin_request=0, blend_tpw_log2=0)), ("tpw1", "tile", dict(bin_request=0, blend_tpw_log2=1)),
            ("tpw2", "tile", dict(bin_request=0, blend_tpw_log2=2)), ("split1", "tile", dict(bin_request=0, blend_split=1)),
            ("order0", "tile", dict(bin_request=0, blend_order=0, blend_tpw_log2=0)),
            ("order1", "tile", dict(bin_request=0, blend_order=1, blend_tpw_log2=0)), ("bin2", "coarse", dict(bin_request=2, blend_tpw_log2=0))],
    "2x2": [("tpw0", "tile", dict(bin_request=0, blend_tpw_log2=0)), ("tpw2", "tile", dict(bin_request=0, blend_tpw_log2=2)),
            ("tpw4", "tile", dict(bin_request=0, blend_tpw_log2=4))],  # (only the 4x4 tile bins at 2 x 2 of its size)
}
SHARED = [("4x4", which, s) for which in B.SHARED_4X4 for s in SHARED_SETTINGS["4x4"]] + [("2x2", "a", s) for s in SHARED_SETTINGS["2x2"]]
_DEFAULT_IMAGE = {}


def _default_image(ws, spec, shape, variant=None):
    """The image of the frame under the default settings of the tile shape (the device decides the binning tile and, at 4x4,
    whether the halves are on): k_blend's, or -- variant "q" -- k_blend_q's."""
    key = (spec.name, variant)
    if key not in _DEFAULT_IMAGE:
        _DEFAULT_IMAGE[key] = _plain(ws, "e" if not variant else "h-e", spec, "auto" if shape == "4x4" else shape, "rgba32float", F32_BG,
                                     f"{shape}-f32-default" + (f"-{variant}" if variant else ""), lengths=None, **_variant_cfg(variant))
    return _DEFAULT_IMAGE[key]


# (the experimental variants: every setting of the 4x4 context that the variant accepts, see VARIANTS)
@pytest.mark.parametrize("shape,which,setting,variant",
                         _variant_params(SHARED, lambda variant, v: v[0] == "4x4" and (VARIANT_SETTINGS[variant] is None or v[2][0] in VARIANT_SETTINGS[variant])),
                         ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_shared_lists(ws, shape, which, setting, variant):
    """Every setting draws the image of the default setting of the same frame, bit for bit.  k_blend2 and the LDS-DMA staging are
    k_blend's arithmetic under another schedule and have to draw K_BLEND's default image.  k_blend_q is another kernel (one wave
    per quadrant, records broadcast from registers, its own evaluation order): it meets the float64 gate, and its settings have
    to agree bit for bit with ITS OWN default setting; how far it is from k_blend's image is printed and recorded."""
    name, lengths, cfg = setting
    spec = B.shared(shape, which)
    image = _plain(ws, "e" if not variant else "h-e", spec, shape, "rgba32float", F32_BG, f"{shape}-f32-{name}" + (f"-{variant}" if variant else ""),
                   lengths=lengths, **dict(cfg, **_variant_cfg(variant)))
    row, own = REPORT[-1], "q" if variant == "q" else None
    assert np.array_equal(_bits(image), _bits(_default_image(ws, spec, shape, own))), "not the image of the default setting"
    if own:
        apart = float(np.abs(image.astype(np.float64) - _default_image(ws, spec, shape).astype(np.float64)).max())
        row["from_k_blend"] = apart
        print(f"k_blend_q differs from k_blend's image of the frame by at most {apart:.3e}")


# ---- f. saturation across the boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LAUNCHES)
def test_saturation_across_the_boundary(ws, shape):
    spec = B.saturating(FRAMES_OF[shape])
    with _open(ws, spec, depth=True, lengths=spec.list_lengths(FRAMES_OF[shape]), bin_request=0, **CFG[shape]) as (r, pc):
        r.render(pc, background=F32_BG)
        image = r.download_target().copy()
        frame, z, ref = _reference(spec, r, depth=True)
        near, far = (ref["first_below"][8 * q[1]:8 * q[1] + 8, 8 * q[0]:8 * q[0] + 8] for q in spec.quadrants)
        print(f"first list position below T_MIN: {near.min()} .. {near.max()} in quadrant {spec.quadrants[0]}, {far.min()} .. {far.max()} "
              f"in quadrant {spec.quadrants[1]}")
        assert near.max() < spec.stage <= far.min() and far.max() < len(spec.rows)
        row = _row("f", spec, f"{shape}-f32-bg")
        _save(row, spec, "rgba32float", image, frame, target=np.array(F32_BG))
        _check_colour(row, "rgba32float", image, B.over(ref, F32_BG))


# ---- g. the exact cut and the strict kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [513, 1024, 1025])
@pytest.mark.parametrize("shape", ["4x4", "split"])
def test_exact_cut_mode(ws, shape, k):
    _plain(ws, "g", B.full(k, 512), shape, "rgba32float", F32_BG, f"{shape}-f32-exact-cut", mode="fast_exact_cut", bin_request=0)


@pytest.mark.parametrize("fmt,mode", [("rgba32float", 0), ("rgba16float", 1), ("rgba8unorm", 2)])
@pytest.mark.parametrize("k", B.STRICT_K)
def test_strict_kernel_against_the_oracle(ws, oracle, k, fmt, mode):
    """k_blend_strict (back to front, the destination rounded to the target's precision after every record) against the oracle's
    target modes over the library's own records and order: f32 within 2e-5 at every pixel (no boundary allowance), f16 and unorm8
    within one unit of the target's last place at every value.  The share of values that differ at all is recorded, not gated."""
    spec = B.strict(k)
    w, h = spec.viewport
    bg = (0.25, 0.5, 0.125, 1.0)
    with _open(ws, spec, fmt, mode="target", lengths=spec.list_lengths("4x4"), bin_request=0) as (r, pc):
        r.render(pc, background=bg)
        got = r.download_target().copy()
        frame = r.download_frame()
        assert frame["num_visible"] == k
        ref = oracle.render(frame["splats"], frame["sorted"], w, h, bg, mode)
        if mode == 0:
            units = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            worst, differ, ok = float(units.max()), float((units > 0).mean()), units.max() <= 2e-5
        elif mode == 1:
            units = scenes.half_ulp_diff(got.view(np.uint16), ref.astype(np.float16).view(np.uint16))
            worst, differ, ok = int(units.max()), float((units > 0).mean()), units.max() <= 1
        else:
            units = np.abs(got.astype(np.int64) - np.rint(ref * 255.0).astype(np.int64))
            worst, differ, ok = int(units.max()), float((units > 0).mean()), units.max() <= 1
        _row("g", spec, f"strict-{fmt[4:]}", worst=worst, share_differing=differ)
        print(f"g {spec.name} strict-{fmt[4:]}: largest difference {worst} ({'absolute' if mode == 0 else 'units in the last place'}), "
              f"share of values that differ {differ:.3e}")
        assert ok, worst
