"""k_blend_strict (csrc/raster.hip: set_blend_mode("target"), the blend the project answers to the reference with) held to the bit
by the numpy restatement of tests/strict_ref.py, in every launch shape.

Every operation of the kernel but expf is an IEEE f32 operation that numpy repeats exactly; expf gets an interval of +-2 ulps
around the correctly rounded value, carried through the walk per pixel and channel.  On rgba16float and rgba8unorm the rounding
after every record swallows that interval on all but a few pixels (tests/test_strict_ref.py caps their share at 1 % per frame, from
the reference alone), so nearly every stored word has exactly one right value; the others have a few.  Each case prepares a
named frame under the context's settings, renders in the target mode, downloads the device's OWN frame (records, draw order and,
for an occluder, depths), walks it on the CPU and runs strict_ref.check: every value inside [lo, hi], and the stored word equal
where lo == hi.  The reference does not restate the kernel's quadrant test, its tile mapping, the clamped last chunk or the
shared lists: it walks the whole draw order at every pixel, so whatever the launch geometry loses, repeats or misplaces is an
error.  Every case also asserts the intended binning tile, overflow == 0 and errors()[0] == 0.

  launch shapes  general, needles, edges-33x17, edges-72x40 x tiles {4x4, 4x2, 2x2} x bin_request {0, and 2 at 4x4: only that
                 shape bins at 2 x 2 of its tiles} x {rgba16float, rgba8unorm}; rgba32float on general at the three shapes, where
                 nothing swallows the interval: containment only
  stacks         k = 1, 63, 64, 65, 128, 129, 193 at 4x4 and 2x2: the 64-entry chunk boundaries and the clamped tail
  saturated      opacities on the 0.99 clamp, colours above 1
  composite      general and the stack of 129: load over a random premultiplied target of the format; that with a constant
                 occluder between two list positions; that with one cut per 8 x 8 quadrant

A module-scoped fixture writes one row per case to blend_strict_exactness.json in WEBSPLAT_REPORT_DIR (default: test_reports/
under the repository root): pixels, pixels whose interval is open, values that are not the centre image's (the walk with the
correctly rounded exp), the largest such distance in units of the last place, and values outside their interval, which has to be
0.  How far the device's expf lands from the centre is recorded there, not gated beyond containment."""
import contextlib
import json
import os

import numpy as np
import pytest

import blend_ref as B
import strict_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
NARROW = ("rgba16float", "rgba8unorm")
# launch -> (context settings, the binning tile the frame has to report)
LAUNCHES = {"4x4-bin0": (dict(bin_request=0), (32, 32)), "4x4-bin2": (dict(bin_request=2), (64, 64)),
            "4x2-bin0": (dict(tile_qw=4, tile_qh=2, bin_request=0), (32, 16)), "2x2-bin0": (dict(tile_qw=2, tile_qh=2, bin_request=0), (16, 16))}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "blend_strict_exactness.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


@contextlib.contextmanager
def _open(ws, name, fmt, launch, depth=False):
    """A context of the launch's settings with the named frame prepared in the target mode: (renderer, cloud, device frame)."""
    cfg, tile = LAUNCHES[launch]
    rows, viewport = S.frame(name)
    c = ws.Context(0, ws.config_from_env({}, **cfg))
    try:
        gpc, args = B.device_scene(ws, rows, viewport)
        pc = ws.PointCloud(c, gpc)
        r = ws.GaussianRenderer(c, fmt, 3, False)
        try:
            r.set_blend_mode("target")
            if depth:
                r.enable_depth(True)
            r.prepare(pc, args)
            assert r.binning_tile() == tile, f"binning tile {r.binning_tile()}, intended {tile}"
            frame = r.download_frame()
            assert frame["num_visible"] > 0.5 * len(rows)
            yield r, pc, frame
            assert r.frame_stats()["overflow"] == 0
            assert r.errors()[0] == 0
        finally:
            r.close()
            pc.close()
    finally:
        c.close()


def _judge(case, name, launch, fmt, image, ref):
    res = S.check(image, ref, fmt)
    first = res.pop("first")
    REPORT.append(dict(case=case, frame=name, launch=launch, format=fmt, **res))
    print(f"{case} {name} {launch} {fmt}: {res}")
    assert res["outside"] == 0, f"{res['outside']} values outside their interval; the first (y, x, channel, device, lo, hi): {first}"
    return res


def _plain(ws, case, name, launch, fmt, whole_lists=None):
    """whole_lists = k: the frame is one stack of k records, and every tile's list is all of them."""
    w, h = S.frame(name)[1]
    bg = S.exact_background(fmt)
    with _open(ws, name, fmt, launch) as (r, pc, frame):
        if whole_lists is not None:
            assert frame["num_visible"] == whole_lists and np.all(r.tile_stats()["list_len"] == whole_lists)
        r.render(pc, background=bg)
        image = r.download_target().copy()
        res = _judge(case, name, launch, fmt, image, S.reference(frame, w, h, fmt, bg))
    return res


# ---- launch shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("name", ("general", "needles") + S.EDGES)
def test_launch_shapes(ws, name, launch, fmt):
    res = _plain(ws, "shapes", name, launch, fmt)
    assert res["open_pixels"] <= S.MAX_OPEN * res["pixels"]  # (the device's frame is as decided as the oracle's)


@pytest.mark.parametrize("launch", ("4x4-bin0", "4x2-bin0", "2x2-bin0"))
def test_launch_shapes_f32_containment(ws, launch):
    _plain(ws, "shapes-f32", "general", launch, "rgba32float")


# ---- stacks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("launch", ("4x4-bin0", "2x2-bin0"))
@pytest.mark.parametrize("k", S.STACK_K)
def test_stacks(ws, k, launch, fmt):
    res = _plain(ws, "stacks", f"stacks-k{k}", launch, fmt, whole_lists=k)
    assert res["open_pixels"] <= S.MAX_OPEN * res["pixels"]


# ---- saturated -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NARROW)
def test_saturated(ws, fmt):
    res = _plain(ws, "saturated", "saturated", "4x4-bin0", fmt)
    assert res["open_pixels"] <= S.MAX_OPEN * res["pixels"]


# ---- composite -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("occluder", S.OCCLUDERS)
@pytest.mark.parametrize("name,launch", [("general", "4x4-bin0"), ("general", "2x2-bin0"), ("stacks-k129", "4x4-bin0")])
def test_composite(ws, name, launch, fmt, occluder):
    w, h = S.frame(name)[1]
    with _open(ws, name, fmt, launch, depth=True) as (r, pc, frame):
        z = r.download_depths()
        occ = S.occluder_plane(occluder, frame, z, w, h)
        target = S.random_target(fmt, w, h)
        r.upload_target(target)
        r.render_composite(pc, load=True, occluder=occ)
        image = r.download_target().copy()
        ref = S.reference(frame, w, h, fmt, target=target, occluder=occ, z=z)
        res = _judge("composite-" + occluder, name, launch, fmt, image, ref)
        assert res["open_pixels"] <= S.MAX_OPEN * res["pixels"]
        if occ is not None:  # (the occluder removes something: the image is not the unoccluded walk's)
            free = S.reference(frame, w, h, fmt, target=target)
            assert S.check(image, free, fmt)["outside"] > 0
