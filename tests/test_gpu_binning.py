"""Binning (web-splat_amd/csrc/raster.hip k_bin_prefix / k_bin_emit, emit_gen.h) and the tile-id sort with its range recording
(sort.hip) against exact lists, on footprints the caller decides (tests/bin_patterns.py; tests/test_bin_patterns.py shows on the
CPU that every pattern is decided, drawn in the intended order and reaches the edge it is named for).

Per prepared frame (_check): the tile lists the device built equal, entry for entry, reference_lists of the frame's OWN records
(download_frame: the f16 splats and the draw order) -- the rectangle of footprint.h restated in float64, entries in draw order, a
stable sort by tile id.  Nothing is compared with another device frame and nothing has a tolerance: a splat within rounding of a
tile boundary would be reported as undecided, and there is none.  The frames hold what random clouds do not put where it
matters: runs of visible splats with no tile in front of, inside and behind a slice (emit::slice_setup's LDS window of E + 2
offsets, and global memory beyond it), rectangles of more than 2 E tiles (several emit_start words from one splat), 65
binning-prefix workgroups of total 0 in a row (a look-back of two polls), every rectangle width up to 256 with k up to 65535
(emit::tile_of_rect's reciprocal division), one list over several sort tiles with every other range empty, entry counts at
sort-tile multiples, 16-bit and 32-bit tile ids, and frames that overflow their entry capacity.

  a. every pattern of the table in the default form (4x4 tiles, bin_request = 0)
  b. the forms: coarse lists (bin_request = 2), tile counts instead of packed rectangles (8256 x 96), 256 tiles on an axis
     (8192 x 64), the 4x2 and 2x2 tile shapes, one and two 6-bit sort passes (256 x 256, 288 x 256), the unfused tile sort
     (capacity 2^20) and WS_TILE_SORT=wide, each on five patterns
  c. one renderer, several frames: stale emit_start / offsets / status words, epochs, the ticket
  d. an overflowed frame keeps the first `capacity` entries in draw order
  e. the image of two of the frames against the float64 walk: the lists the blend consumes are the ones checked"""
import json
import os

import numpy as np
import pytest

import bin_patterns as bp
import blend_ref
from bin_patterns import E, P
from variants import exp_param

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3, 0.4)
REACHED = {}     # form -> what the reference says the device frames of that form reached (written out by the last test)


@pytest.fixture(scope="module")
def contexts(ws):
    """Contexts by configuration, made on first use: the binning tile and the sort's form are the context's."""
    made = {}

    def get(**cfg):
        key = tuple(sorted(cfg.items()))
        if key not in made:
            made[key] = ws.Context(0, ws.config_from_env({}, **cfg))
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _log2(tile):
    return tile[0].bit_length() - 1, tile[1].bit_length() - 1


def _shape_cfg(tile):
    return {"tile_qw": tile[0] // 8, "tile_qh": tile[1] // 8}


def _check(r, v, viewport, tile, form, name, capacity=None):
    """Everything the prepared frame of r says about its lists, against reference_lists of its own records.  capacity: the entry
    capacity the frame was given when it is expected to decide (None: the frame must not overflow)."""
    what = (form, name)
    fr = r.download_frame()
    bt = r.binning_tile()
    assert bt in (tile, (2 * tile[0], 2 * tile[1])), (what, bt)
    st = r.frame_stats()
    L = bp.reference_lists(fr, viewport, _log2(tile), bt != tile, count_cap=capacity)
    assert not L.undecided.any(), (what, "undecided", np.nonzero(L.undecided)[0][:5])
    assert st["num_visible"] == fr["num_visible"] == v, (what, st)
    bits, need = r.errors()
    if capacity is None or L.d <= capacity:
        assert st["overflow"] == 0 and bits == 0, (what, st, bits)
        assert st["num_tile_entries"] == L.d, (what, st, L.d)
    else:
        # (the frame's own flag: the sticky word of errors() is posted by the blend, and nothing has been rendered)
        assert st["overflow"] == 1 and bits & ~1 == 0, (what, st, bits)           # bit 0 alone: no look-back time-out
        assert st["tile_entries_capacity"] == capacity and st["num_tile_entries"] == capacity == L.d_kept, (what, st)
    assert need == L.d, (what, need, L.d)
    ll = r.tile_stats()["list_len"]
    assert len(ll) == L.ntiles, (what, len(ll), L.ntiles)
    bad = np.nonzero(ll != L.list_len)[0]
    assert len(bad) == 0, (what, "list_len", [(int(t), int(ll[t]), int(L.list_len[t])) for t in bad[:5]], _where(L, bad[:1]))
    begin, end, entries = r.tile_lists()
    assert len(begin) == len(end) == L.ntiles and len(entries) == L.d_kept, (what, len(begin), len(entries))
    assert np.array_equal(end.astype(np.int64) - begin, L.list_len), (what, "end - begin")
    some = L.list_len > 0
    run = np.cumsum(L.list_len) - L.list_len
    assert np.array_equal(begin[some], run[some]), (what, "begin is not the running sum in tile order")
    assert np.array_equal(begin, L.begin) and np.array_equal(end, L.end), (what, "ranges (an empty list is (0, 0))")
    if not np.array_equal(entries, L.entries):            # the lists lie one behind the other in tile order: name the first bad one
        e = int(np.nonzero(entries != L.entries)[0][0])
        t = int(np.searchsorted(np.cumsum(L.list_len), e, side="right"))
        raise AssertionError((what, f"tile {t} ({t % L.tiles_x}, {t // L.tiles_x}): list differs at its entry {e - int(run[t])}",
                              entries[begin[t]:end[t]][:16].tolist(), L.entries[begin[t]:end[t]][:16].tolist(), _where(L, [t])))
    for t in np.nonzero(some)[0][:: max(1, int(some.sum()) // 64)]:        # (and spelled out per tile, for a sample of them)
        assert np.array_equal(entries[begin[t]:end[t]], L.entries[L.begin[t]:L.end[t]]), (what, int(t))
    got = REACHED.setdefault(form, {"patterns": [], "frames": 0, "max_ns": 0, "max_slice_starts": 0, "max_zero_workgroups": 0,
                                    "max_entries": 0, "binning_tiles": []})
    got["frames"] += 1
    if name not in got["patterns"]:
        got["patterns"].append(name)
    got["max_ns"] = max(got["max_ns"], int(L.slices[:, 2].max()) if len(L.slices) else 0)
    got["max_slice_starts"] = max(got["max_slice_starts"], int(L.slice_starts.max()) if v else 0)
    got["max_zero_workgroups"] = max(got["max_zero_workgroups"], _longest_zero_run(L.wg_totals))
    got["max_entries"] = max(got["max_entries"], L.d)
    if list(bt) not in got["binning_tiles"]:
        got["binning_tiles"].append(list(bt))
    return L


def _longest_zero_run(totals):
    best = cur = 0
    for t in totals.tolist():
        cur = cur + 1 if t == 0 else 0
        best = max(best, cur)
    return best


def _where(L, tiles):
    """The slices and prefix workgroups that produced the first entries of the given tiles (for a failure's message)."""
    out = []
    for t in tiles:
        e = np.nonzero(L.keys == t)[0]
        if len(e):
            s = int(e[0]) // E
            pos = int(np.searchsorted(L.offsets, int(e[0]), side="right")) - 1
            out.append({"tile": int(t), "entry": int(e[0]), "slice": s, "slice (s_lo, s_hi, ns)": L.slices[s].tolist(), "position": pos,
                        "prefix workgroup": pos // P})
    return out


def _prepare_and_check(ws, ctx, p, form, capacity=None, set_capacity=None, expect_tile=None, cl=None):
    cl = cl or bp.cloud(ws, p)
    tile = ctx.tile_size()
    assert tile == p.tile, (tile, p.tile)
    pc = ws.PointCloud(ctx, cl.gpc)
    r = ws.GaussianRenderer(ctx, "rgba32float", bp.SH_DEG, False)
    try:
        if set_capacity is not None:
            r.set_tile_entry_capacity(set_capacity)
        r.prepare(pc, cl.args)
        if expect_tile is not None:
            assert r.binning_tile() == expect_tile, (form, p.name, r.binning_tile())
        return _check(r, p.v, p.viewport, tile, form, p.name, capacity=capacity)
    finally:
        r.close()
        pc.close()


# ---- a. every pattern of the table, default form -------------------------------------------------------------------------------
TABLE = bp.table()


@pytest.mark.parametrize("build", [b for _, b in TABLE], ids=[i for i, _ in TABLE])
def test_table_default_form(ws, contexts, build):
    p = build()
    ctx = contexts(bin_request=0, **_shape_cfg(p.tile))       # (widths: 16-px tiles, the 2x2 shape)
    form = "default" if p.tile == (32, 32) else "default/2x2"
    L = _prepare_and_check(ws, ctx, p, form, expect_tile=p.tile)
    # what the pattern is named for, on the DEVICE's frame (the numbers come from the reference offsets of the downloaded frame)
    if p.name.startswith("zero_run") and "lead" not in p.name:
        r = int(p.name[len("zero_run("):].split(",")[0])
        assert int(L.slices[:, 2].max()) == r + 2
    if p.name in ("empty_blocks", "one_per_block"):
        assert len(L.wg_totals) == 68 and L.slices[:, 2].max() > E + 2
    if p.name == "empty_blocks":
        assert _longest_zero_run(L.wg_totals) == 65
    if p.name.startswith("big(4096"):
        assert L.slice_starts.max() >= 2
    if p.name.startswith("widths"):
        assert L.counts.max() == 256 * (p.viewport[1] // 16)


# ---- b. the forms ------------------------------------------------------------------------------------------------------------
# id -> (context configuration, viewport of the patterns or None = the table's, tile in px, capacity request, binning tile)
FORMS = {
    "coarse": ({"bin_request": 2}, None, (32, 32), None, (64, 64)),
    "8256x96": ({"bin_request": 0}, (8256, 96), (32, 32), None, (32, 32)),
    "8192x64": ({"bin_request": 0}, (8192, 64), (32, 32), None, (32, 32)),
    "4x2": ({"bin_request": 0, "tile_qw": 4, "tile_qh": 2}, None, (32, 16), None, (32, 16)),
    "2x2": ({"bin_request": 0, "tile_qw": 2, "tile_qh": 2}, None, (16, 16), None, (16, 16)),
    "256x256": ({"bin_request": 0}, (256, 256), (32, 32), None, (32, 32)),
    "288x256": ({"bin_request": 0}, (288, 256), (32, 32), None, (32, 32)),
    "cap_2^20": ({"bin_request": 0}, None, (32, 32), 1 << 20, (32, 32)),
    "wide": ({"bin_request": 0, "exp_tile_sort_wide": 1}, None, (32, 32), None, (32, 32)),
}
FORM_PATTERNS = ("zero_run(E+1,inner)", "zero_run(3E+5,second_slice)", "big", "one_tile(last)", "mixed(0)")


@pytest.mark.parametrize("which", range(5), ids=FORM_PATTERNS)
@pytest.mark.parametrize("form", [exp_param(f) if f == "wide" else f for f in FORMS])
def test_forms(ws, contexts, form, which):
    cfg, viewport, tile, cap, bt = FORMS[form]
    p = bp.form_patterns(viewport or (640, 480), tile, big_viewport=viewport or bp.BIG_VIEWPORTS[0])[which]
    ctx = contexts(**cfg)
    L = _prepare_and_check(ws, ctx, p, form, set_capacity=cap, expect_tile=bt)
    tx, ty = p.grid
    if form == "coarse":
        assert L.ntiles == ((tx + 1) // 2) * ((ty + 1) // 2)
    if form == "8192x64":
        assert tx == 256 and (which != 2 or L.counts.max() == 512)          # an A of w = 256
    if which == 0:
        assert L.slices[:, 2].tolist() == [E + 3]
    if which == 1:
        assert L.slices[:, 2].tolist() == [E + 1, 3 * E + 7]


# ---- c. one renderer, several frames ---------------------------------------------------------------------------------------------
def test_many_frames_on_one_renderer(ws, contexts):
    """20 000 positions in five workgroups, then 68 workgroups of which 65 hold nothing, then one splat, then a frame that
    sees nothing, then rectangles of 4224 tiles at another viewport, then the first frame again: emit_start, the offsets and the
    status words keep what earlier frames left (they are never re-zeroed), the ticket and the counters are reused."""
    ctx = contexts(bin_request=0, tile_qw=4, tile_qh=4)
    tile = ctx.tile_size()
    r = ws.GaussianRenderer(ctx, "rgba32float", bp.SH_DEG, False)
    steps = [bp.mixed(0), bp.empty_blocks(), bp.dots(1), None, bp.big(bp.BIG_VIEWPORTS[1]), bp.mixed(0)]
    try:
        first = None
        for step, p in enumerate(steps):
            if p is None:                                                   # look away from the cloud of the step before
                cl = bp.cloud(ws, steps[step - 1])
                args, v, viewport, name = bp.look_away(ws, cl), 0, cl.viewport, "look_away"
            else:
                cl = bp.cloud(ws, p)
                args, v, viewport, name = cl.args, p.v, p.viewport, p.name
            pc = ws.PointCloud(ctx, cl.gpc)
            try:
                r.prepare(pc, args)
                L = _check(r, v, viewport, tile, "one renderer", f"{step}:{name}")
                if p is None:
                    assert L.d == 0 and not L.list_len.any()
                if step == 0:
                    first = L
                if step == len(steps) - 1:
                    assert np.array_equal(L.entries, first.entries) and np.array_equal(L.begin, first.begin)
            finally:
                pc.close()
    finally:
        r.close()


# ---- d. truncation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", ["D", "D-1", "2304+700"])
def test_overflowed_frame_keeps_the_first_entries(ws, contexts, capacity):
    """big(2048 x 1152): D = 3 x 2304 + 9.  A frame whose capacity is D is whole; with less it flags the overflow, reports D as
    its demand, and its lists are those of the first `capacity` entries in draw order (include/websplat.h,
    ws_renderer_set_tile_entry_capacity) -- the cut falls inside the third A, or inside the second one."""
    p = bp.big(bp.BIG_VIEWPORTS[0])
    d = 3 * 2304 + 9
    cap = {"D": d, "D-1": d - 1, "2304+700": 2304 + 700}[capacity]
    ctx = contexts(bin_request=0, tile_qw=4, tile_qh=4)
    L = _prepare_and_check(ws, ctx, p, "truncated", capacity=cap, set_capacity=cap)
    assert L.d == d and L.d_kept == cap
    if capacity == "2304+700":
        a = np.nonzero(p.kind == bp.A_)[0]
        assert L.offsets[a[1]] < cap < L.offsets[a[1]] + 2304
        assert (L.vals == a[2]).sum() == 0 and (L.vals == a[1]).sum() == cap - L.offsets[a[1]]


# ---- e. the image ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed(0)", "big"])
def test_image_of_the_checked_lists(ws, contexts, which):
    """render() once and compare with the float64 walk of the frame's own records over the background, under the project's 2e-4
    gate (blend_ref.GATE): the lists the blend consumes are the ones _check has just compared.  mixed at 288 x 256 (72 tiles);
    big at 2048 x 1152, of which the float64 walk covers the whole frame (12 records)."""
    p = bp.mixed(0, (288, 256)) if which == "mixed(0)" else bp.big(bp.BIG_VIEWPORTS[0])
    ctx = contexts(bin_request=0, tile_qw=4, tile_qh=4)
    cl = bp.cloud(ws, p)
    w, h = p.viewport
    pc = ws.PointCloud(ctx, cl.gpc)
    r = ws.GaussianRenderer(ctx, "rgba32float", bp.SH_DEG, False)
    try:
        r.prepare(pc, cl.args)
        _check(r, p.v, p.viewport, ctx.tile_size(), "image", p.name)
        fr = r.download_frame()
        r.render(pc, background=BG)
        img = r.download_target()
        assert r.errors()[0] == 0
    finally:
        r.close()
        pc.close()
    ref = blend_ref.reference(fr, None, w, h)
    want = blend_ref.over(ref, BG)
    decided = ~ref["undecided"]
    err = np.abs(img.astype(np.float64) - want).max(axis=2)
    print(f"{p.name}: max |device - float64| = {err[decided].max():.3g} over {int(decided.sum())} of {w * h} pixels; "
          f"T in [{ref['T'].min():.3g}, {ref['T'].max():.3g}]")
    assert decided.mean() > 0.98
    assert err[decided].max() <= blend_ref.GATE, (p.name, float(err[decided].max()))
    assert ref["T"].min() < 0.9                       # the splats are really in the image


# ---- what the device frames reached (keep this test last) --------------------------------------------------------------------------
def test_report_of_what_was_reached(ws, contexts):
    """Per form: the patterns run, the largest ns of a slice (beyond E + 2 = the offsets came from global memory), the most slice
    starts inside one splat, the longest run of prefix workgroups of total 0 -- from the reference offsets of the DOWNLOADED
    frames.  Written to binning_report.json in WEBSPLAT_REPORT_DIR (default: test_reports/ under the repository root).  Run
    alone, this test prepares the three frames it asserts on."""
    ctx = contexts(bin_request=0, tile_qw=4, tile_qh=4)
    if "default" not in REACHED:
        for p in (bp.zero_run(E + 1, "inner"), bp.big(bp.BIG_VIEWPORTS[1]), bp.empty_blocks()):
            _prepare_and_check(ws, ctx, p, "default")
    print(json.dumps(REACHED, indent=1))
    out = os.environ.get("WEBSPLAT_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "binning_report.json"), "w") as f:
        json.dump({"E": E, "P": P, "forms": REACHED}, f, indent=1)
    d = REACHED["default"]
    assert d["max_ns"] > E + 2                        # the global-offset path of emit::slice_setup
    assert d["max_slice_starts"] >= 2                 # a splat holding two or more slice starts
    assert d["max_zero_workgroups"] >= 65             # a look-back of two polls over zero aggregates
