"""CPU test of the frame's plan (web-splat_amd/csrc/frame_plan.h): how a frame is laid out and which launch sequence it gets.  A
one-off at a tile-count boundary shows up on the GPU only as a wrong or faulting frame (the scratch's count rows, the emit kernel's
pitch and the sort's digit width have to coincide), so the decisions themselves are checked here: a few lines of C++ against the
header (plain C++, no HIP) answer every request of an enumerated space; the expected plan of every request is `parent_plan` below,
a transcription of the rules as they stood in ws_api.cpp before frame_plan.h merged them (renderer_ensure_scratch,
alloc_sort_scratch, prepare_setup, enqueue_frame, render_frame, depth_digit_bits), each cited where it is transcribed."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")

# ws_internal.h of the parent
QUAD, RADIX_BITS = 8, 8
SORT_THREADS, SORT_KPT, SORT_KPT_SMALL, SORT_SMALL_MAX = 256, 8, 4, 2 << 20
SORT_TILE = EMIT_TILE = SORT_THREADS * SORT_KPT
TILE_SORT_WIDE_MAX_BINS = 1 << 11
FP_RECT_PACKED, FP_RECT_COUNT, FP_ELLIPSE = 0, 1, 2
RECT_PACKED_MAX_TILES_PER_AXIS, MAX_TILES_PER_AXIS = 256, 65535
BIN_NEVER, BIN_AUTO, BIN_ALWAYS = 0, 1, 2
DEPTH_DIGIT_BITS_DEFAULT, DEPTH_DIGIT_BITS_ADAPTIVE = 8, 1

REQUEST = ("tile_qw", "tile_qh", "footprint", "tile_sort_wide", "bin_request", "blend_tpw_log2", "blend_split", "num_cus",
           "depth_digit_bits", "depth_skip_top", "num_points", "vw", "vh", "capture", "entry_cap_request", "demand", "order_mode",
           "span_class", "graph_depth_bits")
PLAN = ("tile_w_log2", "tile_h_log2", "tiles_x", "tiles_y", "ntiles", "footprint_mode", "bin_request", "entry_cap", "wide_bins",
        "wide_sort", "wide_bits", "fused_hist", "tile_bits", "digit_bits", "tile_hist_mask", "key16", "depth_digit_bits", "blend_order",
        "split_wanted")
DEFAULTS = dict(footprint=FP_RECT_PACKED, tile_sort_wide=0, bin_request=BIN_AUTO, blend_tpw_log2=-1, blend_split=-1, num_cus=256,
                depth_digit_bits=0, depth_skip_top=1, num_points=3000, capture=0, entry_cap_request=0, demand=0, order_mode=1,
                span_class=0, graph_depth_bits=0)


def sort_tile_size(n):
    return SORT_THREADS * SORT_KPT_SMALL if n <= SORT_SMALL_MAX else SORT_TILE  # sort.hip sort_tile_size


def parent_plan(q):
    """The parent's rules, line by line.  (With a mailbox, the parent read span_class 0 -- nothing reported yet -- as 8 bits and
    took the default without one; the default IS 8, so one request field serves both readings.)"""
    p = {}
    vw, vh, n = q["vw"], q["vh"], q["num_points"]
    # renderer_ensure_scratch: the entry capacity
    want = q["entry_cap_request"]
    if want == 0:
        mpix = float(vw) * float(vh) / (1200.0 * 800.0)
        want = max(8 << 20, int(4.0 * float(n) * max(1.0, mpix)))
        if q["demand"]:
            want = max(want, q["demand"] + q["demand"] // 4 + 4096)
    want = min(want, (1 << 30) - 2 * EMIT_TILE)
    p["entry_cap"] = cap = want & 0xFFFFFFFF
    # renderer_ensure_scratch: the tile grid
    tile_w, tile_h = QUAD * q["tile_qw"], QUAD * q["tile_qh"]
    p["tiles_x"], p["tiles_y"] = (vw + tile_w - 1) // tile_w, (vh + tile_h - 1) // tile_h
    p["ntiles"] = ntiles = (p["tiles_x"] * p["tiles_y"]) & 0xFFFFFFFF
    # renderer_ensure_scratch: the single-pass sort's bins, as asked of alloc_sort_scratch ...
    asked = 0
    if q["tile_sort_wide"] and 64 < ntiles <= TILE_SORT_WIDE_MAX_BINS and sort_tile_size(cap) == EMIT_TILE:
        asked = 128
        while asked < ntiles:
            asked <<= 1
    # ... and as alloc_sort_scratch granted them (SortScratch::wide_bins)
    sc_tiles = max((cap + SORT_TILE - 1) // SORT_TILE, 1)
    sc_wide_bins = asked if asked and sc_tiles * asked * 4 <= 1 << 30 else 0
    p["wide_bins"] = sc_wide_bins
    # prepare_setup: tile size, footprint form, K1's binning request
    p["tile_w_log2"], p["tile_h_log2"] = (5 if q["tile_qw"] == 4 else 4), (5 if q["tile_qh"] == 4 else 4)
    p["footprint_mode"] = FP_ELLIPSE if q["footprint"] == FP_ELLIPSE else (
        FP_RECT_COUNT if p["tiles_x"] > RECT_PACKED_MAX_TILES_PER_AXIS or p["tiles_y"] > RECT_PACKED_MAX_TILES_PER_AXIS else FP_RECT_PACKED)
    shape44 = q["tile_qw"] == 4 and q["tile_qh"] == 4
    p["bin_request"] = q["bin_request"] if p["footprint_mode"] == FP_RECT_PACKED and not q["capture"] and shape44 else BIN_NEVER
    # enqueue_frame: the depth sort's digit width
    dbits = q["depth_digit_bits"]
    if dbits not in (8, 9):
        dbits = DEPTH_DIGIT_BITS_DEFAULT
        if DEPTH_DIGIT_BITS_ADAPTIVE and q["depth_skip_top"] and q["graph_depth_bits"] == 0:
            dbits = 9 if q["span_class"] == 2 else 8
    if q["graph_depth_bits"]:
        dbits = q["graph_depth_bits"]
    p["depth_digit_bits"] = dbits
    # enqueue_frame: the tile-id sort
    p["fused_hist"] = fused = int(sort_tile_size(cap) == EMIT_TILE)
    tile_bits = 1
    while (1 << tile_bits) < ntiles:
        tile_bits += 1
    tile_passes = (tile_bits + RADIX_BITS - 1) // RADIX_BITS
    digit_bits = (tile_bits + tile_passes - 1) // tile_passes
    if tile_passes == 1 and ntiles > 64:
        digit_bits = 6
    digit_bits = max(digit_bits, 6)
    p["tile_bits"], p["digit_bits"], p["tile_hist_mask"] = tile_bits, digit_bits, (1 << digit_bits) - 1
    p["wide_sort"] = int(bool(fused and sc_wide_bins >= ntiles and ntiles > 64 and sc_wide_bins != 0))
    wide_bits = 7
    while (1 << wide_bits) < ntiles:
        wide_bits += 1
    p["wide_bits"] = wide_bits if p["wide_sort"] else 0  # (read by the single-pass launch only)
    p["key16"] = int(ntiles < 65535)
    # enqueue_frame: the order table
    p["blend_order"] = q["order_mode"] if q["order_mode"] and shape44 and ntiles <= 4096 and q["blend_tpw_log2"] <= 0 else 0
    # render_frame: the split
    p["split_wanted"] = int(q["blend_split"] != 0 if q["blend_split"] >= 0 else ntiles < 2 * q["num_cus"])
    return tuple(p[f] for f in PLAN)


def parent_viewport_ok(vw, vh, qw, qh):  # prepare_setup
    return not (vw == 0 or vh == 0 or vw > MAX_TILES_PER_AXIS * QUAD * qw or vh > MAX_TILES_PER_AXIS * QUAD * qh or
                vw > 1 << 24 or vh > 1 << 24)


SHAPES = ((2, 2), (4, 2), (4, 4))
# tile grids: the tile counts at which a rule changes, both footprint forms' sides (256 / 257 tiles on an axis), more than 2^24
# tiles, and the counts the header's comments name (3750, 8160, 32400 tiles)
GRIDS = ((1, 1), (2, 1), (8, 6), (8, 8), (13, 5), (16, 8), (43, 3), (16, 16), (257, 1), (64, 32), (683, 3), (64, 64), (241, 17),
         (434, 151), (257, 255), (65535, 1), (256, 256), (65535, 300), (256, 1), (1, 256), (1, 257), (75, 50), (120, 68), (240, 135))
assert sorted(x * y for x, y in GRIDS[:18]) == sorted([1, 2, 48, 64, 65, 128, 129, 256, 257, 2048, 2049, 4096, 4097, 65534, 65535, 65535,
                                                       65536, 65535 * 300])
PIXELS = ((16, 16), (1200, 800), (1920, 1080), (4096, 4096))
# the capacity: explicit requests on both sides of SORT_SMALL_MAX and beyond the 2^30 clamp; automatic at every point count, without
# a demand, with one above the formula's floor, and with one the clamp cuts
CAPACITIES = [dict(entry_cap_request=c) for c in (1000, SORT_SMALL_MAX, SORT_SMALL_MAX + 1, 1 << 31)] + \
             [dict(num_points=n, demand=d) for n in (0, 1, 3000, 1_000_000, 100_000_000) for d in (0, 20_000_000, 900_000_000)]


def viewports(qw, qh):
    """The smallest viewport of every grid at this tile shape (one pixel into the last tile: the ceiling), and the pixel sizes."""
    return [((x - 1) * QUAD * qw + 1, (y - 1) * QUAD * qh + 1) for x, y in GRIDS] + list(PIXELS)


def request_space():
    def product(**dims):
        for values in itertools.product(*dims.values()):
            yield dict(zip(dims, values))
    for qw, qh in SHAPES:
        for vw, vh in viewports(qw, qh):
            base = dict(DEFAULTS, tile_qw=qw, tile_qh=qh, vw=vw, vh=vh)
            # layout: capacity x single-pass sort x footprint x capture x binning request
            for cap in CAPACITIES:
                for d in product(tile_sort_wide=(0, 1), footprint=(FP_RECT_PACKED, FP_ELLIPSE), capture=(0, 1),
                                 bin_request=(BIN_NEVER, BIN_AUTO, BIN_ALWAYS)):
                    yield dict(base, **cap, **d)
            # the blend's order table and split
            for d in product(order_mode=(0, 1, 2), blend_tpw_log2=(-1, 0, 2), blend_split=(-1, 0, 1), tile_sort_wide=(0, 1)):
                yield dict(base, **d)
            # the depth sort's digit width
            for d in product(depth_digit_bits=(0, 8, 9, 7), span_class=(0, 1, 2), graph_depth_bits=(0, 8, 9), depth_skip_top=(0, 1)):
                yield dict(base, **d)


PROBE = r"""
#include <stdio.h>
#include "frame_plan.h"
using namespace ws;
int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'v') {  // frame_viewport_ok
            unsigned vw, vh, qw, qh;
            if (scanf("%u %u %u %u", &vw, &vh, &qw, &qh) != 4) return 1;
            printf("%d\n", frame_viewport_ok(vw, vh, qw, qh) ? 1 : 0);
        } else if (kind == 'd') {  // the stand-alone sorter's digit width
            int forced;
            if (scanf("%d", &forced) != 1) return 1;
            printf("%d\n", depth_sort_digit_bits(forced, false, 0u, 0));
        } else {
            FramePlanRequest q{};
            int wide, capture;
            unsigned long long cap;
            if (scanf("%u %u %d %d %d %d %d %d %d %d %u %u %u %d %llu %u %d %u %d", &q.tile_qw, &q.tile_qh, &q.footprint, &wide, &q.bin_request,
                      &q.blend_tpw_log2, &q.blend_split, &q.num_cus, &q.depth_digit_bits, &q.depth_skip_top, &q.num_points, &q.viewport[0],
                      &q.viewport[1], &capture, &cap, &q.demand, &q.order_mode, &q.span_class, &q.graph_depth_bits) != 19)
                return 1;
            q.tile_sort_wide = wide != 0, q.capture = capture != 0, q.entry_cap_request = cap;
            const FramePlan p = frame_plan(q);
            printf("%u %u %u %u %u %d %u %u %u %d %d %d %d %d %u %d %d %d %d\n", p.tile_w_log2, p.tile_h_log2, p.tiles_x, p.tiles_y, p.ntiles,
                   p.footprint_mode, p.bin_request, p.entry_cap, p.wide_bins, (int)p.wide_sort(), p.wide_bits(), (int)p.fused_hist, p.tile_bits,
                   p.digit_bits, p.tile_hist_mask, (int)p.key16, p.depth_digit_bits, p.blend_order, (int)p.split_wanted);
        }
    }
    // the plan is a constant expression: usable in static_asserts next to the kernels
    constexpr FramePlanRequest hd{4, 4, 0, false, 1, -1, -1, 256, 0, 1, 1000000u, {1920u, 1080u}, false, 0, 0u, 1, 0u, 0};
    static_assert(frame_plan(hd).ntiles == 60u * 34u && frame_plan(hd).tile_bits == 11 && frame_plan(hd).digit_bits == 6, "hd1m");
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [tuple(map(int, line.split())) for line in out]
    return ask


@pytest.fixture(scope="module")
def plans(probe):
    space = list(request_space())
    got = probe(["p " + " ".join(str(q[f]) for f in REQUEST) for q in space])
    return space, got


def test_every_request_gets_the_parents_plan(plans):
    space, got = plans
    assert len(space) == len(SHAPES) * (len(GRIDS) + len(PIXELS)) * (len(CAPACITIES) * 24 + 54 + 72)
    for q, g in zip(space, got):
        e = parent_plan(q)
        assert g == e, (q, {f: (a, b) for f, a, b in zip(PLAN, g, e) if a != b})
    # every boundary is in the space, on both sides
    seen = [dict(zip(PLAN, g)) for g in got]
    for shape in SHAPES:
        counts = {p["ntiles"] for q, p in zip(space, seen) if (q["tile_qw"], q["tile_qh"]) == shape}
        assert counts >= {1, 2, 48, 64, 65, 128, 129, 256, 257, 2048, 2049, 4096, 4097, 65534, 65535, 65536, 65535 * 300}
    for field, values in (("footprint_mode", {0, 1, 2}), ("bin_request", {0, 1, 2}), ("wide_sort", {0, 1}), ("fused_hist", {0, 1}),
                          ("key16", {0, 1}), ("digit_bits", {6, 7, 8}), ("depth_digit_bits", {8, 9}), ("blend_order", {0, 1, 2}),
                          ("split_wanted", {0, 1}), ("wide_bins", {0, 128, 256, 512, 1024, 2048})):
        assert {p[field] for p in seen} == values, field
    caps = {p["entry_cap"] for p in seen}
    assert {1000, SORT_SMALL_MAX, SORT_SMALL_MAX + 1, 8 << 20, (1 << 30) - 2 * EMIT_TILE, 20_000_000 + 5_000_000 + 4096} <= caps
    # asked for but not granted: count rows beyond 1 GiB
    assert any(q["tile_sort_wide"] and 64 < p["ntiles"] <= 2048 and p["fused_hist"] and not p["wide_sort"] for q, p in zip(space, seen))


def test_the_plan_is_consistent_everywhere(plans):
    """What the parent's scattered copies only implied: the scratch's rows, the emit kernel's pitch and the sorts' widths coincide."""
    space, got = plans
    for q, g in zip(space, got):
        p = dict(zip(PLAN, g))
        if p["wide_sort"]:
            assert p["key16"] and p["fused_hist"], q
            assert (1 << p["wide_bits"]) == p["wide_bins"] >= p["ntiles"] and p["wide_bins"] <= TILE_SORT_WIDE_MAX_BINS, q
            assert -(-p["entry_cap"] // SORT_TILE) * p["wide_bins"] * 4 <= 1 << 30, q
        else:
            assert p["wide_bins"] == 0, q
        if p["key16"]:
            assert p["tile_bits"] <= 16, q
        assert p["ntiles"] <= 1 << p["tile_bits"], q
        assert 6 <= p["digit_bits"] <= 8, q
        assert -(-p["tile_bits"] // p["digit_bits"]) <= 4, q
        assert p["tile_hist_mask"] == (1 << p["digit_bits"]) - 1, q
        assert p["fused_hist"] == (p["entry_cap"] > SORT_SMALL_MAX), q
        assert p["entry_cap"] <= (1 << 30) - 2 * EMIT_TILE, q
        assert p["bin_request"] == BIN_NEVER or p["footprint_mode"] == FP_RECT_PACKED, q


def test_fixed_points_of_the_tile_sort(plans):
    """The figures the header's comments state."""
    space, got = plans
    by_tiles = {}
    for q, g in zip(space, got):
        p = dict(zip(PLAN, g))
        by_tiles.setdefault(p["ntiles"], set()).add((p["tile_bits"], p["digit_bits"], p["key16"]))

    def passes(bits, digit):
        return -(-bits // digit)

    assert by_tiles[3750] == {(12, 6, 1)} and by_tiles[8160] == {(13, 7, 1)} and by_tiles[32400] == {(15, 8, 1)}
    assert by_tiles[48] == {(6, 6, 1)}                                              # one 6-bit pass
    assert by_tiles[64] == {(6, 6, 1)}
    for n in (65, 128, 129, 256):                                                   # two 6-bit passes
        (bits, digit, key16), = by_tiles[n]
        assert digit == 6 and passes(bits, digit) == 2 and key16
    assert by_tiles[65534] == {(16, 8, 1)} and by_tiles[65535] == {(16, 8, 0)}
    assert by_tiles[65536] == {(16, 8, 0)}                                          # 32-bit ids, two 8-bit passes
    (bits, digit, key16), = by_tiles[65535 * 300]
    assert bits == 25 and passes(bits, digit) == 4 and not key16


def test_viewports_refused_as_prepare_refused_them(probe):
    cases = []
    for qw, qh in SHAPES:
        limit_w, limit_h = MAX_TILES_PER_AXIS * QUAD * qw, MAX_TILES_PER_AXIS * QUAD * qh
        for vw, vh in ((0, 600), (800, 0), (0, 0), (1, 1), (800, 600), (limit_w, 32), (limit_w + 1, 32), (32, limit_h), (32, limit_h + 1),
                       (limit_w, limit_h), (1 << 24, 32), ((1 << 24) + 1, 32), (32, 1 << 24), (32, (1 << 24) + 1), (0xFFFFFFFF, 32)):
            cases.append((vw, vh, qw, qh))
    # the 2^24 bound on its own, at a tile shape (not one the library offers) whose tile limit lies above it
    cases += [(1 << 24, 32, 64, 64), ((1 << 24) + 1, 32, 64, 64), (32, (1 << 24) + 1, 64, 64)]
    got = probe(["v %d %d %d %d" % c for c in cases])
    for c, (g,) in zip(cases, got):
        assert bool(g) == parent_viewport_ok(*c), c
    assert {g for (g,) in got} == {0, 1}


def test_the_stand_alone_sorter_keeps_its_digit_width(probe):
    """ws_sorter_sort_depth asks the frame's rule without a span class or a graph; the parent's depth_digit_bits() gave it
    9 for 9, 8 for 8, else the default."""
    forced = (0, 8, 9, 7)
    assert [g for (g,) in probe(["d %d" % f for f in forced])] == [9 if f == 9 else (8 if f == 8 else DEPTH_DIGIT_BITS_DEFAULT) for f in forced]
