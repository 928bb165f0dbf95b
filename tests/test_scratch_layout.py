"""CPU test of the renderer's scratch layout (web-splat_amd/csrc/frame_scratch.h): how many elements every per-frame array gets.
An array one element short shows up on the GPU only as a fault or a wrong frame at some odd size, so the sizes themselves are
checked here: a few lines of C++ against the header answer every request of an enumerated space; the expected sizes are
`parent_scratch` below, a transcription of the allocations as ws_api.cpp spelled them out before frame_scratch.h merged them
(renderer_ensure_scratch, alloc_sort_scratch and the three sites that allocate on first use), each cited by its line there.  The
plan of every request is tests/test_frame_plan.py's `parent_plan`."""
import itertools
import os
import subprocess

import pytest

from test_frame_plan import (BIN_AUTO, DEFAULTS, EMIT_TILE, PLAN, REQUEST, SORT_KPT_SMALL, SORT_SMALL_MAX, SORT_THREADS, SORT_TILE,
                             parent_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

# ws_internal.h of the parent
SPLAT_STRIDE, RADIX, BLEND_TIMING_WORDS = 20, 256, 16
SIZEOF_FRAME_COUNTERS = 128 + 16 * 16 * 4                                          # :104-134 (its static_assert)
SIZEOF_FRAME_ZERO = SIZEOF_FRAME_COUNTERS + 4 * 512 * 4 + 4 * RADIX * 4 + 9 * 16 * 4  # :138-144
SIZEOF_UINT2 = 8
FAT_STATUS_WORDS = 4 * 256 * RADIX  # experimental/sort_variants_host.hip fat_sort_status_words(); a plain request field here

SORT = ("cap", "rows", "tiles", "tiles_cap", "wide_bins", "sum_words", "wide_hist_words")
LAYOUT = ("splats", "points", "k1_status", "bin_status", "entries", "emit_start", "blend_order", "debug_consumed", "debug_walked", "zero") + \
         tuple("depth_" + f for f in SORT) + tuple("tiles_" + f for f in SORT) + ("fat_status", "depths", "debug_timing", "removal_base")
EXTRA = ("fat", "k1_blocks", "bin_blocks", "order_blocks", "fat_status_words")


def parent_sort_scratch(cap, wide_bins=0, rows=RADIX):
    """alloc_sort_scratch (ws_api.cpp:234-255) with own_alt = false, as the renderer called it."""
    tiles = max((cap + SORT_TILE - 1) // SORT_TILE, 1)                                     # :237-238
    small_n = min(cap, SORT_SMALL_MAX)                                                     # :244
    small_tiles = (small_n + SORT_THREADS * SORT_KPT_SMALL - 1) // (SORT_THREADS * SORT_KPT_SMALL)  # :245
    tiles_cap = max(small_tiles, tiles, 1)                                                 # :246
    sum_words = tiles_cap * rows                                                           # :247
    wide_hist = 0
    if wide_bins:                                                                          # :248-252
        sum_words = max(sum_words, tiles * wide_bins)
        wide_hist = wide_bins
    return (cap, rows, tiles, tiles_cap, wide_bins, sum_words, wide_hist)                  # :253 dmalloc(tile_sums, sum_words)


def parent_scratch(q):
    """The parent's allocations, line by line: the count each dmalloc / hipMalloc was given."""
    plan = dict(zip(PLAN, parent_plan(q)))
    n, cap, ntiles = q["num_points"], plan["entry_cap"], plan["ntiles"]
    s = {}
    np_ = n + 8                                               # renderer_ensure_scratch :346
    s["splats"] = np_ * SPLAT_STRIDE                          # :347
    s["points"] = np_                                         # :348-355 keys_a/b, vals_a/b, fpw_a/b, src_index, bin_offsets
    s["k1_status"] = q["k1_blocks"] + 1                       # :356-357 preprocess_blocks(n) + 1
    s["bin_status"] = q["bin_blocks"] + 1                     # :356, :358 bin_prefix_blocks(n) + 1
    s["entries"] = cap + 8                                    # :361-365 ekeys_a/b, evals_a/b
    s["emit_start"] = cap // EMIT_TILE + 4                    # :366
    s["blend_order"] = q["order_blocks"] + 8                  # :367 blend_order_blocks(tiles_x, tiles_y) + 8
    s["debug_consumed"] = ntiles                              # :368
    s["debug_walked"] = ntiles * 17                           # :369
    s["zero"] = SIZEOF_FRAME_ZERO + ntiles * SIZEOF_UINT2     # :371 (bytes)
    depth = parent_sort_scratch(n if n else 1, 0, 512)        # :376
    tiles = parent_sort_scratch(cap, plan["wide_bins"])       # :381
    s.update({"depth_" + f: v for f, v in zip(SORT, depth)})
    s.update({"tiles_" + f: v for f, v in zip(SORT, tiles)})
    s["fat_status"] = q["fat_status_words"] if q["fat"] else 0  # :385-388 (DS_ONESWEEP | DS_COOP only)
    s["depths"] = n + 8                                       # prepare_setup :1249
    s["debug_timing"] = ntiles * 16 * BLEND_TIMING_WORDS      # render_frame :1515-1519
    s["removal_base"] = q["vw"] * q["vh"]                     # base_plane :2253-2259
    return tuple(s[f] for f in LAYOUT)


POINTS = (1, 7, 1023, 1024, 1025, 3000, 1 << 21, (1 << 21) + 1)  # (the last two straddle SORT_SMALL_MAX)
VIEWPORTS = ((1, 1), (16, 16), (33, 17), (320, 240), (1920, 1080), (3840, 2160), (8200, 16))  # (the last: more than 256 tiles on an axis)
SHAPES = ((2, 2), (4, 2), (4, 4))
CAPACITIES = (0, 1000, 1 << 24)


def request_space():
    for n, (vw, vh), (qw, qh), cap, wide, fat, capture in itertools.product(POINTS, VIEWPORTS, SHAPES, CAPACITIES, (0, 1), (0, 1), (0, 1)):
        q = dict(DEFAULTS, bin_request=BIN_AUTO, num_points=n, vw=vw, vh=vh, tile_qw=qw, tile_qh=qh, entry_cap_request=cap,
                 tile_sort_wide=wide, capture=capture, fat=fat)
        # the block counts live next to their kernels and arrive as plain numbers: any values with the kernels' growth will do
        q.update(k1_blocks=-(-n // 2048), bin_blocks=-(-n // 1024), order_blocks=-(-vw // (8 * qw)) * -(-vh // (8 * qh)),
                 fat_status_words=FAT_STATUS_WORDS)
        yield q


PROBE = r"""
#include <stdio.h>
#include "frame_scratch.h"
using namespace ws;
int ws::device_alloc(void**, size_t) { return WS_ERR_OOM; }  // (the layout allocates nothing)
void ws::device_free(void*) {}
static void print_sort(const SortShape& s) {
    printf(" %u %u %u %u %u %zu %zu", s.cap, s.rows, s.tiles, s.tiles_cap, s.wide_bins, s.sum_words, s.wide_hist_words);
}
int main() {
    printf("%zu %zu %u %d\n", sizeof(FrameZero), sizeof(uint2), SPLAT_STRIDE, BLEND_TIMING_WORDS);
    for (;;) {
        FramePlanRequest p{};
        ScratchRequest q{};
        int wide, capture, fat;
        unsigned long long cap, fat_words;
        if (scanf("%u %u %d %d %d %d %d %d %d %d %u %u %u %d %llu %u %d %u %d %d %u %u %u %llu", &p.tile_qw, &p.tile_qh, &p.footprint, &wide,
                  &p.bin_request, &p.blend_tpw_log2, &p.blend_split, &p.num_cus, &p.depth_digit_bits, &p.depth_skip_top, &p.num_points,
                  &p.viewport[0], &p.viewport[1], &capture, &cap, &p.demand, &p.order_mode, &p.span_class, &p.graph_depth_bits, &fat,
                  &q.k1_blocks, &q.bin_blocks, &q.order_blocks, &fat_words) != 24)
            break;
        p.tile_sort_wide = wide != 0, p.capture = capture != 0, p.entry_cap_request = cap;
        q.plan = frame_plan(p), q.num_points = p.num_points, q.vw = p.viewport[0], q.vh = p.viewport[1];
        q.fat_depth_sort = fat != 0, q.fat_status_words = fat_words;
        const ScratchLayout l = scratch_layout(q);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", l.splats, l.points, l.k1_status, l.bin_status, l.entries, l.emit_start, l.blend_order,
               l.debug_consumed, l.debug_walked, l.zero);
        print_sort(l.sort_depth);
        print_sort(l.sort_tiles);
        printf(" %zu %zu %zu %zu\n", l.fat_status, l.depths, l.debug_timing, l.removal_base);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("scratch_layout")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-isystem", os.path.join(ROCM, "include"), str(src), "-o", str(exe)], check=True)
    space = list(request_space())
    lines = [" ".join(str(q[f]) for f in REQUEST + EXTRA) for q in space]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(space) + 1
    return tuple(map(int, out[0].split())), space, [tuple(map(int, line.split())) for line in out[1:]]


def test_the_constants_are_the_parents(layouts):
    assert layouts[0] == (SIZEOF_FRAME_ZERO, SIZEOF_UINT2, SPLAT_STRIDE, BLEND_TIMING_WORDS)


def test_every_request_gets_the_parents_sizes(layouts):
    _, space, got = layouts
    assert len(space) == len(POINTS) * len(VIEWPORTS) * len(SHAPES) * len(CAPACITIES) * 8
    for q, g in zip(space, got):
        e = parent_scratch(q)
        assert g == e, (q, {f: (a, b) for f, a, b in zip(LAYOUT, g, e) if a != b})
    # the space reaches both sides of what the sizes turn on
    seen = [dict(zip(LAYOUT, g)) for g in got]
    assert {s["tiles_wide_bins"] != 0 for s in seen} == {False, True}             # the single-pass sort's rows, granted and not
    assert any(s["tiles_sum_words"] == s["tiles_tiles"] * s["tiles_wide_bins"] > s["tiles_tiles_cap"] * RADIX for s in seen)
    assert {s["fat_status"] for s in seen} == {0, FAT_STATUS_WORDS}
    assert {s["depth_tiles_cap"] > s["depth_tiles"] for s in seen} == {False, True}   # 1024-key tiles up to SORT_SMALL_MAX, 2048 above
    assert {s["entries"] - 8 for s in seen} >= {1000, 1 << 24, 8 << 20}              # explicit capacities and the automatic floor
    assert any(s["entries"] - 8 > 8 << 20 and q["entry_cap_request"] == 0 for q, s in zip(space, seen))  # ... and above it
    assert min(s["debug_consumed"] for s in seen) == 1 and max(s["debug_consumed"] for s in seen) == 240 * 135
