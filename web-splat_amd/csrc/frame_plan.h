// frame_plan.h -- how one frame is laid out and which launch sequence it gets: the tile grid, the footprint form, the entry
// capacity, the tile-id sort's shape, the depth sort's digit width, the blend's order table and split.  Every rule is a pure
// function of the context's switches, the point count, the viewport and the capacity request, stated ONCE here.  Plain C++ (no
// HIP include): api_renderer.cpp asks frame_plan() once per prepare(), sizes the scratch by it (frame_scratch.h), fills the kernels'
// parameter blocks and the sort jobs from the one answer; a CPU test (tests/test_frame_plan.py) enumerates it at every boundary.
#pragma once

#include <stdint.h>

#include "websplat.h"

namespace ws {

// ---- geometry of the rasteriser ----------------------------------------------------------------
// Binning tiles are QW x QH quadrants of 8x8 pixels (one wave each): 2x2 = the north star's 16x16 tile; 4x2 / 4x4
// bin two / four such tiles into one list (ws_context::tile_qw/qh, WS_TILE_SHAPE).  Default 4x4, by measurement:
// a 24-px splat touches 8.3 16x16 tiles but 3.7 32x32 ones, so the (tile, splat) entry list -- emit, tile sort,
// gather -- shrinks 2.2x while the per-quadrant compositing work is unchanged.
constexpr int QUAD = 8;

#ifndef WS_DEPTH_DIGIT_BITS_DEFAULT
#define WS_DEPTH_DIGIT_BITS_DEFAULT 8
#endif
#ifndef WS_DEPTH_DIGIT_BITS_ADAPTIVE   // 1: a renderer picks 8 or 9 bits per frame from its previous frame's key range (depth_sort_digit_bits)
#define WS_DEPTH_DIGIT_BITS_ADAPTIVE 1
#endif
constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;

// ---- sort ---------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 256;
#ifndef WS_SORT_KPT
#define WS_SORT_KPT 8
#endif
constexpr int SORT_KPT = WS_SORT_KPT;                 // keys per thread
constexpr int SORT_TILE = SORT_THREADS * SORT_KPT;    // keys per work tile
constexpr int SORT_KPT_SMALL = 4;                     // small inputs: 1024-key tiles -> 4x the workgroups
#ifndef WS_SORT_SMALL_MAX
#define WS_SORT_SMALL_MAX (2u << 20)
#endif
constexpr uint32_t SORT_SMALL_MAX = WS_SORT_SMALL_MAX;  // host-side bound n up to which the small tile is used
// tile size the scan path (the production sort) uses for bound n
constexpr uint32_t sort_tile_size(uint32_t n) { return n <= SORT_SMALL_MAX ? (uint32_t)(SORT_THREADS * SORT_KPT_SMALL) : (uint32_t)SORT_TILE; }
constexpr int EMIT_TILE = SORT_TILE;  // tile entries produced per workgroup of the emit kernel (= the sort's tile)

// Single-pass tile-id sort (launch_tile_sort_wide): the whole tile id is ONE digit of up to 11 bits.
constexpr int TILE_SORT_WIDE_MAX_BITS = 11;
constexpr int TILE_SORT_WIDE_MAX_BINS = 1 << TILE_SORT_WIDE_MAX_BITS;

// ---- binning footprint of a splat: the companion value of the depth sort ----------------------------------------
// K1 stores one 32-bit word per visible splat that says which binning tiles the splat is listed in; it rides through the
// depth sort with the splat index (sort.hip), so the binning prefix streams it in draw order.  Three forms:
//   FP_RECT_PACKED (default)  the bounding rectangle of the kept ellipse, x0 | y0 << 8 | (w - 1) << 16 | (h - 1) << 24
//                  in binning tiles: at most 256 tiles per axis (8192 px at the default 32-px tile); RECT_EMPTY = no
//                  tile.  k_bin_emit derives a tile from the word alone.
//   FP_RECT_COUNT  the NUMBER of tiles of the same rectangle; k_bin_emit re-derives the rectangle from the 12 geometry
//                  bytes of the Splat record (footprint.h).  Taken automatically for viewports beyond 256 tiles per axis:
//                  any target the reference can create (it asks for the adapter's own max_texture_dimension_2d,
//                  src/lib.rs:99-110) is accepted, at the price of a slower emit kernel.
//   FP_ELLIPSE     the number of tiles the kept ELLIPSE reaches (per tile row the exact column span, footprint.h):
//                  15 % fewer entries on the 1 M / 1080p scene, but the span arithmetic costs more VALU time in K1 and
//                  k_bin_emit than the entries cost downstream (profiles/r03/footprint_*) -- WS_FOOTPRINT=ellipse.
enum FootprintMode { FP_RECT_PACKED = 0, FP_RECT_COUNT = 1, FP_ELLIPSE = 2 };
constexpr uint32_t RECT_PACKED_MAX_TILES_PER_AXIS = 256u;
constexpr uint32_t MAX_TILES_PER_AXIS = 65535u;  // tile coordinates are 16-bit (the blend packs tx | ty << 16)

// ---- binning granularity, decided PER FRAME ON THE DEVICE -----------------------------------------------------------
// The blend composites 32x32-px tiles (default shape).  Binning may use those tiles, or 2 x 2 blocks of them (64x64 px):
// four blend workgroups then share one binned list -- half the (tile, splat) entries to emit and sort when splats span
// several tiles, at the price of every entry being staged by up to four workgroups.  Measured (profiles/r03/bin64_*):
// +16..+20 % frames/s where the rectangles shrink 2.07x (hd1m, c4), +3..+5 % at 1.75x (c2), -14 % / -23 % at 1.14x / 1.10x
// (c5, c3: pixel-sized splats); an N x resolution sweep (profiles/r03/sweep_bin_auto_v24.json) has 64 px ahead (+1..+63 %) at
// all ratios 1.75..2.63 and by +4 % on average (-3..+13 %) at 1.53: the threshold sits just below the smallest ratio measured to win.  K1 sums both tile counts while it writes the rectangles; the binning prefix derives
// the decision from the two sums (a pure function of the frame: ranks and renderers agree), no host round trip.
enum BinRequest { BIN_NEVER = 0, BIN_AUTO = 1, BIN_ALWAYS = 2 };

// ---- the request: what the decisions read, and nothing else -------------------------------------------------------------
struct FramePlanRequest {
    // the context's switches (ws_context)
    uint32_t tile_qw, tile_qh;  // quadrants per binning tile: 2x2, 4x2 or 4x4
    int footprint;              // FP_ELLIPSE: WS_FOOTPRINT=ellipse; anything else: the rectangle, in the form the tile grid allows
    bool tile_sort_wide;        // WS_TILE_SORT=wide
    int bin_request;            // BinRequest for frames that can use coarse binning
    int blend_tpw_log2;         // tiles per blend workgroup = 2^n; -1 = automatic
    int blend_split;            // 4x4 tiles composited as two 4x2 halves: 0 / 1, -1 = automatic
    int num_cus;
    int depth_digit_bits;       // 8 / 9 force the depth sort's digit width, anything else: the default, or per frame
    int depth_skip_top;         // the depth sort may skip its last pass (the adaptive digit width needs the key range it reports)
    // the frame
    uint32_t num_points;
    uint32_t viewport[2];       // (frame_viewport_ok)
    bool capture;               // the renderer keeps per-tile debug words: parity tooling reads the blend's own tiles back
    // the capacity
    uint64_t entry_cap_request; // ws_renderer_set_tile_entry_capacity; 0 = automatic
    uint32_t demand;            // automatic: the largest tile-entry demand an overflowed frame of this scene and viewport left (0 = none)
    // the per-frame inputs
    int order_mode;             // decide_blend_order(): 0 = image order, 1 = longest list first, 2 / 3 the measured experiments
    uint32_t span_class;        // FrameCounters::depth_span_class of the renderer's last started frame (0 = none known)
    int graph_depth_bits;       // != 0: a captured frame graph is valid, and keeps the width it was captured with
};

// Tile coordinates are 16-bit: 65535 binning tiles per axis, i.e. any target the reference can create (it asks for the
// adapter's own max_texture_dimension_2d, src/lib.rs:99-110: 16384 or 32768 on today's adapters).  Pixel coordinates are
// converted through f32 (exact below 2^24).
constexpr bool frame_viewport_ok(uint32_t vw, uint32_t vh, uint32_t tile_qw, uint32_t tile_qh) {
    return vw != 0 && vh != 0 && (uint64_t)vw <= (uint64_t)MAX_TILES_PER_AXIS * QUAD * tile_qw &&
           (uint64_t)vh <= (uint64_t)MAX_TILES_PER_AXIS * QUAD * tile_qh && vw <= (1u << 24) && vh <= (1u << 24);
}

// Digit width of a depth sort, for the frame's sort and the stand-alone sorter's (which knows no span class and no graph).
// Three 8-bit passes when the renderer's previous frame says its keys span < 2^24 (the cheapest form), three 9-bit passes when
// it says they do not (c5: every frame; hd1m: the views that see the cloud end on) -- the answer of the last frame whose
// blend has started.  Either width yields the same stable order, so the image does not depend on which frame's answer was the
// latest.  Nothing known (the first frame, a renderer without a mailbox, the stand-alone sorter) takes the default; a captured
// frame graph keeps the width it was captured with.
constexpr int depth_sort_digit_bits(int forced, bool skip_top, uint32_t span_class, int graph_depth_bits) {
    if (graph_depth_bits) return graph_depth_bits;
    if (forced == 8 || forced == 9) return forced;
    if (WS_DEPTH_DIGIT_BITS_ADAPTIVE && skip_top && span_class != 0u) return span_class == 2u ? 9 : 8;
    return WS_DEPTH_DIGIT_BITS_DEFAULT;
}

// The entry capacity a frame gets after one that needed `demand` entries overflowed: 1.25 x the demand and a margin.  The one rule
// of the automatic capacity below and of every driver that grows a renderer's list and draws again (drivers.cpp).
constexpr uint64_t grown_entry_capacity(uint32_t demand) { return (uint64_t)demand + demand / 4 + 4096; }

struct FramePlan {
    // the grid of binning tiles
    uint32_t tile_w_log2, tile_h_log2;  // tile size in pixels (8 * QW, 8 * QH)
    uint32_t tiles_x, tiles_y, ntiles;
    int footprint_mode;    // FootprintMode of the word K1 leaves per splat
    uint32_t bin_request;  // BinRequest K1 gets
    uint32_t entry_cap;    // (tile, splat) entries the frame has room for
    // the tile-id sort
    uint32_t wide_bins;       // != 0: ONE counting pass over the whole tile id with this many bins (a power of two >= ntiles); 0: digit passes
    bool fused_hist;          // k_bin_emit writes the first pass's per-tile digit counts (or the single pass's bin counts)
    int tile_bits;            // key bits that take part in the digit passes
    int digit_bits;           // their digit width, 6..8; ceil(tile_bits / digit_bits) <= 4 passes
    uint32_t tile_hist_mask;  // (1 << digit_bits) - 1: the first pass's digit, for k_bin_emit
    bool key16;               // the key arrays of the tile sort hold uint16_t
    int depth_digit_bits;     // the depth sort's digit width, 8 | 9 (depth_sort_digit_bits)
    int blend_order;          // != 0: k_blend_order runs, in this order mode (1 = the blend's workgroups take the longest list first)
    bool split_wanted;        // BlendFrameRequest::split_wanted

    constexpr bool wide_sort() const { return wide_bins != 0u; }
    // log2(wide_bins): the single pass's `bits`; the count rows' length and k_bin_emit's pitch are wide_bins itself
    constexpr int wide_bits() const {
        int b = 0;
        while ((1u << b) < wide_bins) ++b;
        return b;
    }
};

constexpr FramePlan frame_plan(const FramePlanRequest& q) {
    FramePlan p{};
    const uint32_t tile_w = QUAD * q.tile_qw, tile_h = QUAD * q.tile_qh;
    p.tile_w_log2 = q.tile_qw == 4 ? 5u : 4u;
    p.tile_h_log2 = q.tile_qh == 4 ? 5u : 4u;
    p.tiles_x = (q.viewport[0] + tile_w - 1) / tile_w;
    p.tiles_y = (q.viewport[1] + tile_h - 1) / tile_h;
    p.ntiles = p.tiles_x * p.tiles_y;
    const bool shape44 = q.tile_qw == 4 && q.tile_qh == 4;

    // the footprint word K1 leaves per splat: the packed rectangle while the viewport has at most 256 binning tiles per
    // axis, the rectangle's tile count beyond that; WS_FOOTPRINT=ellipse: the ellipse's own tile count
    p.footprint_mode = q.footprint == FP_ELLIPSE ? FP_ELLIPSE
                       : ((p.tiles_x > RECT_PACKED_MAX_TILES_PER_AXIS || p.tiles_y > RECT_PACKED_MAX_TILES_PER_AXIS) ? FP_RECT_COUNT : FP_RECT_PACKED);
    // Coarse binning (2 x 2 blend tiles per binning tile, decided per frame on the device: ws_internal.h bin_shift_decide) is
    // offered to frames of the default 32x32 shape whose rectangles travel packed; parity tooling that reads per-tile
    // lists back (capture mode) always sees the blend's own tiles.
    p.bin_request = (p.footprint_mode == FP_RECT_PACKED && !q.capture && shape44) ? (uint32_t)q.bin_request : (uint32_t)BIN_NEVER;

    uint64_t want_cap = q.entry_cap_request;
    if (want_cap == 0) {
        // automatic: 4 tile entries per Gaussian at ~1 Mpixel, growing with the pixel count (a splat's footprint in tiles
        // scales with the resolution), at least 8 M: twice what the BASELINE scenes need at the 32-px tile (hd1m 4.1 per
        // Gaussian at 2.2 Mpixel, c3 1.2), 16 B per entry -- c3 0.7 GB instead of the 4.1 GB of rounds 1-3 (24 per Gaussian;
        // round-3 verdict).  The safety net: an overflow is always flagged, the blend leaves the overflowed frame's demand
        // in the sticky words, and once the host has seen it the next prepare() allocates 1.25 x that.
        const double mpix = (double)q.viewport[0] * (double)q.viewport[1] / (1200.0 * 800.0);
        const uint64_t formula = (uint64_t)(4.0 * (double)q.num_points * (1.0 < mpix ? mpix : 1.0));
        want_cap = formula < (8ull << 20) ? (8ull << 20) : formula;
        if (q.demand && want_cap < grown_entry_capacity(q.demand)) want_cap = grown_entry_capacity(q.demand);
    }
    // look-back words carry 30-bit counts (lookback.h): keep D below 2^30
    const uint64_t cap_max = (1ull << 30) - 2 * EMIT_TILE;
    p.entry_cap = (uint32_t)(want_cap < cap_max ? want_cap : cap_max);

    // the emit kernel cuts the entry list into the same 4096-entry tiles the radix sort uses, so it can hand
    // the sort the digit counts of its first pass for free
    p.fused_hist = sort_tile_size(p.entry_cap) == (uint32_t)EMIT_TILE;
    // The tile-id sort is "segmented": only the bits a tile id can have take part, split evenly over the passes
    // (3750 tiles -> 12 bits -> 6 + 6; 8160 tiles -> 13 bits -> 7 + 6(7); 32400 tiles -> 15 bits -> 8 + 7(8)).
    p.tile_bits = 1;
    while ((1ull << p.tile_bits) < p.ntiles) ++p.tile_bits;
    const int tile_passes = (p.tile_bits + RADIX_BITS - 1) / RADIX_BITS;
    p.digit_bits = (p.tile_bits + tile_passes - 1) / tile_passes;
    // A single pass (at most 256 tiles) would let EVERY sort workgroup end runs of EVERY tile: the last pass records the
    // tile ranges with two atomics per (workgroup, tile) run, the whole range table is then 16 cache lines, and atomics on
    // one line serialise -- measured 127 us for 247 tiles x 413 workgroups.  Two 6-bit passes instead: behind the first one
    // a workgroup holds a handful of tiles.
    if (tile_passes == 1 && p.ntiles > 64) p.digit_bits = 6;
    if (p.digit_bits < 6) p.digit_bits = 6;
    p.tile_hist_mask = (1u << p.digit_bits) - 1u;
    // tile ids fit 16 bits up to 65534 tiles (4096 x 4080 px): the key arrays of the tile sort then hold uint16_t
    p.key16 = p.ntiles < 65535u;
    // WS_TILE_SORT=wide: ONE counting pass over the whole tile id when the viewport has at most 2048 binning tiles: the emit
    // kernel leaves [sort tile][bin] counts, a column scan and a scatter follow -- two launches instead of five, the
    // entries are read once, and the tile ranges are prefix sums of the bin totals (launch_tile_sort_wide).  The count rows
    // are 4 B x sort tiles x bins: 8 KiB per 2048 entries of capacity at 2048 bins, 1.3 x the entry lists themselves; beyond
    // 1 GiB -- 250 M entries -- the tile sort stays with its digit passes.
    if (q.tile_sort_wide && p.fused_hist && p.ntiles > 64u && p.ntiles <= (uint32_t)TILE_SORT_WIDE_MAX_BINS) {
        uint32_t bins = 128u;
        while (bins < p.ntiles) bins <<= 1;
        const uint64_t sort_tiles = ((uint64_t)p.entry_cap + SORT_TILE - 1) / SORT_TILE;  // (>= 1: fused_hist)
        if (sort_tiles * bins * sizeof(uint32_t) <= (1ull << 30)) p.wide_bins = bins;
    }

    p.depth_digit_bits = depth_sort_digit_bits(q.depth_digit_bits, q.depth_skip_top != 0, q.span_class, q.graph_depth_bits);
    // The compositing workgroups in longest-list-first order: one tile per workgroup at the 32x32 tile, up to 4096 tiles =
    // eight rounds of workgroups on this chip: beyond that the tail is a small share of the kernel and the one-workgroup
    // ordering kernel, 3 us at 2040 tiles and 7.6 us at 8160, costs what it saves -- c5, 4K: measured; 4K-class frames
    // composite several tiles per workgroup and keep the image order.
    p.blend_order = (shape44 && p.ntiles <= 4096u && q.blend_tpw_log2 <= 0) ? q.order_mode : 0;
    // Split: two 512-thread workgroups (32x16 halves) per 32x32 binning tile, both reading the tile's list.  Automatic: when the
    // frame has fewer binning tiles than the chip holds 1024-thread blend workgroups (two per CU) -- small viewports --
    // the halves fill the chip and balance the long tiles (800x600, 0.5 M Gaussians: +24 % frames/s); above that the
    // doubled staging costs more with frames in flight than the finer synchronisation saves.
    p.split_wanted = q.blend_split >= 0 ? q.blend_split != 0 : (p.ntiles < 2u * (uint32_t)q.num_cus);
    return p;
}

}  // namespace ws
