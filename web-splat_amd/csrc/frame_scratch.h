// frame_scratch.h -- a renderer's per-frame device memory: how large every array is (scratch_layout, a pure function of the
// frame's plan, in the style of frame_plan.h) and the one object that owns them (FrameScratch).  A new per-frame array is one
// line in scratch_layout, one member and one alloc line below.  What the arrays are initialised with, and the syncs around a
// reallocation, stay with the caller (api_renderer.cpp renderer_ensure_scratch).  Host code; tests/test_scratch_layout.py enumerates
// the layout against the sizes the call sites used to spell out, tests/test_frame_scratch.py runs the ownership on the CPU.
#pragma once

#include <cstddef>
#include <initializer_list>

#include "device_buf.h"
#include "ws_internal.h"

namespace ws {

// The count rows of one radix sort over at most `cap` pairs (launch_sort_pairs, launch_tile_sort_wide)
struct SortShape {
    uint32_t cap, rows;
    uint32_t tiles;        // ceil(cap / SORT_TILE)
    uint32_t tiles_cap;    // row pitch of the count rows: the largest tile count any n <= cap can need
    uint32_t wide_bins;    // != 0: also room for the [tiles][wide_bins] rows of the single-pass tile-id sort
    size_t sum_words;      // words of SortScratch::tile_sums
    size_t wide_hist_words;  // words of SortScratch::wide_hist (0: none)
};
constexpr SortShape sort_shape(uint32_t cap, uint32_t wide_bins = 0, uint32_t rows = RADIX) {
    SortShape s{};
    s.cap = cap, s.rows = rows, s.wide_bins = wide_bins;
    s.tiles = (cap + SORT_TILE - 1) / SORT_TILE;
    if (s.tiles == 0) s.tiles = 1;
    const uint32_t small_n = cap < SORT_SMALL_MAX ? cap : SORT_SMALL_MAX;
    const uint32_t small_tiles = (small_n + SORT_THREADS * SORT_KPT_SMALL - 1) / (SORT_THREADS * SORT_KPT_SMALL);
    s.tiles_cap = small_tiles > s.tiles ? small_tiles : s.tiles;
    s.sum_words = (size_t)s.tiles_cap * rows;
    if (wide_bins) {
        if (s.sum_words < (size_t)s.tiles * wide_bins) s.sum_words = (size_t)s.tiles * wide_bins;
        s.wide_hist_words = wide_bins;
    }
    return s;
}
// the view the sort launchers take, over count rows of this shape
inline SortScratch sort_view(const SortShape& s, uint32_t* keys_alt, uint32_t* vals_alt, uint32_t* hist, uint32_t hist_pitch,
                             uint32_t* tile_sums, uint32_t* wide_hist) {
    SortScratch v;
    v.keys_alt = keys_alt, v.vals_alt = vals_alt, v.hist = hist, v.hist_pitch = hist_pitch;
    v.tile_sums = tile_sums, v.wide_hist = wide_hist;
    v.rows = s.rows, v.cap = s.cap, v.tiles = s.tiles, v.tiles_cap = s.tiles_cap, v.wide_bins = s.wide_bins;
    return v;
}

struct ScratchRequest {
    FramePlan plan;
    uint32_t num_points, vw, vh;
    bool fat_depth_sort;      // the context's depth sort is a fat form (DS_ONESWEEP | DS_COOP)
    // block counts that live next to their kernels
    uint32_t k1_blocks;       // preprocess_blocks(num_points)
    uint32_t bin_blocks;      // bin_prefix_blocks(num_points)
    uint32_t order_blocks;    // blend_order_blocks(plan.tiles_x, plan.tiles_y)
    size_t fat_status_words;  // fat_sort_status_words()
};

// Elements of every per-frame array
struct ScratchLayout {
    size_t splats;          // bytes: (n + 8) Splat records
    size_t points;          // each of keys_a/b, vals_a/b, fpw_a/b, src_index, bin_offsets
    size_t k1_status, bin_status;  // look-back words: one per block and one
    size_t entries;         // each of ekeys_a/b, evals_a/b
    size_t emit_start, blend_order;
    size_t debug_consumed, debug_walked;
    size_t zero;            // bytes: FrameZero and the tile ranges behind it
    SortShape sort_depth, sort_tiles;
    size_t fat_status;      // 0: the depth sort is not a fat form
    // allocated on first use
    size_t depths;          // the z plane (ws_renderer_enable_depth)
    size_t debug_timing;    // ws_renderer_enable_blend_timing
    size_t removal_base;    // pixels: ws_renderer_accumulate_removal / _gradient without d_base
};

constexpr ScratchLayout scratch_layout(const ScratchRequest& q) {
    ScratchLayout l{};
    const size_t n = q.num_points;
    l.points = n + 8;
    l.splats = l.points * SPLAT_STRIDE;
    l.k1_status = (size_t)q.k1_blocks + 1;
    l.bin_status = (size_t)q.bin_blocks + 1;
    l.entries = (size_t)q.plan.entry_cap + 8;
    l.emit_start = (size_t)q.plan.entry_cap / EMIT_TILE + 4;
    l.blend_order = (size_t)q.order_blocks + 8;
    l.debug_consumed = q.plan.ntiles;
    l.debug_walked = (size_t)q.plan.ntiles * 17;
    l.zero = sizeof(FrameZero) + (size_t)q.plan.ntiles * sizeof(uint2);
    l.sort_depth = sort_shape(q.num_points ? q.num_points : 1u, 0, 512);  // (512 count rows: 9-bit digits)
    l.sort_tiles = sort_shape(q.plan.entry_cap, q.plan.wide_bins);
    l.fat_status = q.fat_depth_sort ? q.fat_status_words : 0;
    l.depths = n + 8;
    l.debug_timing = (size_t)q.plan.ntiles * 16 * BLEND_TIMING_WORDS;
    l.removal_base = (size_t)q.vw * q.vh;
    return l;
}

struct FrameScratch {
    ScratchLayout layout{};  // what alloc() was asked for (the arrays allocated on first use take their size from it)
    DeviceBuf<uint8_t> splats;  // Splat[N] (pointcloud.rs:103-108 allocates it in PointCloud; per renderer here, so that renderers never share scratch)
    DeviceBuf<uint32_t> keys_a, keys_b, vals_a, vals_b;
    DeviceBuf<uint32_t> fpw_a, fpw_b;  // footprint words (FootprintMode): store order / ping-pong of the depth sort
    DeviceBuf<uint32_t> src_index, bin_offsets;
    DeviceBuf<uint64_t> k1_status, bin_status;  // epoch-tagged look-back words (re-zeroed only when the epoch wraps)
    DeviceBuf<uint32_t> ekeys_a, ekeys_b, evals_a, evals_b, emit_start;
    DeviceBuf<uint4> blend_order;      // the blend's tiles, longest list first (k_blend_order)
    DeviceBuf<uint32_t> debug_consumed, debug_walked;  // [tiles], [tiles][17]: written in capture mode only
    DeviceBuf<uint8_t> zero;           // counters | histograms | tile ranges: ONE memset per frame
    DeviceBuf<uint32_t> depth_sums, tile_sums, tile_wide_hist;  // the two sorts' count rows
    DeviceBuf<uint64_t> fat_status;    // fat-tile one-sweep depth sort: chunk-count rows
    DeviceBuf<float> depths;           // [N] view-space depth per store slot
    DeviceBuf<uint32_t> debug_timing;  // [tiles][16][BLEND_TIMING_WORDS]
    DeviceBuf<float4> removal_base;

    // All arrays but the three allocated on first use.  On a failure the object is empty and the code is returned.
    int alloc(const ScratchLayout& l) {
        *this = FrameScratch();
        const int rc = alloc_all(l);
        if (rc) *this = FrameScratch();
        else layout = l;
        return rc;
    }

    FrameZero* arena() const { return reinterpret_cast<FrameZero*>(zero.get()); }
    FrameCounters* counters() const { return reinterpret_cast<FrameCounters*>(zero.get()); }  // = &arena()->counters
    uint2* tile_ranges() const { return zero.get() ? reinterpret_cast<uint2*>(zero.get() + sizeof(FrameZero)) : nullptr; }

    // the views the sort launchers take
    SortScratch sort_depth() const {
        return sort_view(layout.sort_depth, keys_b.get(), vals_b.get(), arena()->depth_hist, 512, depth_sums.get(), nullptr);
    }
    SortScratch sort_tiles() const {
        return sort_view(layout.sort_tiles, ekeys_b.get(), evals_b.get(), arena()->tile_hist, 256, tile_sums.get(), tile_wide_hist.get());
    }
    FatSortScratch fat_sort(int grid_request) const {
        FatSortScratch fs;
        fs.cap = layout.sort_depth.cap, fs.status = fat_status.get(), fs.grid_request = grid_request;
        fs.keys_alt = keys_b.get(), fs.vals_alt = vals_b.get(), fs.aux_alt = fpw_b.get();
        fs.hist = arena()->depth_hist;
        fs.tickets = counters()->sort_ticket;  // [0..3]; the tile sort uses [4..7]
        fs.barrier = arena()->fat_barrier;
        fs.d_epoch = &counters()->epoch;       // written by K1 every frame: a captured frame graph replays with it
        fs.error = &counters()->overflow;
        return fs;
    }

private:
    int alloc_all(const ScratchLayout& l) {  // (in this order: what a failure half-way has reserved is part of the behaviour)
        WS_TRY(splats.alloc(l.splats));
        for (auto* b : {&keys_a, &keys_b, &vals_a, &vals_b, &fpw_a, &fpw_b, &src_index, &bin_offsets}) WS_TRY(b->alloc(l.points));
        WS_TRY(k1_status.alloc(l.k1_status));
        WS_TRY(bin_status.alloc(l.bin_status));
        for (auto* b : {&ekeys_a, &ekeys_b, &evals_a, &evals_b}) WS_TRY(b->alloc(l.entries));
        WS_TRY(emit_start.alloc(l.emit_start));
        WS_TRY(blend_order.alloc(l.blend_order));
        WS_TRY(debug_consumed.alloc(l.debug_consumed));
        WS_TRY(debug_walked.alloc(l.debug_walked));
        WS_TRY(zero.alloc(l.zero));
        WS_TRY(depth_sums.alloc(l.sort_depth.sum_words));
        if (l.sort_tiles.wide_hist_words) WS_TRY(tile_wide_hist.alloc(l.sort_tiles.wide_hist_words));
        WS_TRY(tile_sums.alloc(l.sort_tiles.sum_words));
        if (l.fat_status) WS_TRY(fat_status.alloc(l.fat_status));
        return WS_OK;
    }
};
static_assert(offsetof(FrameZero, counters) == 0, "FrameScratch::counters()");

}  // namespace ws
