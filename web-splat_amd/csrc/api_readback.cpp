// api_readback.cpp -- what is read back from a renderer's prepared frame: counters, the sorted arrays, tile ranges and lists, the
// stage and kernel times, the error words.  Every copy is ordered on the renderer's own stream (api_state.h copy_d2h).
#include <cstddef>
#include <cstring>
#include <vector>

#include "api_state.h"

using namespace ws;

// The first line of the frame's counters (up to the footprint totals), behind the frame's stream
static int read_frame_counters(ws_renderer* r, FrameCounters* fc) {
    WS_HIP(hipStreamSynchronize(r->last_stream));
    return copy_d2h(fc, r->scratch.counters(), offsetof(FrameCounters, tile_sums), r->last_stream);
}

// A tile's list as the tile-id sort's last pass leaves it: x = 0xFFFFFFFF - begin (an atomic max finds the smallest index),
// y = end, y == 0: no entry
struct TileList {
    uint32_t begin, end, length;
};
static TileList tile_list(uint2 range) {
    const uint32_t begin = range.y ? 0xFFFFFFFFu - range.x : 0u;
    return {begin, range.y, range.y - begin};
}

extern "C" {

int ws_renderer_download_depths(ws_renderer* r, uint32_t capacity, float* z, uint32_t* num_visible) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_download_depths: null renderer");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_download_depths: no prepared frame");
    if (!r->frame.depth) return fail(WS_ERR_STATE, "ws_renderer_download_depths: depth was off at prepare()");
    ws_frame_stats st;
    int rc = ws_renderer_frame_stats(r, &st);
    if (rc) return rc;
    if (num_visible) *num_visible = st.num_visible;
    const uint32_t v = st.num_visible;
    if (z && capacity < v) return fail(WS_ERR_INVALID, "ws_renderer_download_depths: capacity smaller than the visible count");
    if (!z || v == 0) return WS_OK;
    return copy_d2h(z, r->scratch.depths.get(), (size_t)v * sizeof(float), r->last_stream);
}

int ws_renderer_frame_stats(ws_renderer* r, ws_frame_stats* out) {
    if (!r || !out) return fail(WS_ERR_INVALID, "ws_renderer_frame_stats: null argument");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_frame_stats: no prepared frame");
    FrameCounters fc;
    WS_TRY(read_frame_counters(r, &fc));
    out->num_visible = fc.num_visible;
    out->num_tile_entries = fc.num_entries;
    out->tile_entries_capacity = r->plan.entry_cap;
    out->overflow = fc.overflow;
    return WS_OK;
}

// Number of tile LISTS of the last prepared frame and the shift from blend tiles to binning tiles: the device decides per
// frame (bin_shift_decide, k_bin_prefix) whether a list serves one blend tile or a 2x2 block of them.
static int frame_list_counts(ws_renderer* r, uint32_t* shift, uint32_t* lists_x, uint32_t* lists_y) {
    FrameCounters fc;
    WS_TRY(read_frame_counters(r, &fc));
    const uint32_t s = fc.bin_shift;
    *shift = s;
    *lists_x = (r->plan.tiles_x + s) >> s;
    *lists_y = (r->plan.tiles_y + s) >> s;
    return WS_OK;
}

int ws_renderer_binning_tile(ws_renderer* r, uint32_t* width, uint32_t* height) {
    if (!r || !width || !height) return fail(WS_ERR_INVALID, "ws_renderer_binning_tile: null argument");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_binning_tile: no prepared frame");
    uint32_t s, lx, ly;
    WS_TRY(frame_list_counts(r, &s, &lx, &ly));
    *width = (QUAD * r->ctx->tile_qw) << s;
    *height = (QUAD * r->ctx->tile_qh) << s;
    return WS_OK;
}

// Which depth-sorted arrays hold the prepared frame's order: where the sort's last pass left them, or -- decided on the device,
// read back here only when the frame could skip -- where pass 2 did (*skipped).
static int frame_depth_order(ws_renderer* r, const uint32_t** keys, const uint32_t** vals, bool* skipped) {
    const SortResult& d = r->frame.arrays.depth;
    uint32_t skip = 0;
    if (d.vals_skipped) {
        WS_HIP(hipStreamSynchronize(r->last_stream));
        WS_TRY(copy_d2h(&skip, &r->scratch.counters()->depth_skip_top, sizeof skip, r->last_stream));
    }
    *keys = skip ? d.keys_skipped : d.keys;
    *vals = skip ? d.vals_skipped : d.vals;
    *skipped = skip != 0;
    return WS_OK;
}

int ws_renderer_depth_sort_passes(ws_renderer* r, uint32_t* passes) {
    if (!r || !passes) return fail(WS_ERR_INVALID, "ws_renderer_depth_sort_passes: null argument");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_depth_sort_passes: no prepared frame");
    const uint32_t *keys, *vals;
    bool skipped;
    WS_TRY(frame_depth_order(r, &keys, &vals, &skipped));
    *passes = skipped ? 3u : 4u;
    return WS_OK;
}

int ws_renderer_depth_sort_digit_bits(ws_renderer* r, uint32_t* digit_bits) {
    if (!r || !digit_bits) return fail(WS_ERR_INVALID, "ws_renderer_depth_sort_digit_bits: null argument");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_depth_sort_digit_bits: no prepared frame");
    *digit_bits = (uint32_t)r->plan.depth_digit_bits;
    return WS_OK;
}

int ws_renderer_errors(ws_renderer* r, uint32_t* bits, uint32_t* entries_needed, int reset) {
    if (!r || !bits) return fail(WS_ERR_INVALID, "ws_renderer_errors: null argument");
    *bits = 0;
    if (entries_needed) *entries_needed = 0;
    if (!r->sticky.get()) return WS_OK;  // (never: allocated with the renderer)
    // The sticky word outlives failed prepare() calls and scratch reallocations (both clear `prepared`): bits that earlier
    // frames left must not disappear behind them.  Only the per-frame counter needs a prepared frame.
    WS_HIP(hipStreamSynchronize(r->last_stream));
    uint32_t both[2] = {0u, 0u};
    WS_TRY(copy_d2h(both, r->sticky.get(), sizeof(both), r->last_stream));
    *bits = both[0];
    if (both[1] > r->needed_seen) r->needed_seen = both[1];  // an overflowed frame's demand: the next prepare() allocates it
    if (entries_needed && r->frame.prepared && r->scratch.counters()) WS_TRY(copy_d2h(entries_needed, &r->scratch.counters()->entries_needed, sizeof(uint32_t), r->last_stream));
    if (reset && *bits) {
        WS_HIP(hipMemsetAsync(r->sticky.get(), 0, sizeof(uint32_t), r->last_stream));
        WS_HIP(hipStreamSynchronize(r->last_stream));
    }
    return WS_OK;
}

int ws_renderer_num_visible(ws_renderer* r, uint32_t* out) {
    if (!out) return fail(WS_ERR_INVALID, "ws_renderer_num_visible: null argument");
    ws_frame_stats st;
    int rc = ws_renderer_frame_stats(r, &st);
    if (rc) return rc;
    *out = st.num_visible;
    return WS_OK;
}

int ws_renderer_stage_times(ws_renderer* r, ws_stage_times* out) {
    if (!r || !out) return fail(WS_ERR_INVALID, "ws_renderer_stage_times: null argument");
    if (!r->timers || !r->ev_prepare_valid) return fail(WS_ERR_STATE, "ws_renderer_stage_times: timers not enabled");
    std::memset(out, 0, sizeof *out);
    WS_HIP(hipEventSynchronize(r->ev[3].get()));
    WS_HIP(hipEventElapsedTime(&out->preprocess_ms, r->ev[0].get(), r->ev[1].get()));
    WS_HIP(hipEventElapsedTime(&out->sorting_ms, r->ev[1].get(), r->ev[2].get()));
    WS_HIP(hipEventElapsedTime(&out->binning_ms, r->ev[2].get(), r->ev[3].get()));
    if (r->ev_render_valid) {
        WS_HIP(hipEventSynchronize(r->ev[5].get()));
        WS_HIP(hipEventElapsedTime(&out->rasterization_ms, r->ev[4].get(), r->ev[5].get()));
    }
    return WS_OK;
}

int ws_renderer_kernel_times(ws_renderer* r, uint32_t capacity, ws_kernel_time* out, uint32_t* count) {
    if (!r || !count) return fail(WS_ERR_INVALID, "ws_renderer_kernel_times: null argument");
    if (!r->marks.active) return fail(WS_ERR_STATE, "ws_renderer_kernel_times: needs ws_renderer_enable_timers(r, 2)");
    const KernelMarks& km = r->marks;
    *count = (uint32_t)km.n;
    if (km.n == 0) return WS_OK;
    WS_HIP(hipEventSynchronize(km.ev[km.n].get()));
    for (int i = 0; i < km.n && (uint32_t)i < capacity && out; ++i) {
        std::memset(&out[i], 0, sizeof out[i]);
        std::strncpy(out[i].name, km.label[i] ? km.label[i] : "?", sizeof(out[i].name) - 1);
        WS_HIP(hipEventElapsedTime(&out[i].ms, km.ev[i].get(), km.ev[i + 1].get()));
    }
    return WS_OK;
}

int ws_renderer_download_tile_stats(ws_renderer* r, uint32_t capacity, uint32_t* list_len, uint32_t* consumed,
                                    uint32_t* num_tiles) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_download_tile_stats: null renderer");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_download_tile_stats: no prepared frame");
    uint32_t bs, lx, ly;
    WS_TRY(frame_list_counts(r, &bs, &lx, &ly));
    const uint32_t nt = lx * ly;  // one entry per LIST (= per binning tile; capture keeps them at the blend tile)
    if (num_tiles) *num_tiles = nt;
    if (!list_len && !consumed) return WS_OK;
    if (capacity < nt) return fail(WS_ERR_INVALID, "ws_renderer_download_tile_stats: capacity smaller than the tile count");
    if (consumed && !r->capture)
        return fail(WS_ERR_STATE, "ws_renderer_download_tile_stats: consumed needs ws_renderer_enable_capture before render");
    WS_HIP(hipStreamSynchronize(r->last_stream));
    if (list_len) {
        std::vector<uint2> rg(nt);
        WS_TRY(copy_d2h(rg.data(), r->scratch.tile_ranges(), (size_t)nt * sizeof(uint2), r->last_stream));
        for (uint32_t i = 0; i < nt; ++i) list_len[i] = tile_list(rg[i]).length;
    }
    if (consumed) WS_TRY(copy_d2h(consumed, r->scratch.debug_consumed.get(), (size_t)nt * 4, r->last_stream));
    return WS_OK;
}

int ws_renderer_download_wave_stats(ws_renderer* r, uint32_t tile_capacity, uint32_t* walked) {
    if (!r || !walked) return fail(WS_ERR_INVALID, "ws_renderer_download_wave_stats: null argument");
    if (!r->frame.prepared || !r->capture)
        return fail(WS_ERR_STATE, "ws_renderer_download_wave_stats: needs ws_renderer_enable_capture and a rendered frame");
    const uint32_t nt = r->plan.ntiles;
    if (tile_capacity < nt) return fail(WS_ERR_INVALID, "ws_renderer_download_wave_stats: capacity smaller than the tile count");
    WS_HIP(hipStreamSynchronize(r->last_stream));
    WS_TRY(copy_d2h(walked, r->scratch.debug_walked.get(), r->scratch.debug_walked.bytes(), r->last_stream));
    return WS_OK;
}

int ws_renderer_download_tile_lists(ws_renderer* r, uint32_t tile_capacity, uint32_t* begin, uint32_t* end,
                                    uint32_t entry_capacity, uint32_t* entries, uint32_t* num_entries) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_download_tile_lists: null renderer");
    ws_frame_stats st;
    int rc = ws_renderer_frame_stats(r, &st);
    if (rc) return rc;
    uint32_t bs, lx, ly;
    WS_TRY(frame_list_counts(r, &bs, &lx, &ly));
    const uint32_t nt = lx * ly;  // one range per LIST (= per binning tile, ws_renderer_binning_tile)
    if (num_entries) *num_entries = st.num_tile_entries;
    if ((begin || end) && tile_capacity < nt) return fail(WS_ERR_INVALID, "ws_renderer_download_tile_lists: tile capacity too small");
    if (entries && entry_capacity < st.num_tile_entries)
        return fail(WS_ERR_INVALID, "ws_renderer_download_tile_lists: entry capacity too small");
    if (begin || end) {
        std::vector<uint2> rg(nt);
        WS_TRY(copy_d2h(rg.data(), r->scratch.tile_ranges(), (size_t)nt * sizeof(uint2), r->last_stream));
        for (uint32_t i = 0; i < nt; ++i) {
            const TileList l = tile_list(rg[i]);
            if (begin) begin[i] = l.begin;
            if (end) end[i] = l.end;
        }
    }
    if (entries && st.num_tile_entries)
        WS_TRY(copy_d2h(entries, r->frame.arrays.entries, (size_t)st.num_tile_entries * 4, r->last_stream));
    return WS_OK;
}

int ws_renderer_download_frame(ws_renderer* r, uint32_t capacity, void* splats, uint32_t* keys, uint32_t* src_index,
                               uint32_t* sorted, uint32_t* num_visible) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_download_frame: null renderer");
    ws_frame_stats st;
    int rc = ws_renderer_frame_stats(r, &st);
    if (rc) return rc;
    if (num_visible) *num_visible = st.num_visible;
    const uint32_t v = st.num_visible;
    if ((splats || keys || src_index || sorted) && capacity < v)
        return fail(WS_ERR_INVALID, "ws_renderer_download_frame: capacity smaller than the visible count");
    if (src_index && !r->capture && !r->frame.contrib)
        return fail(WS_ERR_STATE, "ws_renderer_download_frame: src_index needs ws_renderer_enable_capture before prepare");
    if (v == 0) return WS_OK;
    const uint32_t *sorted_keys, *sorted_idx;
    bool skipped;
    WS_TRY(frame_depth_order(r, &sorted_keys, &sorted_idx, &skipped));
    if (splats) {  // the caller gets the reference's 20-B records whatever stride the device keeps them at
        if (SPLAT_STRIDE == 20u) {
            WS_TRY(copy_d2h(splats, r->scratch.splats.get(), (size_t)v * 20, r->last_stream));
        } else {
            std::vector<uint8_t> padded((size_t)v * SPLAT_STRIDE);
            WS_TRY(copy_d2h(padded.data(), r->scratch.splats.get(), padded.size(), r->last_stream));
            for (size_t i = 0; i < (size_t)v; ++i) std::memcpy(static_cast<uint8_t*>(splats) + i * 20, padded.data() + i * SPLAT_STRIDE, 20);
        }
    }
    if (src_index) WS_TRY(copy_d2h(src_index, r->scratch.src_index.get(), (size_t)v * 4, r->last_stream));
    if (sorted) WS_TRY(copy_d2h(sorted, sorted_idx, (size_t)v * 4, r->last_stream));
    if (keys) {
        // the sort permutes the keys in place; un-permute them with the sorted indices so that the caller
        // gets keys in STORE order (what preprocess wrote)
        std::vector<uint32_t> ks(v), idx(v);
        WS_TRY(copy_d2h(ks.data(), sorted_keys, (size_t)v * 4, r->last_stream));
        WS_TRY(copy_d2h(idx.data(), sorted_idx, (size_t)v * 4, r->last_stream));
        for (uint32_t i = 0; i < v; ++i)
            if (idx[i] < v) keys[idx[i]] = ks[i];
    }
    return WS_OK;
}

}  // extern "C"
