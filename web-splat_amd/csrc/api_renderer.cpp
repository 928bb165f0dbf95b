// api_renderer.cpp -- ws_renderer (GaussianRenderer, renderer.rs:17-283): create, destroy and the switches, the scratch and its
// demand, and the frame: prepare() (launch by launch, or as a captured graph: frame_graph.h), the grouped prepare of a view batch,
// and render() with its auxiliary and composite forms.  What is read back from a frame is in api_readback.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_state.h"

namespace ws {

int KernelMarks::create() {
    if (created) return WS_OK;
    for (auto& e : ev) WS_TRY(e.create(true));
    created = true;
    return WS_OK;
}
void KernelMarks::begin(hipStream_t s, bool restart) {
    stream = s;
    if (restart) n = 0;
    // render() continues the frame prepare() started: ev[n] already closes the previous interval
    if (n == 0) (void)hipEventRecord(ev[0].get(), s);
}
void KernelMarks::mark(const char* what) {
    if (n >= MAX) return;
    label[n] = what;
    (void)hipEventRecord(ev[n + 1].get(), stream);
    ++n;
}

}  // namespace ws

using namespace ws;

// Frees the captured frame graph: the one place that does.  The depth sort's digit width is the plan's one rule that reads the graph
// (a valid graph keeps the width it was captured with): it is asked again, so that a plan made while the graph stood chooses its own width.
static void renderer_free_graph(ws_renderer* r) {
    r->fg.reset();
    r->plan.depth_digit_bits = depth_sort_digit_bits(r->ctx->depth_digit_bits, r->ctx->depth_skip_top != 0, r->mailbox.span_class(), 0);
}

// Lets the scratch go (no sync: the callers have waited for the device) and with it the frame that lived in it
static void renderer_free_scratch(ws_renderer* r) {
    renderer_free_graph(r);
    ++r->scratch_generation;
    r->scratch = FrameScratch();
    r->cap_points = 0;
    r->vw = r->vh = 0;
    r->frame = PreparedFrame();
}

// What the automatic entry capacity of a frame of n points at vw x vh may grow to (FramePlanRequest::demand): an overflowed
// frame's demand arrives by the mailbox (no sync, no polling by the caller) or by ws_renderer_errors.
// It belongs to THIS point-cloud size and viewport: another scene or target size starts from the formula again
// (one heavy frame must not inflate the scratch for the renderer's lifetime).
static int renderer_refresh_demand(ws_renderer* r, uint32_t n, uint32_t vw, uint32_t vh) {
    if (r->scratch.zero.get() && (r->cap_points != n || r->vw != vw || r->vh != vh)) {
        r->needed_seen = 0;
        if (r->mailbox.present()) {
            WS_HIP(hipDeviceSynchronize());
            r->mailbox.clear_demand();
            WS_HIP(hipMemset(r->sticky.get() + 1, 0, sizeof(uint32_t)));
        }
    } else {
        const uint32_t posted = r->mailbox.demand();
        if (posted > r->needed_seen) r->needed_seen = posted;
    }
    return WS_OK;
}

// The scratch of frames of n points at vw x vh laid out by `plan` (frame_scratch.h); kept while those three and the entry
// capacity stay.  Here: the syncs around a reallocation and what the new arrays start with.
static int renderer_ensure_scratch(ws_renderer* r, uint32_t n, uint32_t vw, uint32_t vh, const FramePlan& plan) {
    const bool keep = r->cap_points == n && r->vw == vw && r->vh == vh && r->plan.entry_cap == plan.entry_cap && r->scratch.zero.get();
    r->plan = plan;
    if (keep) return WS_OK;
    WS_HIP(hipDeviceSynchronize());
    renderer_free_scratch(r);
    ScratchRequest q{};
    q.plan = plan, q.num_points = n, q.vw = vw, q.vh = vh;
    q.fat_depth_sort = r->ctx->depth_sort_mode == DS_ONESWEEP || r->ctx->depth_sort_mode == DS_COOP;
    q.k1_blocks = preprocess_blocks(n), q.bin_blocks = bin_prefix_blocks(n);
    q.order_blocks = blend_order_blocks(plan.tiles_x, plan.tiles_y), q.fat_status_words = fat_sort_status_words();
    FrameScratch& sc = r->scratch;
    WS_TRY(sc.alloc(scratch_layout(q)));
    WS_HIP(hipMemset(sc.k1_status.get(), 0, sc.k1_status.bytes()));
    WS_HIP(hipMemset(sc.bin_status.get(), 0, sc.bin_status.bytes()));
    // the per-frame zero arena: counters | depth histograms | tile histograms | tile ranges
    WS_HIP(hipMemset(sc.zero.get(), 0, sc.zero.bytes()));
    if (sc.fat_status.get()) WS_HIP(hipMemset(sc.fat_status.get(), 0, sc.fat_status.bytes()));
    r->cap_points = n, r->vw = vw, r->vh = vh;
    r->epoch = 0;  // fresh (zeroed) status arrays
    // The allocation-time memsets above ran on the null stream; frames run on hipStreamNonBlocking streams, which are
    // not ordered against it, and recycled memory may still hold a previous renderer's epoch-tagged words.
    WS_HIP(hipDeviceSynchronize());
    return WS_OK;
}

extern "C" {

// ---- GaussianRenderer --------------------------------------------------------------------------------
int ws_renderer_create(ws_context* ctx, ws_color_format format, uint32_t sh_deg, int compressed, ws_renderer** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_renderer_create: null argument");
    *out = nullptr;
    if (sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_renderer_create: sh_deg > 3");
    if (format != WS_FORMAT_RGBA8_UNORM && format != WS_FORMAT_RGBA16_FLOAT && format != WS_FORMAT_RGBA32_FLOAT)
        return fail(WS_ERR_INVALID, "ws_renderer_create: unknown colour format");
    std::unique_ptr<ws_renderer, SyncedDelete> r(new (std::nothrow) ws_renderer());
    if (!r) return fail(WS_ERR_OOM, "ws_renderer_create: host allocation failed");
    r->ctx = ctx;
    r->format = format;
    r->sh_deg = sh_deg;
    r->compressed = compressed != 0;
    r->capture = ctx->capture;
    for (auto& e : r->ev)
        if (e.create(true) != WS_OK) return fail(WS_ERR_HIP, "ws_renderer_create: hipEventCreate failed");
    if (r->sticky.alloc(2) != WS_OK || hipMemset(r->sticky.get(), 0, r->sticky.bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(WS_ERR_HIP, "ws_renderer_create: error word allocation failed");
    // the mailbox (optional: without pinned memory the capacity still grows through ws_renderer_errors)
    (void)r->mailbox.create();
    (void)hipGetLastError();
    *out = r.release();
    return WS_OK;
}

void ws_renderer_destroy(ws_renderer* r) { SyncedDelete()(r); }

ws_color_format ws_renderer_color_format(const ws_renderer* r) { return r ? r->format : WS_FORMAT_RGBA32_FLOAT; }

int ws_renderer_enable_timers(ws_renderer* r, int enable) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_timers: null renderer");
    r->timers = enable != 0;
    r->ev_prepare_valid = r->ev_render_valid = false;
    r->marks.active = false;
    r->marks.n = 0;
    if (enable >= 2) {  // per-kernel events
        int rc = r->marks.create();
        if (rc) return rc;
        r->marks.active = true;
    }
    return WS_OK;
}

int ws_renderer_set_blend_mode(ws_renderer* r, int mode) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_set_blend_mode: null renderer");
    if (mode != WS_BLEND_FAST && mode != WS_BLEND_TARGET_PRECISION && mode != WS_BLEND_FAST_EXACT_CUT)
        return fail(WS_ERR_INVALID, "ws_renderer_set_blend_mode: unknown mode");
    r->blend_mode = mode;
    return WS_OK;
}

int ws_renderer_enable_capture(ws_renderer* r, int enable) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_capture: null renderer");
    // Whether a frame bins coarse (64-px lists) is latched at prepare() from the capture state, and the capture blend's
    // per-tile read-backs are sized by that frame's lists: a frame prepared under the other state must not be drawn or
    // read back under this one -- the caller prepares again.
    if (r->capture != (enable != 0)) r->frame = PreparedFrame();
    r->capture = enable != 0;
    return WS_OK;
}

int ws_renderer_download_blend_order(ws_renderer* r, uint32_t capacity_blocks, uint32_t* order4, uint32_t* num_blocks) {
    if (!r || !num_blocks) return fail(WS_ERR_INVALID, "ws_renderer_download_blend_order: null argument");
    if (!r->frame.prepared) return fail(WS_ERR_STATE, "ws_renderer_download_blend_order: no prepared frame");
    const uint32_t nb = r->frame.arrays.blend_order_valid ? blend_order_blocks(r->plan.tiles_x, r->plan.tiles_y) : 0u;
    *num_blocks = nb;
    if (!order4 || nb == 0) return WS_OK;
    if (capacity_blocks < nb) return fail(WS_ERR_INVALID, "ws_renderer_download_blend_order: capacity smaller than the block count");
    WS_HIP(hipStreamSynchronize(r->last_stream));
    return copy_d2h(order4, r->scratch.blend_order.get(), (size_t)nb * sizeof(uint4), r->last_stream);
}

// Analysis of frames in flight (round 6): rocprofv3's kernel trace serialises the queues, so what really runs beside what is
// measured on the device -- K1 and the blend of the next `frames` frames of this renderer leave {min start, max end} of their
// workgroups on the 100-MHz device clock (one 64-bit atomic per workgroup at each end; off: a null pointer, one scalar branch).
static uint32_t trace_capacity(const ws_renderer* r) { return (uint32_t)(r->frame_trace.count() / 4); }  // frames

int ws_renderer_enable_frame_trace(ws_renderer* r, uint32_t frames) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_frame_trace: null renderer");
    if (r->last_stream || r->frame.prepared) WS_HIP(hipStreamSynchronize(r->last_stream));
    r->frame_trace.reset();
    r->trace_count = 0;
    r->frame.trace_slot = nullptr;
    if (frames == 0) return WS_OK;
    std::vector<unsigned long long> init((size_t)frames * 4);
    for (uint32_t i = 0; i < frames; ++i) {
        init[4 * i + 0] = init[4 * i + 2] = ~0ull;
        init[4 * i + 1] = init[4 * i + 3] = 0ull;
    }
    DeviceBuf<unsigned long long> trace;
    WS_TRY(trace.alloc(init.size()));
    WS_HIP(hipMemcpyAsync(trace.get(), init.data(), trace.bytes(), hipMemcpyHostToDevice, r->last_stream));
    WS_HIP(hipStreamSynchronize(r->last_stream));
    r->frame_trace = std::move(trace);  // (from here on prepare() hands its slots out)
    return WS_OK;
}

int ws_renderer_download_frame_trace(ws_renderer* r, uint32_t capacity, uint64_t* stamps, uint32_t* count) {
    if (!r || !count) return fail(WS_ERR_INVALID, "ws_renderer_download_frame_trace: null argument");
    *count = std::min(r->trace_count, trace_capacity(r));
    if (!stamps) return WS_OK;
    if (capacity < *count) return fail(WS_ERR_INVALID, "ws_renderer_download_frame_trace: capacity smaller than the traced frames");
    if (*count == 0) return WS_OK;
    // (on the renderer's own stream, like every read-back of this library: never the legacy NULL stream)
    return copy_d2h(stamps, r->frame_trace.get(), (size_t)*count * 4 * sizeof(unsigned long long), r->last_stream);
}

int ws_renderer_enable_blend_timing(ws_renderer* r, int enable) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_blend_timing: null renderer");
    r->blend_timing = enable != 0;
    return WS_OK;
}

int ws_renderer_download_blend_timing(ws_renderer* r, uint32_t tile_capacity, uint32_t* times, uint32_t* num_tiles) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_download_blend_timing: null renderer");
    const uint32_t nt = r->plan.ntiles;
    if (num_tiles) *num_tiles = nt;
    if (!times) return WS_OK;
    if (!r->frame.prepared || !r->blend_timing || !r->scratch.debug_timing.get())
        return fail(WS_ERR_STATE, "ws_renderer_download_blend_timing: needs ws_renderer_enable_blend_timing and a rendered frame");
    if (tile_capacity < nt) return fail(WS_ERR_INVALID, "ws_renderer_download_blend_timing: capacity smaller than the tile count");
    WS_HIP(hipStreamSynchronize(r->last_stream));
    return copy_d2h(times, r->scratch.debug_timing.get(), r->scratch.debug_timing.bytes(), r->last_stream);
}

int ws_renderer_set_tile_entry_capacity(ws_renderer* r, uint64_t entries) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_set_tile_entry_capacity: null renderer");
    r->entry_cap_request = entries;
    return WS_OK;
}

// The frame's launch sequence behind prepare(): reset -> K1 -> depth sort -> binning -> tile-id sort.  Enqueued launch
// by launch, or once under stream capture (ws_renderer_prepare replays the captured graph afterwards).
// phase: FRAME_ALL = the whole sequence; FRAME_CLEAR = the arena memset only, FRAME_REST = everything behind K1 (a view
// batch runs K1 for several renderers in ONE launch between the two: ws_internal_prepare_group).
enum FramePhase { FRAME_ALL = 0, FRAME_CLEAR = 1, FRAME_REST = 2 };
// The order of the blend's workgroups for the frame about to be enqueued: 0 = image order, 1 = longest list first (k_blend_order),
// 2 / 3 the measured experiments.  Decided ONCE per prepare() and outside any stream capture (a frame graph captured
// under one decision and replayed under another composited with a stale order table): the graph path re-captures when the
// decision changes.
// Longest first is what a frame drawn ALONE wants (blend -12 % hd1m, -18 % c3 / c2: no tail of idle slots).  With several
// frames in flight it is the wrong order, measured (profiles/r05/blend_order_ab.txt: hd1m -9 %, c3 -17 % frames/s): the first
// 512 workgroups are then the longest tiles, no slot retires for 40 (hd1m) to 120 us (c3), and the other frames' small
// dependent kernels, which live on the slots the blend's short tiles keep freeing, starve behind it.
// "In flight" = a slot of a view batch with several slots, or -- for renderers driven by the caller's own loop -- a context
// whose prepare() calls change stream from call to call (frames in flight on a ring of streams do; a renderer that draws
// one frame at a time stays on its stream: after four consecutive calls on one stream it orders its tiles).
static int decide_blend_order(ws_renderer* r, hipStream_t stream) {
    bool in_flight = r->throughput_mode;
    if (!in_flight) {
        ws_context* c = r->ctx;
        void* const prev = c->last_prepare_stream.exchange(static_cast<void*>(stream), std::memory_order_relaxed);
        uint32_t run = 0;
        if (prev == static_cast<void*>(stream)) run = c->same_stream_run.fetch_add(1u, std::memory_order_relaxed) + 1u;
        else c->same_stream_run.store(0u, std::memory_order_relaxed);
        in_flight = run < 4u;
    }
    return r->ctx->blend_order < 0 ? (in_flight ? 0 : 1) : r->ctx->blend_order;
}

// the renderer holds a prepared frame of pc, enqueued on stream
static int frame_prepared(ws_renderer* r, const ws_pointcloud* pc, hipStream_t stream) {
    r->frame.prepared = true;
    r->frame.pc = pc;
    r->last_stream = stream;
    return WS_OK;
}

static int enqueue_frame(ws_renderer* r, const ws_pointcloud* pc, const K1Params& kp, const K1Buffers& kb, hipStream_t stream,
                         int phase = FRAME_ALL) {
    int rc;
    const FramePlan& plan = r->plan;
    const FrameScratch& sc = r->scratch;
    FrameCounters* const counters = sc.counters();
    uint2* const tile_ranges = sc.tile_ranges();
    KernelMarks* km = r->marks.active ? &r->marks : nullptr;
    if (phase != FRAME_REST) {
        // GPURSSorter::record_reset_indirect_buffer (gpu_rs.rs:720-727): keys_size = 0, dispatch = 0 -- here ONE
        // memset clears the counters, every ticket, both sorts' digit histograms and the tile ranges
        WS_HIP(hipMemsetAsync(sc.zero.get(), 0, sc.zero.bytes(), stream));
        if (phase == FRAME_CLEAR) return WS_OK;
        if (km) km->begin(stream, true);
        if (r->timers) WS_HIP(hipEventRecord(r->ev[0].get(), stream));
        if ((rc = launch_preprocess(kp, kb, pc->compressed, plan.footprint_mode, stream, r->frame.k1_depths))) return rc;
        km_mark(km, pc->compressed ? "k_preprocess<compressed>" : "k_preprocess");
        if (r->timers) WS_HIP(hipEventRecord(r->ev[1].get(), stream));
        if (km) {  // calibration interval between two kernels: the dispatch latency of a dependent launch
            if ((rc = launch_empty(stream))) return rc;
            km_mark(km, "_empty_launch");
        }
    }

    const int cut = r->ctx->debug_cut;
    if (cut == 1) return frame_prepared(r, pc, stream);  // analysis only (WS_DEBUG_CUT): the image is NOT produced
    // depth sort: V (key, store index) pairs, values start as iota (preprocess.wgsl:274), the splat's footprint word
    // (packed tile rectangle, or tile count) rides along as a companion value.  Default: the generic 4 x 8-bit sorter
    // (GPURSSorter's shape); WS_DEPTH_SORT=onesweep | coop: the fat-tile one-sweep (measured variants).
    const bool fat_sort = (r->ctx->depth_sort_mode == DS_ONESWEEP || r->ctx->depth_sort_mode == DS_COOP) && sc.fat_status.get() &&
                          fat_sort_grid(pc->num_points, r->ctx->num_cus, r->ctx->dsort_fat_grid) != 0u;
    if (fat_sort) {
        // fat-tile one-sweep (sort.hip k_dsort_fat): four 8-bit passes A -> B -> A -> B -> A, everything ends where it started
        if ((rc = launch_depth_sort_fat(sc.fat_sort(r->ctx->dsort_fat_grid), sc.keys_a.get(), sc.vals_a.get(), sc.fpw_a.get(), &counters->num_visible, pc->num_points, true,
                                        // (the single-launch form needs all its workgroups resident at once: never beside other
                                        // frames' kernels -- a slot of a view batch falls back to the one-sweep form)
                                        r->ctx->depth_sort_mode == DS_COOP && !r->throughput_mode, r->epoch, r->ctx->num_cus, stream,
                                        km, &r->frame.arrays.depth)))
            return rc;
    } else {
        // Four 8-bit passes over the 32-bit keys (gpu_rs.rs:865-884), of which the last one leaves at once on frames whose keys
        // span less than 2^24 (decided on the device from the key range the sort's first histogram kernel leaves: ws_internal.h
        // depth_range_decide; WS_DEPTH_SKIP_TOP=0 switches it off).  (K1c's keys are NOT confined to 24 bits: preprocess_compressed.wgsl:325 scales
        // clip z, which is below znear for the nearest splats.)
        SortJob job;
        job.kind = SORT_DEPTH;
        job.keys = sc.keys_a.get(), job.vals = sc.vals_a.get(), job.d_count = &counters->num_visible, job.n = pc->num_points;
        job.implicit_iota = true;
        job.aux = sc.fpw_a.get(), job.aux_alt = sc.fpw_b.get();
        job.skip_top = r->ctx->depth_skip_top ? counters : nullptr;
        job.kpt9 = r->ctx->depth_tile_kpt ? r->ctx->depth_tile_kpt : 8;
        job.digit_bits = plan.depth_digit_bits;  // (8 | 9, per frame: frame_plan.h depth_sort_digit_bits)
        if ((rc = launch_sort_pairs(sc.sort_depth(), job, stream, km, &r->frame.arrays.depth))) return rc;
    }
    if (r->timers) WS_HIP(hipEventRecord(r->ev[2].get(), stream));
    if (cut == 2) return frame_prepared(r, pc, stream);  // analysis only (WS_DEBUG_CUT): the image is NOT produced

    // tile binning
    BinBuffers bb;
    bb.sorted_idx = r->frame.arrays.depth.vals;
    bb.fp_sorted = r->frame.arrays.depth.aux;
    bb.sorted_idx_alt = r->frame.arrays.depth.vals_skipped;
    bb.fp_sorted_alt = r->frame.arrays.depth.aux_skipped;
    bb.footprint_mode = plan.footprint_mode;
    bb.splats = sc.splats.get();
    bb.vw = kp.cam.viewport[0];
    bb.vh = kp.cam.viewport[1];
    bb.tile_w_log2 = plan.tile_w_log2;
    bb.tile_h_log2 = plan.tile_h_log2;
    bb.offsets = sc.bin_offsets.get();
    bb.emit_start = sc.emit_start.get();
    bb.block_status = sc.bin_status.get();
    bb.entry_keys = sc.ekeys_a.get();
    bb.entry_vals = sc.evals_a.get();
    bb.entry_cap = plan.entry_cap;
    bb.tile_ranges = tile_ranges;
    bb.counters = counters;
    bb.max_points = pc->num_points;
    bb.tiles_x = plan.tiles_x;
    bb.tiles_y = plan.tiles_y;
    // the tile-id sort's shape (frame_plan.h): k_bin_emit writes the counts of its first pass -- or of its only pass, as
    // [sort tile][bin] rows of wide_bins words -- and the sort below reads them with the same digit width and key width
    const SortScratch sort_tiles = sc.sort_tiles();
    bb.tile_hist = plan.fused_hist ? sort_tiles.tile_sums : nullptr;
    bb.tile_hist_pitch = plan.wide_sort() ? plan.wide_bins : sort_tiles.tiles_cap;
    bb.tile_hist_mask = plan.tile_hist_mask;
    bb.tile_hist_wide = plan.wide_sort() ? 1 : 0;
    bb.key16 = plan.key16 ? 1 : 0;
    if ((rc = launch_bin_prefix(bb, stream))) return rc;
    km_mark(km, "k_bin_prefix");
    if ((rc = launch_bin_emit(bb, stream))) return rc;
    km_mark(km, "k_bin_emit");
    if (cut == 3) return frame_prepared(r, pc, stream);
    SortResult tiles;
    if (plan.wide_sort()) {
        if ((rc = launch_tile_sort_wide(sort_tiles, sc.ekeys_a.get(), sc.evals_a.get(), &counters->num_entries, plan.entry_cap,
                                        plan.wide_bits(), stream, km, tile_ranges, plan.ntiles, &tiles)))
            return rc;
    } else {
        SortJob job;
        job.kind = SORT_TILE_IDS;
        job.keys = sc.ekeys_a.get(), job.vals = sc.evals_a.get(), job.d_count = &counters->num_entries, job.n = plan.entry_cap;
        job.end_bit = plan.tile_bits, job.digit_bits = plan.digit_bits;
        job.first_tile_hist_ready = plan.fused_hist, job.key16 = plan.key16;
        job.ranges = tile_ranges, job.nranges = plan.ntiles;
        if ((rc = launch_sort_pairs(sort_tiles, job, stream, km, &tiles))) return rc;
    }
    r->frame.arrays.entries = tiles.vals;  // the last pass wrote the per-tile ranges instead of the sorted tile ids
    // the compositing workgroups in longest-list-first order, where the plan says so (the order mode itself is decided once
    // per prepare(), OUTSIDE any captured region: decide_blend_order)
    r->frame.arrays.blend_order_valid = false;
    if (plan.blend_order) {
        if ((rc = launch_blend_order(tile_ranges, counters, plan.tiles_x, plan.tiles_y, sc.blend_order.get(), plan.blend_order, stream))) return rc;
        km_mark(km, "k_blend_order");
        r->frame.arrays.blend_order_valid = true;
    }
    if (r->timers) {
        WS_HIP(hipEventRecord(r->ev[3].get(), stream));
        r->ev_prepare_valid = true;
    }
    return frame_prepared(r, pc, stream);
}

// Validation, scratch, uniforms, buffers and the frame's look-back epoch: everything of prepare() in front of the first
// launch.  Shared by ws_renderer_prepare and the view batch's grouped prepare.
static int prepare_setup(ws_renderer* r, const ws_pointcloud* pc, const ws_splatting_args* args, hipStream_t stream,
                         K1Params* kp_out, K1Buffers* kb_out) {
    if (!r || !pc || !args) return fail(WS_ERR_INVALID, "ws_renderer_prepare: null argument");
    if (pc->compressed != r->compressed)
        return fail(WS_ERR_INVALID, "ws_renderer_prepare: renderer and point cloud disagree on `compressed`");
    if (!frame_viewport_ok(args->viewport[0], args->viewport[1], r->ctx->tile_qw, r->ctx->tile_qh))
        return fail(WS_ERR_INVALID, "ws_renderer_prepare: bad viewport (at most 65535 binning tiles per axis)");
    if (args->max_sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_renderer_prepare: max_sh_deg > 3");
    // (uncompressed, max_sh_deg above the point cloud's degree: the 96-B record always holds 16 coefficients, zeros above the
    // file's degree -- harmless, as in the reference)
    if (pc->compressed && args->max_sh_deg > r->sh_deg)
        return fail(WS_ERR_INVALID, "ws_renderer_prepare: max_sh_deg exceeds the renderer's SH layout degree");
    if (pc->compressed && pc->sh_deg > r->sh_deg)
        return fail(WS_ERR_INVALID, "ws_renderer_prepare: compressed point cloud has a higher SH degree than the renderer was created for");
    r->frame = PreparedFrame();
    int rc;
    // an automatic capacity follows the demand of this scene's and viewport's overflowed frames
    if (r->entry_cap_request == 0 && (rc = renderer_refresh_demand(r, pc->num_points, args->viewport[0], args->viewport[1]))) return rc;
    // the frame's plan (frame_plan.h): everything below -- scratch, K1's parameters, the launches of enqueue_frame -- reads it
    const ws_context* c = r->ctx;
    FramePlanRequest q{};
    q.tile_qw = c->tile_qw, q.tile_qh = c->tile_qh, q.footprint = c->footprint, q.tile_sort_wide = c->tile_sort_wide;
    q.bin_request = c->bin_request, q.blend_tpw_log2 = c->blend_tpw_log2, q.blend_split = c->blend_split, q.num_cus = c->num_cus;
    q.depth_digit_bits = c->depth_digit_bits, q.depth_skip_top = c->depth_skip_top;
    q.num_points = pc->num_points, q.viewport[0] = args->viewport[0], q.viewport[1] = args->viewport[1], q.capture = r->capture;
    q.entry_cap_request = r->entry_cap_request, q.demand = r->needed_seen;
    q.order_mode = r->order_mode = decide_blend_order(r, stream);
    q.span_class = r->mailbox.span_class();
    q.graph_depth_bits = r->fg.depth_bits();
    if ((rc = renderer_ensure_scratch(r, pc->num_points, args->viewport[0], args->viewport[1], frame_plan(q)))) return rc;
    const FramePlan& plan = r->plan;
    FrameScratch& sc = r->scratch;
    // the z plane: 4 B per splat, allocated while depth is on and freed with the scratch
    if (r->depth && !sc.depths.get() && (rc = sc.depths.alloc(sc.layout.depths))) return rc;
    r->frame.k1_depths = r->depth ? sc.depths.get() : nullptr;

    K1Params kp;
    std::memset(&kp, 0, sizeof kp);
    build_camera_uniform(args->camera, args->viewport, &kp.cam);
    if ((rc = ws_build_settings_uniform(args, pc, &kp.rs))) return rc;
    kp.quant = pc->quant;
    kp.num_points = pc->num_points;
    // stride of the packed int8 SH records: the POINT CLOUD's degree (the records were laid out by its loader); a
    // renderer created for another degree must not re-interpret them (WebGPU would clamp the reads, HIP would not)
    kp.sh_deg_layout = (pc->sh_deg + 1) * (pc->sh_deg + 1);
    kp.tiles_x = plan.tiles_x;
    kp.tiles_y = plan.tiles_y;
    kp.tile_w_log2 = plan.tile_w_log2;
    kp.tile_h_log2 = plan.tile_h_log2;
    kp.bin_request = plan.bin_request;
    kp.znear = -kp.cam.proj[3 * 4 + 2] / kp.cam.proj[2 * 4 + 2];
    kp.zfar = -kp.cam.proj[3 * 4 + 2] / (kp.cam.proj[2 * 4 + 2] - 1.0f);
    r->frame.znear = kp.znear;
    r->frame.zfar = kp.zfar;
    for (int i = 0; i < 3; ++i) r->frame.cam_pos[i] = kp.cam.view_inv[12 + i];
    r->frame.max_sh_deg = kp.rs.max_sh_deg;
    r->frame.cam = kp.cam;
    r->frame.settings = kp.rs;
    // fade-in (preprocess.wgsl:196-203): once walltime is past (largest possible dd) + 1, smoothstep(walltime - dd) is exactly
    // 1 for every Gaussian and the kernel skips the computation.  One rule, dd = 5 |centre - xyz| / extend bounded two ways:
    //   * every Gaussian that reaches k1_math lies inside the bbox (the default clip box IS the bbox; a user box may admit
    //     Gaussians outside it, so the shortcut is off with one), and extend >= the bbox radius;
    //   * the centre is the CALLER's (ws_pointcloud_create copies it unchecked).  Inside the bbox, |centre - xyz| <= 2 radius,
    //     dd <= 10, and walltime >= 11 suffices (every cloud a loader produces).  Anywhere else the triangle inequality gives
    //     dd <= 5 (|centre - bbox midpoint| + radius) / extend, and walltime has to pass that bound (with a margin far above
    //     the kernel's f32 rounding of dd) plus 1 as well.
    bool fade_done = kp.rs.walltime >= 11.0f && kp.rs.scene_extend > 0.0f && std::isfinite(kp.rs.scene_extend) &&
                     !args->has_clipping_box;
    bool centre_inside = true;
    for (int i = 0; i < 3; ++i)
        centre_inside = centre_inside && pc->center[i] >= pc->bbox.min[i] && pc->center[i] <= pc->bbox.max[i];
    if (fade_done && !centre_inside) {  // (a NaN centre lands here too, and fails the comparison below)
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double mid = 0.5 * ((double)pc->bbox.min[i] + (double)pc->bbox.max[i]);
            d2 += ((double)pc->center[i] - mid) * ((double)pc->center[i] - mid);
        }
        const double dd_max = 5.0 * (std::sqrt(d2) + (double)ws_aabb_radius(&pc->bbox)) / (double)kp.rs.scene_extend;
        fade_done = (double)kp.rs.walltime >= dd_max * 1.0001 + 1.0;
    }
    kp.fade_done = fade_done ? 1u : 0u;

    K1Buffers kb;
    kb.planes = pc->planes.get();
    kb.gaussians_c = pc->gaussians_c.get();
    kb.sh_bytes = pc->sh_bytes.get();
    kb.covars = pc->covars.get();
    kb.splats = sc.splats.get();
    kb.keys = sc.keys_a.get();
    kb.footprints = sc.fpw_a.get();
    kb.src_index = (r->capture || r->contrib) ? sc.src_index.get() : nullptr;
    r->frame.contrib = r->contrib;
    kb.block_status = sc.k1_status.get();
    kb.counters = sc.counters();
    // (the next frames of a traced renderer, as many as it has slots: one slot of four stamps per frame, each used once)
    r->frame.trace_slot = r->trace_count < trace_capacity(r) ? r->frame_trace.get() + (size_t)r->trace_count * 4 : nullptr;
    if (r->frame.trace_slot) ++r->trace_count;
    kb.trace = r->frame.trace_slot;

    // look-back epoch of this frame (lookback.h); on wrap-around the status arrays are re-zeroed
    if (++r->epoch == 0) {
        WS_HIP(hipMemsetAsync(sc.k1_status.get(), 0, sc.k1_status.bytes(), stream));
        WS_HIP(hipMemsetAsync(sc.bin_status.get(), 0, sc.bin_status.bytes(), stream));
        if (sc.fat_status.get()) WS_HIP(hipMemsetAsync(sc.fat_status.get(), 0, sc.fat_status.bytes(), stream));
        r->epoch = 1;
    }
    kp.epoch = r->epoch;
    *kp_out = kp;
    *kb_out = kb;
    return WS_OK;
}

int ws_renderer_prepare(ws_renderer* r, const ws_pointcloud* pc, const ws_splatting_args* args, void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    K1Params kp;
    K1Buffers kb;
    int rc = prepare_setup(r, pc, args, stream, &kp, &kb);
    if (rc) return rc;
    const int cut_mode = r->ctx->debug_cut;
    // A captured frame graph (one hipGraphLaunch + one kernel-argument update instead of 22 launches + a memset on the host)
    // when the caller gave a real stream and no per-launch instrumentation is on.  The legacy NULL stream cannot be captured.
    const bool use_graph = r->ctx->use_graph && stream != nullptr && !r->marks.active && !r->timers && !r->capture &&
                           !r->contrib && cut_mode == 0;
    if (!use_graph) {
        rc = enqueue_frame(r, pc, kp, kb, stream);
        if (rc == WS_OK) r->frame.depth = r->frame.k1_depths != nullptr;
        return rc;
    }
    const FrameGraphKey key{pc, r->scratch_generation, r->order_mode};
    if (!r->fg.matches(key)) {
        renderer_free_graph(r);  // (with it the digit width it kept: this capture's depth sort chooses its own)
        const void* k1_func = preprocess_kernel_func(pc->compressed, r->plan.footprint_mode, r->frame.k1_depths != nullptr);
        WS_TRY(r->fg.capture(key, stream, k1_func, r->plan.depth_digit_bits, [&](FrameArrays* captured) {
            const int erc = enqueue_frame(r, pc, kp, kb, stream);
            if (erc) r->frame = PreparedFrame();
            *captured = r->frame.arrays;
            return erc;
        }));
    }
    // (the DEPTH form of K1 takes the z plane as a third argument; toggling depth re-captures: ws_renderer_enable_depth)
    float* k1_depths = r->frame.k1_depths;
    void* k1_args[3] = {const_cast<K1Params*>(&kp), const_cast<K1Buffers*>(&kb), &k1_depths};
    WS_TRY(r->fg.launch(stream, k1_args, &r->frame.arrays));
    r->frame.depth = r->frame.k1_depths != nullptr;
    return frame_prepared(r, pc, stream);
}

}  // extern "C"

uint32_t ws_internal_renderer_frames_enqueued(const ws_renderer* r) { return r ? r->frames_enqueued : 0u; }
bool ws_internal_renderer_progress(const ws_renderer* r, uint32_t* started_seq) {
    if (!r || !r->mailbox.present()) return false;
    *started_seq = r->mailbox.started_seq();
    return true;
}
void ws_internal_renderer_set_throughput_mode(ws_renderer* r, bool on) {
    if (r) r->throughput_mode = on;
}

uint32_t ws_internal_renderer_demand(const ws_renderer* r) {
    if (!r) return 0u;
    return std::max(r->needed_seen, r->mailbox.demand());
}

// prepare() for a GROUP of renderers drawing different views of ONE scene (a view batch): each renderer's frame runs on
// its own stream as usual, but K1 runs ONCE for the whole group (k_preprocess_multi: the scene is read from HBM once
// instead of once per view), on the first renderer's stream, between "every arena is cleared" and "the rest of every
// frame".  Returns WS_ERR_UNSUPPORTED (nothing enqueued, nothing changed) when the renderers cannot share a launch; the
// caller then prepares them one by one.
int ws_internal_prepare_group(ws_renderer* const* rs, uint32_t n, const ws_pointcloud* pc, const ws_splatting_args* views,
                              hipStream_t const* streams) {
    if (!rs || !pc || !views || !streams || n < 2 || n > (uint32_t)K1_MAX_VIEWS) return WS_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < n; ++i) {
        ws_renderer* r = rs[i];
        if (!r || !streams[i] || r->ctx != rs[0]->ctx || r->compressed != pc->compressed || r->timers || r->marks.active ||
            r->capture || r->contrib || r->depth || r->ctx->use_graph || r->ctx->debug_cut)
            return WS_ERR_UNSUPPORTED;
        for (uint32_t j = 0; j < i; ++j)
            if (rs[j] == r || streams[j] == streams[i]) return WS_ERR_UNSUPPORTED;
        // the only argument check of prepare_setup that answers WS_ERR_UNSUPPORTED: made here, BEFORE any renderer of the
        // group is touched, so that "unsupported" keeps meaning "nothing enqueued, nothing changed" 
        if (views[i].max_sh_deg > 3) return fail(WS_ERR_INVALID, "ws_view_batch_render: max_sh_deg > 3");
    }
    K1Params kp[K1_MAX_VIEWS];
    K1Buffers kb[K1_MAX_VIEWS];
    int rc;
    for (uint32_t i = 0; i < n; ++i) {
        if ((rc = prepare_setup(rs[i], pc, &views[i], streams[i], &kp[i], &kb[i]))) return rc;
        for (int e = 0; e < 2; ++e)
            if (!rs[i]->ev_group[e].get()) WS_TRY(rs[i]->ev_group[e].create(false));
    }
    for (uint32_t i = 1; i < n; ++i)
        if (rs[i]->plan.footprint_mode != rs[0]->plan.footprint_mode) {  // (cannot happen within one batch: same viewport class)
            for (uint32_t k = 0; k < n; ++k)  // fall back in place: the set-up is done, finish every frame on its own
                if ((rc = enqueue_frame(rs[k], pc, kp[k], kb[k], streams[k]))) return rc;
            return WS_OK;
        }
    // every renderer's arena is cleared on its own stream (behind its previous frame); the shared K1 waits for all of them
    for (uint32_t i = 0; i < n; ++i) {
        if ((rc = enqueue_frame(rs[i], pc, kp[i], kb[i], streams[i], FRAME_CLEAR))) return rc;
        if (i > 0) {
            WS_HIP(hipEventRecord(rs[i]->ev_group[0].get(), streams[i]));
            WS_HIP(hipStreamWaitEvent(streams[0], rs[i]->ev_group[0].get(), 0));
        }
    }
    if ((rc = launch_preprocess_multi(kp, kb, n, pc->compressed, rs[0]->plan.footprint_mode, streams[0]))) return rc;
    WS_HIP(hipEventRecord(rs[0]->ev_group[1].get(), streams[0]));
    // (Measured and removed: starting the frames of a group one after another behind events, so that they do not run the
    // same stage in lock-step -- 3781 instead of 5155 frames/s; every cross-stream wait costs more than the lock-step does.)
    for (uint32_t i = 0; i < n; ++i) {
        if (i > 0) WS_HIP(hipStreamWaitEvent(streams[i], rs[0]->ev_group[1].get(), 0));
        if ((rc = enqueue_frame(rs[i], pc, kp[i], kb[i], streams[i], FRAME_REST))) return rc;
    }
    return WS_OK;
}

extern "C" {

// render(), render_aux() and render_composite(): planes == nullptr and comp == nullptr is the colour image alone over the
// background (the launch render() has always made)
static int render_frame(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba_out,
                        size_t row_pitch_bytes, void* stream_v, const BlendAuxPlanes* planes,
                        const BlendComposite* comp = nullptr) {
    if (!r || !pc || !d_rgba_out) return fail(WS_ERR_INVALID, "ws_renderer_render: null argument");
    if (!r->frame.prepared || r->frame.pc != pc)
        return fail(WS_ERR_STATE, "ws_renderer_render: prepare() was not called for this point cloud");
    const size_t texel = r->format == WS_FORMAT_RGBA8_UNORM ? 4 : (r->format == WS_FORMAT_RGBA16_FLOAT ? 8 : 16);
    if (row_pitch_bytes < texel * r->vw || (row_pitch_bytes % texel) != 0 ||
        (reinterpret_cast<uintptr_t>(d_rgba_out) % texel) != 0)
        return fail(WS_ERR_INVALID, "ws_renderer_render: row pitch / alignment does not fit the colour format");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    BlendFrameRequest fr{};
    fr.target_precision = r->blend_mode == WS_BLEND_TARGET_PRECISION, fr.exact_mode = r->blend_mode == WS_BLEND_FAST_EXACT_CUT;
    fr.variant = r->ctx->blend_variant, fr.capture = r->capture, fr.timing = r->blend_timing;
    fr.split_wanted = r->plan.split_wanted;
    fr.order_valid = r->frame.arrays.blend_order_valid, fr.qw = r->ctx->tile_qw, fr.qh = r->ctx->tile_qh;
    const BlendFrameChoice form = blend_frame_choice(fr);
    BlendParams bp;
    bp.splats = r->scratch.splats.get();
    bp.entry_vals = r->frame.arrays.entries;
    bp.tile_ranges = r->scratch.tile_ranges();
    bp.width = r->vw;
    bp.height = r->vh;
    bp.tiles_x = r->plan.tiles_x;
    bp.tiles_y = r->plan.tiles_y;
    bp.qw = r->ctx->tile_qw;
    bp.qh = r->ctx->tile_qh;
    for (int i = 0; i < 4; ++i) bp.background[i] = background ? background[i] : 0.0f;
    bp.out = d_rgba_out;
    bp.pitch = row_pitch_bytes;
    bp.format = (int)r->format;
    bp.tpw_log2 = r->ctx->blend_tpw_log2;
    bp.lds_pad_kb = r->ctx->blend_lds_pad_kb;
    bp.dma = r->ctx->blend_dma;
    bp.exact_cut = form.exact_cut ? 1 : 0;
    bp.async_staging = r->ctx->blend_async < 0 ? WS_BLEND_ASYNC_DEFAULT : (r->ctx->blend_async ? 1 : 0);
    bp.num_cus = r->ctx->num_cus;
    bp.range_row_shift = 0;
    bp.bin_tiles_x = r->plan.tiles_x;
    if (form.split) {
        bp.qh = 2;
        bp.tiles_y = (r->vh + 15u) / 16u;
        bp.range_row_shift = 1;
    }
    bp.counters = r->scratch.counters();
    bp.sticky = r->sticky.get();
    bp.demand_mailbox = r->mailbox.dev();
    bp.progress_mailbox = r->mailbox.dev() ? r->mailbox.dev() + 1 : nullptr;
    bp.frame_seq = r->frames_enqueued + 1u;  // (counted below, once the launch is certain)
    bp.order = form.ordered ? r->scratch.blend_order.get() : nullptr;
    bp.debug_consumed = r->capture ? r->scratch.debug_consumed.get() : nullptr;
    bp.debug_walked = r->capture ? r->scratch.debug_walked.get() : nullptr;
    bp.debug_timing = nullptr;
    bp.trace = r->frame.trace_slot ? r->frame.trace_slot + 2 : nullptr;
    if (r->blend_timing && !r->capture) {
        DeviceBuf<uint32_t>& timing = r->scratch.debug_timing;  // (allocated on first use, freed with the scratch)
        if (!timing.get()) {
            WS_HIP(hipStreamSynchronize(stream));
            WS_TRY(timing.alloc(r->scratch.layout.debug_timing));
        }
        WS_HIP(hipMemsetAsync(timing.get(), 0, timing.bytes(), stream));
        bp.debug_timing = timing.get();
    }
    if (bp.debug_consumed) {
        WS_HIP(hipMemsetAsync(r->scratch.debug_consumed.get(), 0, r->scratch.debug_consumed.bytes(), stream));
        WS_HIP(hipMemsetAsync(r->scratch.debug_walked.get(), 0, r->scratch.debug_walked.bytes(), stream));
    }
    KernelMarks* km = r->marks.active ? &r->marks : nullptr;
    if (km) km->begin(stream, false);
    if (r->timers) WS_HIP(hipEventRecord(r->ev[4].get(), stream));
    if (r->ctx->debug_cut >= 1 && r->ctx->debug_cut <= 4) return WS_OK;  // analysis only
    int rc = launch_blend(bp, form.variant, stream, planes, comp);
    if (rc) return rc;
    r->frames_enqueued = bp.frame_seq;
    km_mark(km, fr.target_precision ? "k_blend_strict" : "k_blend");
    if (r->timers) {
        WS_HIP(hipEventRecord(r->ev[5].get(), stream));
        r->ev_render_valid = true;
    }
    r->last_stream = stream;
    return WS_OK;
}

int ws_renderer_render(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba_out,
                       size_t row_pitch_bytes, void* stream_v) {
    return render_frame(r, pc, background, d_rgba_out, row_pitch_bytes, stream_v, nullptr);
}

int ws_renderer_enable_depth(ws_renderer* r, int enable) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_depth: null renderer");
    if (r->depth != (enable != 0)) {
        r->depth = enable != 0;
        // K1's other form: a captured frame graph holds the old one (and its argument list) -- the next prepare() captures anew
        ++r->scratch_generation;
    }
    return WS_OK;
}

// What the entry points know of "the FAST production launch" before a frame is enqueued (the blend mode is theirs to check;
// the launcher adds the launch's own switches)
static bool production_launch(const ws_renderer* r) {
    BlendLaunchMode m{};
    m.capture = r->capture, m.timing = r->blend_timing, m.dma = r->ctx->blend_dma, m.variant = r->ctx->blend_variant, m.debug_cut = r->ctx->debug_cut;
    return blend_production_launch(m);
}

// The checks of render_aux() on a ws_aux_targets with at least one plane; fills *bp (z: the frame's plane, if it has one).
static int aux_planes_of(ws_renderer* r, const ws_pointcloud* pc, const ws_aux_targets* aux, BlendAuxPlanes* bp) {
    for (int i = 0; i < 4; ++i)
        if (aux->reserved[i]) return fail(WS_ERR_INVALID, "ws_renderer_render_aux: reserved words must be zero");
    const size_t row = (size_t)4 * r->vw;
    const struct { const float* p; size_t pitch; } planes[3] = {{aux->depth, aux->depth_pitch}, {aux->median_depth, aux->median_depth_pitch},
                                                                 {aux->alpha, aux->alpha_pitch}};
    for (const auto& pl : planes)
        if (pl.p && (pl.pitch < row || (pl.pitch % 4) != 0 || (reinterpret_cast<uintptr_t>(pl.p) % 4) != 0))
            return fail(WS_ERR_INVALID, "ws_renderer_render_aux: plane pitch below 4 x width, or pitch / pointer not 4-B aligned");
    if (r->blend_mode != WS_BLEND_FAST)
        return fail(WS_ERR_UNSUPPORTED, "ws_renderer_render_aux: auxiliary planes need WS_BLEND_FAST");
    if (!production_launch(r))
        return fail(WS_ERR_UNSUPPORTED, "ws_renderer_render_aux: auxiliary planes need the production blend (no capture / timing / variants)");
    if (r->frame.prepared && r->frame.pc == pc && (aux->depth || aux->median_depth) && !r->frame.depth)
        return fail(WS_ERR_STATE, "ws_renderer_render_aux: depth planes need ws_renderer_enable_depth before prepare()");
    bp->depth = aux->depth;
    bp->depth_pitch = aux->depth_pitch;
    bp->median = aux->median_depth;
    bp->median_pitch = aux->median_depth_pitch;
    bp->alpha = aux->alpha;
    bp->alpha_pitch = aux->alpha_pitch;
    bp->z = r->frame.depth ? r->scratch.depths.get() : nullptr;
    return WS_OK;
}

int ws_renderer_render_aux(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba_out,
                           size_t row_pitch_bytes, const ws_aux_targets* aux, void* stream) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_render_aux: null renderer");
    if (!aux || (!aux->depth && !aux->median_depth && !aux->alpha))
        return render_frame(r, pc, background, d_rgba_out, row_pitch_bytes, stream, nullptr);
    BlendAuxPlanes bp;
    const int rc = aux_planes_of(r, pc, aux, &bp);
    if (rc) return rc;
    return render_frame(r, pc, background, d_rgba_out, row_pitch_bytes, stream, &bp);
}

int ws_renderer_render_composite(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba,
                                 size_t row_pitch_bytes, const ws_aux_targets* aux, const ws_composite_desc* comp,
                                 void* stream) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_render_composite: null renderer");
    if (comp) {
        for (int i = 0; i < 4; ++i)
            if (comp->reserved[i]) return fail(WS_ERR_INVALID, "ws_renderer_render_composite: reserved words must be zero");
        if (comp->load > 1u) return fail(WS_ERR_INVALID, "ws_renderer_render_composite: load is 0 or 1");
        if (comp->occluder_kind != WS_OCCLUDER_VIEW_Z && comp->occluder_kind != WS_OCCLUDER_NDC_DEPTH)
            return fail(WS_ERR_INVALID, "ws_renderer_render_composite: unknown occluder kind");
        if (comp->occluder && (comp->occluder_pitch < (size_t)4 * r->vw || (comp->occluder_pitch % 4) != 0 ||
                               (reinterpret_cast<uintptr_t>(comp->occluder) % 4) != 0))
            return fail(WS_ERR_INVALID, "ws_renderer_render_composite: occluder pitch below 4 x width, or pitch / pointer not 4-B aligned");
    }
    // no composite asked for: render_aux (the same launch, the same bytes)
    if (!comp || (!comp->load && !comp->occluder))
        return ws_renderer_render_aux(r, pc, background, d_rgba, row_pitch_bytes, aux, stream);
    if (r->blend_mode == WS_BLEND_FAST_EXACT_CUT)
        return fail(WS_ERR_UNSUPPORTED, "ws_renderer_render_composite: load / occluder need WS_BLEND_FAST or WS_BLEND_TARGET_PRECISION");
    if (!production_launch(r))
        return fail(WS_ERR_UNSUPPORTED, "ws_renderer_render_composite: load / occluder need the production blend (no capture / timing / variants)");
    BlendAuxPlanes bp = {};
    if (aux && (aux->depth || aux->median_depth || aux->alpha)) {
        const int rc = aux_planes_of(r, pc, aux, &bp);
        if (rc) return rc;
    }
    if (comp->occluder && r->frame.prepared && r->frame.pc == pc && !r->frame.depth)
        return fail(WS_ERR_STATE, "ws_renderer_render_composite: an occluder needs ws_renderer_enable_depth before prepare()");
    bp.z = r->frame.depth ? r->scratch.depths.get() : nullptr;
    BlendComposite c;
    c.occluder = comp->occluder;
    c.occluder_pitch = comp->occluder_pitch;
    c.znear = r->frame.znear;
    c.zfar = r->frame.zfar;
    c.occ_ndc = comp->occluder_kind == WS_OCCLUDER_NDC_DEPTH ? 1 : 0;
    c.load = comp->load ? 1 : 0;
    return render_frame(r, pc, background, d_rgba, row_pitch_bytes, stream, &bp, &c);
}

}  // extern "C"
