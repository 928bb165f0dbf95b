// ws_api.cpp -- the C ABI (include/websplat.h): handles, device memory, frame orchestration.  The passes that only read a
// prepared frame, and the objects they fill, are in api_attrib.cpp, api_metrics.cpp and api_refit.cpp (shared state: api_state.h).
//
// Mirrors the reference's object model: WGPUContext (lib.rs:57-125) -> ws_context,
// PointCloud (pointcloud.rs:72-222) -> ws_pointcloud, GaussianRenderer (renderer.rs:17-283) -> ws_renderer,
// GPURSSorter + PointCloudSortStuff (gpu_rs.rs:23-175, 865-884) -> ws_sorter.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_state.h"
#include "contrib.h"
#include "ply_encode.h"

namespace ws {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? WS_ERR_OOM : WS_ERR_HIP;
}

// The runtime behind every DeviceBuf (device_buf.h).  The text of a failure is the one this library's allocations have always given.
int device_alloc(void** p, size_t bytes) {
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? WS_OK : hip_fail(e, "hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T))");
}
void device_free(void* p) { (void)hipFree(p); }
// ... under the name an entry point gives its uploads ("ws_pointcloud_create: upload: out of memory"): hip_fail's "what: why"
static int alloc_as(int rc, const char* what) {
    if (rc) g_last_error.replace(0, g_last_error.rfind(": "), what);
    return rc;
}

int KernelMarks::create() {
    if (created) return WS_OK;
    for (auto& e : ev) WS_HIP(hipEventCreate(&e));
    created = true;
    return WS_OK;
}
void KernelMarks::destroy() {
    if (!created) return;
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    created = false;
}
void KernelMarks::begin(hipStream_t s, bool restart) {
    stream = s;
    if (restart) n = 0;
    // render() continues the frame prepare() started: ev[n] already closes the previous interval
    if (n == 0) (void)hipEventRecord(ev[0], s);
}
void KernelMarks::mark(const char* what) {
    if (n >= MAX) return;
    label[n] = what;
    (void)hipEventRecord(ev[n + 1], stream);
    ++n;
}

}  // namespace ws

using namespace ws;

// depth sort of a context that does not say otherwise (WS_DEPTH_SORT): decided by measurement, profiles/r04/
#ifndef WS_DEPTH_SORT_DEFAULT
#define WS_DEPTH_SORT_DEFAULT DS_SCAN
#endif

// small per-sort zero arena of a stand-alone sorter: tickets, error word, digit histograms, the depth sort's key-range fold
struct SorterZero {
    uint32_t tickets[4];
    uint32_t error;
    uint32_t _pad[3];
    uint32_t hist[4 * 512];                                  // (rows of 512: 9-bit digits; 8-bit digits use the first 256)
    uint32_t fat_barrier[9 * 16];                            // single-launch depth sort: barrier state
    FrameCounters counters;                                  // ws_sorter_sort_depth: the range report and decision (depth_range_decide)
};

struct ws_sorter {
    ws_context* ctx = nullptr;
    DeviceBuf<uint32_t> keys_alt, vals_alt, aux_alt, tile_sums;  // ping-pong partners [max_n + 4] and the count rows
    DeviceBuf<SorterZero> zero;
    DeviceBuf<uint64_t> fat_status;  // a context whose depth sort is the fat-tile one-sweep: its chunk-count rows
    SortScratch sc;        // what the launchers take: views of the buffers above
    FatSortScratch fat;
    uint32_t epoch = 0;
    bool folded = false;              // the last ws_sorter_sort_depth folded the key range (ws_sorter_depth_range)
    hipStream_t last_stream = nullptr;
};

// FrameCounters::depth_span_class of the renderer's last frame whose blend has started: the blend posts it to pinned memory,
// read here without a sync (0: none yet, or no mailbox)
static uint32_t renderer_span_class(const ws_renderer* r) {
    return r->demand_mailbox ? *reinterpret_cast<volatile const uint32_t*>(r->demand_mailbox + 2) : 0u;
}

// Frees the captured frame graph.  The depth sort's digit width is the plan's one rule that reads the graph (a valid graph keeps
// the width it was captured with): it is asked again, so that a plan made while the graph stood chooses its own width.
static void renderer_free_graph(ws_renderer* r) {
    ws_renderer::FrameGraph& g = r->fg;
    for (int i = 0; i < ws_renderer::GRAPH_RING; ++i) {
        if (g.exec[i]) (void)hipGraphExecDestroy(g.exec[i]);
        if (g.done[i]) (void)hipEventDestroy(g.done[i]);
    }
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g = ws_renderer::FrameGraph();
    r->plan.depth_digit_bits = depth_sort_digit_bits(r->ctx->depth_digit_bits, r->ctx->depth_skip_top != 0, renderer_span_class(r), 0);
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
        if (r->demand_mailbox) {
            WS_HIP(hipDeviceSynchronize());
            *reinterpret_cast<volatile uint32_t*>(r->demand_mailbox) = 0u;
            WS_HIP(hipMemset(r->sticky.get() + 1, 0, sizeof(uint32_t)));
        }
    } else if (r->demand_mailbox) {
        const uint32_t posted = *reinterpret_cast<volatile uint32_t*>(r->demand_mailbox);
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

const char* ws_last_error(void) { return g_last_error.c_str(); }
uint32_t ws_abi_version(void) { return WS_ABI_VERSION; }
uint32_t ws_build_flags(void) {
#ifdef WS_EXPERIMENTAL
    return WS_BUILD_EXPERIMENTAL;
#else
    return 0u;
#endif
}

// ---- context ---------------------------------------------------------------------------------------
void ws_context_config_init(ws_context_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->depth_skip_top = 1;
    c->blend_order = -1;
    c->blend_split = -1;
    c->bin_request = BIN_AUTO;
    c->batch_threads = -1;
    c->batch_queue_depth = -1;
    c->blend_tpw_log2 = -1;
    c->tile_qw = c->tile_qh = 4;
    c->exp_batch_k1 = 1;
    c->blend_async = -1;
}

int ws_context_create(int hip_device, ws_context** out) {
    ws_context_config c;
    ws_context_config_init(&c);
    return ws_context_create_with_config(hip_device, &c, out);
}

// The library reads NO environment variable (round 6; verdict r05 "a drop-in library steered by the environment of whoever loads
// it"): every switch arrives in the config.  bench.py / the tests / the tools translate their WS_* environment outside.
int ws_context_create_with_config(int hip_device, const ws_context_config* cfg_in, ws_context** out) {
    if (!out) return fail(WS_ERR_INVALID, "ws_context_create: out is null");
    *out = nullptr;
    ws_context_config cfg;
    ws_context_config_init(&cfg);
    if (cfg_in) {  // a caller built against an older (shorter) struct: its fields, our defaults for the rest
        if (cfg_in->struct_size < 8u || cfg_in->struct_size > 4096u)
            return fail(WS_ERR_INVALID, "ws_context_create_with_config: struct_size is not set (ws_context_config_init)");
        std::memcpy(&cfg, cfg_in, cfg_in->struct_size < sizeof cfg ? cfg_in->struct_size : sizeof cfg);
        cfg.struct_size = (uint32_t)sizeof cfg;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        (void)hipGetLastError();
        return fail(WS_ERR_HIP, "ws_context_create: no HIP device available (this library has no CPU fallback)");
    }
    if (hip_device < 0 || hip_device >= count) return fail(WS_ERR_INVALID, "ws_context_create: bad device index");
    if (!((cfg.tile_qw == 2 && cfg.tile_qh == 2) || (cfg.tile_qw == 4 && cfg.tile_qh == 2) || (cfg.tile_qw == 4 && cfg.tile_qh == 4)))
        return fail(WS_ERR_INVALID, "ws_context_config: tile_qw x tile_qh must be 2x2, 4x2 or 4x4");
    if (cfg.bin_request < (int)BIN_NEVER || cfg.bin_request > (int)BIN_ALWAYS)
        return fail(WS_ERR_INVALID, "ws_context_config: bin_request must be 0 (never), 1 (per frame on the device) or 2 (always)");
    if (cfg.depth_digit_bits != 0 && cfg.depth_digit_bits != 8 && cfg.depth_digit_bits != 9)
        return fail(WS_ERR_INVALID, "ws_context_config: depth_digit_bits must be 0 (default), 8 or 9");
    WS_HIP(hipSetDevice(hip_device));
    ws_context* ctx = new (std::nothrow) ws_context();
    if (!ctx) return fail(WS_ERR_OOM, "ws_context_create: host allocation failed");
    ctx->device = hip_device;
    WS_HIP(hipGetDeviceProperties(&ctx->props, hip_device));
    ctx->depth_sort_mode = WS_DEPTH_SORT_DEFAULT;
    // ---- measured-and-lost variants (DESIGN_LOG.md): compiled only into the EXPERIMENTAL build (make experimental ->
    // lib_exp/libwebsplat_hip.so, -DWS_EXPERIMENTAL), which the variant tests load; the product library refuses their switches
    // loudly instead of carrying their kernels ------------------------------------------------------------------------
#ifdef WS_EXPERIMENTAL
    ctx->tile_sort_wide = cfg.exp_tile_sort_wide != 0;
    if (cfg.exp_depth_sort == 1) ctx->depth_sort_mode = DS_ONESWEEP;
    else if (cfg.exp_depth_sort == 2) ctx->depth_sort_mode = DS_COOP;
    ctx->dsort_fat_grid = cfg.exp_dsort_fat_grid;
    ctx->blend_variant = cfg.exp_blend_variant;
    ctx->blend_dma = cfg.exp_blend_dma ? 1 : 0;
    ctx->batch_k1 = cfg.exp_batch_k1;
    if (ctx->batch_k1 < 1 || ctx->batch_k1 > K1_MAX_VIEWS) ctx->batch_k1 = 1;
    ctx->footprint = cfg.exp_footprint_ellipse ? FP_ELLIPSE : FP_RECT_PACKED;
#else
    if (cfg.exp_depth_sort || cfg.exp_blend_variant || cfg.exp_blend_dma || cfg.exp_batch_k1 != 1 || cfg.exp_footprint_ellipse ||
        cfg.exp_tile_sort_wide || cfg.blend_async > 0) {
        delete ctx;
        return fail(WS_ERR_UNSUPPORTED, "ws_context_create: exp_depth_sort, exp_blend_variant, exp_blend_dma, "
                                        "exp_batch_k1, exp_footprint_ellipse, exp_tile_sort_wide and blend_async = 1 select measured-and-lost variants that are only in "
                                        "the experimental build (make -C web-splat_amd experimental; WEBSPLAT_LIB=.../lib_exp/libwebsplat_hip.so)");
    }
#endif
    ctx->debug_cut = cfg.debug_cut;  // analysis only: stop the frame after stage n (1 = K1 ... 4 = tile sort)
    ctx->blend_tpw_log2 = cfg.blend_tpw_log2 > 4 ? 4 : cfg.blend_tpw_log2;
    ctx->use_graph = cfg.use_graph;
    ctx->depth_skip_top = cfg.depth_skip_top;  // 0: the depth sort always runs all of its passes (A/B)
    // the blend's workgroups: -1 (default) longest list first for a renderer that draws one frame at a time, image order for
    // the slots of a view batch with frames in flight (ws_renderer_render); 0 / 1 force image order / longest first;
    // 2 (shortest first) and 3 (alternating) are the measured experiments of DESIGN 3.3
    ctx->blend_order = cfg.blend_order;
    ctx->blend_split = cfg.blend_split;  // -1 = automatic (ws_renderer_render)
    ctx->bin_request = cfg.bin_request;  // binning at twice the blend's tile size: never | per frame on the device | always
    ctx->batch_threads = cfg.batch_threads;
    ctx->batch_queue_depth = cfg.batch_queue_depth;
    ctx->num_cus = ctx->props.multiProcessorCount > 0 ? ctx->props.multiProcessorCount : 256;
    ctx->blend_lds_pad_kb = (cfg.blend_lds_pad_kb < 0 || cfg.blend_lds_pad_kb > 96) ? 0 : cfg.blend_lds_pad_kb;
    ctx->tile_qw = (uint32_t)cfg.tile_qw;
    ctx->tile_qh = (uint32_t)cfg.tile_qh;
    ctx->capture = cfg.capture != 0;
    ctx->render_views_fast_blend = cfg.render_views_fast_blend != 0;
    ctx->ply_decode_host = cfg.ply_decode_host != 0;
    ctx->depth_digit_bits = cfg.depth_digit_bits;
    ctx->blend_async = cfg.blend_async;
    ctx->depth_tile_kpt = (cfg.depth_tile_kpt == 4 || cfg.depth_tile_kpt == 8) ? cfg.depth_tile_kpt : 0;
    *out = ctx;
    return WS_OK;
}

void ws_context_destroy(ws_context* ctx) { delete ctx; }

int ws_context_tile_size(const ws_context* ctx, uint32_t* width, uint32_t* height) {
    if (!ctx || !width || !height) return fail(WS_ERR_INVALID, "ws_context_tile_size: null argument");
    *width = QUAD * ctx->tile_qw;
    *height = QUAD * ctx->tile_qh;
    return WS_OK;
}

int ws_debug_stage_splat(const uint32_t splat[5], float viewport_w, float viewport_h, float tile_x0, float tile_y0,
                         uint32_t tile_w, uint32_t tile_h, float rec[10], uint32_t* quadrant_mask) {
    if (!splat || !rec || !quadrant_mask) return fail(WS_ERR_INVALID, "ws_debug_stage_splat: null argument");
    return debug_stage_splat(splat, viewport_w, viewport_h, tile_x0, tile_y0, tile_w / QUAD, tile_h / QUAD, rec,
                             quadrant_mask);
}

int ws_debug_packed_rect(uint32_t rect, uint32_t* tiles, uint32_t* tiles_coarse, uint32_t* rect_coarse_out) {
    if (!tiles || !tiles_coarse || !rect_coarse_out) return fail(WS_ERR_INVALID, "ws_debug_packed_rect: null argument");
    *tiles = rect_tiles(rect);
    *tiles_coarse = rect_tiles64(rect);
    *rect_coarse_out = rect == RECT_EMPTY ? RECT_EMPTY : rect_coarse(rect);
    return WS_OK;
}

int ws_debug_binning_decision(uint32_t request, const uint32_t* sums, const uint32_t* sums_coarse, uint32_t nslots,
                              uint32_t* shift) {
    if (!shift || (nslots && (!sums || !sums_coarse))) return fail(WS_ERR_INVALID, "ws_debug_binning_decision: null argument");
    if (nslots > (uint32_t)TILE_SUM_SLOTS || request > (uint32_t)BIN_ALWAYS)
        return fail(WS_ERR_INVALID, "ws_debug_binning_decision: at most 16 slots, request 0..2");
    FrameCounters fc;
    std::memset(&fc, 0, sizeof fc);
    fc.bin_request = request;
    for (uint32_t i = 0; i < nslots; ++i) {
        fc.tile_sums[i * TILE_SUM_STRIDE] = sums[i];
        fc.tile_sums[i * TILE_SUM_STRIDE + 1] = sums_coarse[i];
    }
    *shift = bin_shift_decide(&fc);
    return WS_OK;
}

int ws_debug_depth_range(uint32_t key_min, uint32_t key_max, int have_keys, uint32_t digits, uint32_t* base, uint32_t* skip,
                         uint32_t* span_class) {
    if (!base || !skip || !span_class || (digits != 256u && digits != 512u))
        return fail(WS_ERR_INVALID, "ws_debug_depth_range: null argument, or a radix other than 256 / 512");
    FrameCounters fc;
    std::memset(&fc, 0, sizeof fc);
    if (have_keys) {  // what the sort's first histogram kernel leaves in one slot: max(~key) and max(key)
        fc.tile_sums[5 * TILE_SUM_STRIDE + 2] = ~key_min;
        fc.tile_sums[5 * TILE_SUM_STRIDE + 3] = key_max;
    }
    depth_range_decide(&fc, digits);
    *base = fc.depth_key_base;
    *skip = fc.depth_skip_top;
    *span_class = fc.depth_span_class;
    return WS_OK;
}

int ws_debug_depth_fold(const uint32_t* keys, uint32_t count, uint32_t tile_n, uint32_t digits, uint32_t* base, uint32_t* skip,
                        uint32_t* span_class) {
    if (!base || !skip || !span_class || (count && !keys) || tile_n == 0 || (digits != 256u && digits != 512u))
        return fail(WS_ERR_INVALID, "ws_debug_depth_fold: null argument, a tile of no keys, or a radix other than 256 / 512");
    FrameCounters fc;
    std::memset(&fc, 0, sizeof fc);
    // what the depth sort's first histogram kernel does per sort tile: max(~key) and max(key) over its valid keys, reported by
    // the shared rule into slot t & 15 (k_sort_tile_hist, k_dsort9_tile_hist)
    for (uint32_t t = 0; (uint64_t)t * tile_n < count; ++t) {
        const uint32_t b = t * tile_n, e = (uint64_t)b + tile_n < count ? b + tile_n : count;
        uint32_t knmin = 0u, kmax = 0u;
        for (uint32_t i = b; i < e; ++i) {
            knmin = std::max(knmin, ~keys[i]);
            kmax = std::max(kmax, keys[i]);
        }
        if (depth_tile_reports(knmin, kmax)) {
            uint32_t* ts = depth_range_slot(&fc, t);
            ts[2] = std::max(ts[2], knmin);
            ts[3] = std::max(ts[3], kmax);
        }
    }
    depth_range_decide(&fc, digits);
    *base = fc.depth_key_base;
    *skip = fc.depth_skip_top;
    *span_class = fc.depth_span_class;
    return WS_OK;
}

int ws_debug_footprint(const uint32_t splat[3], float viewport_w, float viewport_h, uint32_t tile_w, uint32_t tile_h,
                       uint32_t capacity, uint32_t* tiles, uint32_t* count) {
    if (!splat || !count || (capacity && !tiles)) return fail(WS_ERR_INVALID, "ws_debug_footprint: null argument");
    if ((tile_w != 16 && tile_w != 32) || (tile_h != 16 && tile_h != 32) || !(viewport_w >= 1.0f) || !(viewport_h >= 1.0f))
        return fail(WS_ERR_INVALID, "ws_debug_footprint: tile size must be 16 or 32 per axis, the viewport at least one pixel");
    const uint32_t twl = tile_w == 32 ? 5u : 4u, thl = tile_h == 32 ? 5u : 4u;
    const uint32_t tiles_x = ((uint32_t)viewport_w + tile_w - 1) / tile_w;
    return debug_footprint(splat, viewport_w, viewport_h, twl, thl, tiles_x, capacity, tiles, count);
}

int ws_sync(ws_context* ctx, void* stream) {
    if (!ctx) return fail(WS_ERR_INVALID, "ws_sync: null context");
    WS_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return WS_OK;
}

int ws_context_set_host_wait(ws_context* ctx, ws_host_wait mode) {
    if (!ctx) return fail(WS_ERR_INVALID, "ws_context_set_host_wait: null context");
    if (mode != WS_HOST_WAIT_SPIN && mode != WS_HOST_WAIT_BLOCK) return fail(WS_ERR_INVALID, "ws_context_set_host_wait: unknown mode");
    WS_HIP(hipSetDevice(ctx->device));
    WS_HIP(hipSetDeviceFlags(mode == WS_HOST_WAIT_BLOCK ? hipDeviceScheduleBlockingSync : hipDeviceScheduleSpin));
    return WS_OK;
}

int ws_device_info(ws_context* ctx, char* name, size_t name_len, uint32_t* num_cus, uint64_t* hbm_bytes) {
    if (!ctx) return fail(WS_ERR_INVALID, "ws_device_info: null context");
    if (name && name_len) {
        std::strncpy(name, ctx->props.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (num_cus) *num_cus = (uint32_t)ctx->props.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)ctx->props.totalGlobalMem;
    return WS_OK;
}

int ws_device_malloc(ws_context* ctx, size_t bytes, void** d_ptr) {
    if (!ctx || !d_ptr) return fail(WS_ERR_INVALID, "ws_device_malloc: null argument");
    WS_HIP(hipMalloc(d_ptr, bytes ? bytes : 1));
    return WS_OK;
}
int ws_device_free(ws_context* ctx, void* d_ptr) {
    if (!ctx) return fail(WS_ERR_INVALID, "ws_device_free: null context");
    if (d_ptr) WS_HIP(hipFree(d_ptr));
    return WS_OK;
}
int ws_memcpy_h2d(ws_context* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream) {
    if (!ctx || (!d_dst && bytes) || (!h_src && bytes)) return fail(WS_ERR_INVALID, "ws_memcpy_h2d: null argument");
    WS_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    WS_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return WS_OK;
}
int ws_memcpy_d2h(ws_context* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream) {
    if (!ctx || (!h_dst && bytes) || (!d_src && bytes)) return fail(WS_ERR_INVALID, "ws_memcpy_d2h: null argument");
    WS_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    WS_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return WS_OK;
}

// ---- PointCloud --------------------------------------------------------------------------------------
// what a descriptor says about how its scene wants to be drawn
static void set_render_hints(PointCloudMeta* pc, const ws_pointcloud_desc* d) {
    pc->has_mip = d->has_mip_splatting != 0;
    pc->mip = d->mip_splatting != 0;
    pc->has_kernel_size = d->has_kernel_size != 0;
    pc->kernel_size = d->kernel_size;
    pc->has_background = d->has_background_color != 0;
    std::memcpy(pc->background, d->background_color, sizeof pc->background);
}
int ws_pointcloud_create(ws_context* ctx, const ws_pointcloud_desc* d, ws_pointcloud** out) {
    if (!ctx || !d || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create: null argument");
    *out = nullptr;
    if (d->sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create: sh_deg > 3");
    const uint32_t n = d->num_points;
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create: empty point cloud");
    if (n >= (1u << 30)) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create: more than 2^30-1 points");
    if (!d->gaussians || !d->sh_coefs) return fail(WS_ERR_INVALID, "ws_pointcloud_create: missing buffers");
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create: host allocation failed");
    pc->ctx = ctx;
    pc->num_points = n;
    pc->sh_deg = d->sh_deg;
    pc->compressed = d->compressed != 0;
    pc->bbox = d->bbox;
    std::memcpy(pc->center, d->center, sizeof pc->center);
    pc->has_up = d->has_up != 0;
    std::memcpy(pc->up, d->up, sizeof pc->up);
    set_render_hints(pc.get(), d);
    if (!pc->compressed) {
        if (d->gaussians_bytes != (size_t)n * 28 || d->sh_coefs_bytes != (size_t)n * 96)
            return fail(WS_ERR_INVALID, "ws_pointcloud_create: expected 28 B Gaussians and 96 B SH records");
        // re-lay the loader's AoS records as eight planes of 16-B chunks (ws_internal.h)
        std::vector<uint32_t> staging;
        try {
            staging.resize((size_t)n * PC_PLANES * 4);
        } catch (...) {
            return fail(WS_ERR_OOM, "ws_pointcloud_create: host staging allocation failed");
        }
        const uint8_t* g = static_cast<const uint8_t*>(d->gaussians);
        const uint8_t* s = static_cast<const uint8_t*>(d->sh_coefs);
        uint32_t* st = staging.data();
        const ws::OmpQuietWorkers omp_quiet;  // (ws_internal.h: the region's workers sleep at once instead of spinning 200 ms)
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)n; ++i) {
            const uint8_t* gi = g + (size_t)i * 28;
            uint32_t* p0 = st + ((size_t)0 * n + i) * 4;
            std::memcpy(p0, gi, 16);  // x, y, z, opacity f16 | pad
            uint32_t* p1 = st + ((size_t)1 * n + i) * 4;
            std::memcpy(p1, gi + 16, 12);  // cov f16 x 6
            p1[3] = 0u;
            const uint8_t* si = s + (size_t)i * 96;
            for (int q = 0; q < 6; ++q) std::memcpy(st + ((size_t)(2 + q) * n + i) * 4, si + q * 16, 16);
        }
        WS_TRY(alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), "ws_pointcloud_create: upload"));
        const hipError_t e = hipMemcpy(pc->planes.get(), st, pc->planes.bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "ws_pointcloud_create: upload");
    } else {
        const uint32_t ncoef = (d->sh_deg + 1) * (d->sh_deg + 1);
        if (d->gaussians_bytes != (size_t)n * 24 || !d->covars || !d->quantization || (d->covars_bytes % 12) != 0 ||
            (d->sh_coefs_bytes % (3 * ncoef)) != 0)
            return fail(WS_ERR_INVALID, "ws_pointcloud_create: compressed layout mismatch (24 B splats, 12 B covars, "
                                        "3*(deg+1)^2 B SH records, quantization block)");
        // the kernel indexes covars / SH records with the per-Gaussian indices: validate them on the host,
        // where WebGPU would have clamped out-of-bounds reads
        const uint8_t* g = static_cast<const uint8_t*>(d->gaussians);
        const uint32_t n_cov = (uint32_t)(d->covars_bytes / 12), n_sh = (uint32_t)(d->sh_coefs_bytes / (3 * ncoef));
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t gi, si;
            std::memcpy(&gi, g + (size_t)i * 24 + 16, 4);
            std::memcpy(&si, g + (size_t)i * 24 + 20, 4);
            if (gi >= n_cov || si >= n_sh) return fail(WS_ERR_INVALID, "ws_pointcloud_create: geometry_idx / sh_idx out of range");
        }
        pc->quant = *d->quantization;
        // (the index check above has seen n_cov >= 1: no codebook is empty)
        const char* what = "ws_pointcloud_create: upload (compressed)";
        WS_TRY(alloc_as(pc->gaussians_c.alloc(d->gaussians_bytes), what));
        WS_TRY(alloc_as(pc->sh_bytes.alloc(d->sh_coefs_bytes + 16), what));
        WS_TRY(alloc_as(pc->covars.alloc(d->covars_bytes), what));
        hipError_t e = hipMemcpy(pc->gaussians_c.get(), d->gaussians, d->gaussians_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(pc->sh_bytes.get(), d->sh_coefs, d->sh_coefs_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(pc->covars.get(), d->covars, d->covars_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, what);
    }
    *out = pc.release();
    return WS_OK;
}

// PlyReader::read + PointCloud::new with the per-vertex conversion (io/ply.rs:50-100) done by a kernel: the rows go
// to the device as they sit in the file, k_ply_decode writes the resident planes directly (ply_decode.hip).
int ws_pointcloud_create_from_ply_rows(ws_context* ctx, const float* rows, uint32_t n, uint32_t sh_deg,
                                       const ws_pointcloud_desc* meta, ws_pointcloud** out) {
    if (!ctx || !rows || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create_from_ply_rows: null argument");
    *out = nullptr;
    if (sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create_from_ply_rows: sh_deg > 3");
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create_from_ply_rows: empty point cloud");
    if (n >= (1u << 30)) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create_from_ply_rows: more than 2^30-1 points");
    const uint32_t row_len = 14u + 3u * (sh_deg + 1u) * (sh_deg + 1u);
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create_from_ply_rows: host allocation failed");
    pc->ctx = ctx;
    pc->num_points = n;
    pc->sh_deg = sh_deg;
    pc->compressed = false;
    ws_aabb zero;  // Aabb::zeroed(), io/mod.rs:74: the positions are the first three floats of every row
    std::memset(&zero, 0, sizeof zero);
    int32_t has_up = 0;
    int rc = ws_pointcloud_stats(rows, n, row_len * (uint32_t)sizeof(float), &zero, &pc->bbox, pc->center, &has_up, pc->up);
    pc->has_up = has_up != 0;
    if (meta) set_render_hints(pc.get(), meta);
    // Upload and decode run on a PRIVATE stream and are waited for with hipStreamSynchronize: no legacy-NULL-stream work
    // (it would serialise against every renderer and break replays of a captured frame graph) and no
    // device-wide synchronisation of other renderers' frames.
    if (rc) return rc;
    DeviceBuf<float> d_rows;  // (let go at the return, behind the stream sync)
    hipStream_t ls = nullptr;
    const char* what = "ws_pointcloud_create_from_ply_rows: upload";
    hipError_t e = hipStreamCreateWithFlags(&ls, hipStreamNonBlocking);
    if (e != hipSuccess) rc = hip_fail(e, what);
    if (rc == WS_OK) rc = alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), what);
    if (rc == WS_OK) rc = alloc_as(d_rows.alloc((size_t)n * row_len), what);
    if (rc == WS_OK && (e = hipMemcpyAsync(d_rows.get(), rows, d_rows.bytes(), hipMemcpyHostToDevice, ls)) != hipSuccess) rc = hip_fail(e, what);
    if (rc == WS_OK) rc = launch_ply_decode(d_rows.get(), n, sh_deg, pc->planes.get(), ls);
    if (rc == WS_OK) {
        e = hipStreamSynchronize(ls);
        if (e != hipSuccess) rc = hip_fail(e, "ws_pointcloud_create_from_ply_rows: decode");
    } else if (ls) {
        (void)hipStreamSynchronize(ls);
    }
    if (ls) (void)hipStreamDestroy(ls);
    if (rc) return rc;
    *out = pc.release();
    return WS_OK;
}

// The scene blobs as the loader would have produced them (parity tooling / accessors): uncompressed clouds are
// re-assembled from the resident planes into 28-B Gaussians + 96-B SH records, compressed blobs are copied back as is.
int ws_pointcloud_download(const ws_pointcloud* pc, void* gaussians, size_t gaussians_bytes, void* sh_coefs, size_t sh_bytes) {
    if (!pc || !gaussians || !sh_coefs) return fail(WS_ERR_INVALID, "ws_pointcloud_download: null argument");
    const size_t n = pc->num_points;
    if (pc->compressed) {
        if (gaussians_bytes < n * 24) return fail(WS_ERR_INVALID, "ws_pointcloud_download: gaussians buffer too small");
        WS_HIP(hipMemcpy(gaussians, pc->gaussians_c.get(), n * 24, hipMemcpyDeviceToHost));
        return WS_OK;  // (the packed SH / covariance codebooks are what the caller uploaded; not re-exported)
    }
    if (gaussians_bytes < n * 28 || sh_bytes < n * 96) return fail(WS_ERR_INVALID, "ws_pointcloud_download: buffers too small");
    std::vector<uint32_t> st;
    try {
        st.resize(n * PC_PLANES * 4);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_pointcloud_download: host allocation failed");
    }
    WS_HIP(hipMemcpy(st.data(), pc->planes.get(), st.size() * 4, hipMemcpyDeviceToHost));
    uint8_t* g = static_cast<uint8_t*>(gaussians);
    uint8_t* s = static_cast<uint8_t*>(sh_coefs);
    const ws::OmpQuietWorkers omp_quiet;  // (ws_internal.h: the region's workers sleep at once instead of spinning 200 ms)
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        std::memcpy(g + (size_t)i * 28, st.data() + ((size_t)0 * n + i) * 4, 16);
        std::memcpy(g + (size_t)i * 28 + 16, st.data() + ((size_t)1 * n + i) * 4, 12);
        for (int q = 0; q < 6; ++q) std::memcpy(s + (size_t)i * 96 + q * 16, st.data() + ((size_t)(2 + q) * n + i) * 4, 16);
    }
    return WS_OK;
}

// Saving (websplat.h "Saving a point cloud"): k_ply_encode writes the rows into one DeviceBuf, which is copied to the host and
// let go at the return.  Kernel and copy run on a private stream and are waited for, as ws_pointcloud_create_from_ply_rows does.
static int ply_rows_device_check(const ws_pointcloud* pc, const void* d_rows, size_t rows_bytes, const char* who, size_t* need) {
    if (!pc) return fail(WS_ERR_INVALID, std::string(who) + ": null argument");
    if (pc->compressed)
        return fail(WS_ERR_UNSUPPORTED, std::string(who) + ": a compressed cloud has no PLY rows (its codebooks are shared between Gaussians)");
    const uint32_t row_len = 14u + 3u * (pc->sh_deg + 1u) * (pc->sh_deg + 1u);
    *need = (size_t)pc->num_points * row_len * sizeof(float);
    if (!d_rows && *need) return fail(WS_ERR_INVALID, std::string(who) + ": null argument");
    if (rows_bytes < *need) return fail(WS_ERR_INVALID, std::string(who) + ": rows buffer too small");
    return WS_OK;
}

int ws_pointcloud_encode_ply_rows_device(const ws_pointcloud* pc, float* d_rows, size_t rows_bytes, void* stream) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, d_rows, rows_bytes, "ws_pointcloud_encode_ply_rows_device", &need));
    return launch_ply_encode(pc->planes.get(), pc->num_points, pc->sh_deg, d_rows, static_cast<hipStream_t>(stream));
}

int ws_pointcloud_decode_ply_rows_device(ws_pointcloud* pc, const float* d_rows, size_t rows_bytes, void* stream) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, d_rows, rows_bytes, "ws_pointcloud_decode_ply_rows_device", &need));
    return launch_ply_decode(d_rows, pc->num_points, pc->sh_deg, pc->planes.get(), static_cast<hipStream_t>(stream));
}

int ws_pointcloud_encode_ply_rows(const ws_pointcloud* pc, float* rows, size_t rows_bytes) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, rows, rows_bytes, "ws_pointcloud_encode_ply_rows", &need));
    const uint32_t n = pc->num_points;
    if (n == 0) return WS_OK;
    DeviceBuf<float> d_rows;  // (let go at the return, behind the stream sync)
    hipStream_t ls = nullptr;
    const char* what = "ws_pointcloud_encode_ply_rows: encode";
    int rc = WS_OK;
    hipError_t e = hipStreamCreateWithFlags(&ls, hipStreamNonBlocking);
    if (e != hipSuccess) rc = hip_fail(e, what);
    if (rc == WS_OK) rc = alloc_as(d_rows.alloc(need / sizeof(float)), what);
    if (rc == WS_OK) rc = launch_ply_encode(pc->planes.get(), n, pc->sh_deg, d_rows.get(), ls);
    if (rc == WS_OK && (e = hipMemcpyAsync(rows, d_rows.get(), need, hipMemcpyDeviceToHost, ls)) != hipSuccess) rc = hip_fail(e, what);
    if (ls) {
        e = hipStreamSynchronize(ls);
        if (rc == WS_OK && e != hipSuccess) rc = hip_fail(e, what);
        (void)hipStreamDestroy(ls);
    }
    return rc;
}

int ws_pointcloud_save_ply(const ws_pointcloud* pc, const char* path) {
    if (!pc || !path) return fail(WS_ERR_INVALID, "ws_pointcloud_save_ply: null argument");
    if (pc->compressed)
        return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_save_ply: a compressed cloud cannot be saved as a PLY (its codebooks are shared between Gaussians)");
    const uint32_t row_len = 14u + 3u * (pc->sh_deg + 1u) * (pc->sh_deg + 1u);
    std::vector<float> rows;
    try {
        rows.resize((size_t)pc->num_points * row_len);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_pointcloud_save_ply: host allocation failed");
    }
    WS_TRY(ws_pointcloud_encode_ply_rows(pc, rows.data(), rows.size() * sizeof(float)));
    ws_pointcloud_desc meta;  // the file is opened only now, with the rows in hand
    std::memset(&meta, 0, sizeof meta);
    meta.has_mip_splatting = pc->has_mip;
    meta.mip_splatting = pc->mip;
    meta.has_kernel_size = pc->has_kernel_size;
    meta.kernel_size = pc->kernel_size;
    meta.has_background_color = pc->has_background;
    std::memcpy(meta.background_color, pc->background, sizeof meta.background_color);
    return ws_ply_write(path, rows.data(), pc->num_points, pc->sh_deg, &meta);
}

int ws_pointcloud_create_subset(ws_context* ctx, const ws_pointcloud* src, const uint32_t* indices, uint32_t n, ws_pointcloud** out) {
    if (!ctx || !src || !indices || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: null argument");
    *out = nullptr;
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: empty subset");
    for (uint32_t i = 0; i < n; ++i)
        if (indices[i] >= src->num_points || (i && indices[i] <= indices[i - 1]))
            return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: indices must be strictly ascending and below the number of points");
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create_subset: host allocation failed");
    static_cast<PointCloudMeta&>(*pc) = *src;  // bbox, centre, up, metadata, sh_deg, quantisation: verbatim
    pc->ctx = ctx;
    pc->num_points = n;
    // upload, gather and the codebook copies run on a private stream and are waited for (as ws_pointcloud_create_from_ply_rows)
    DeviceBuf<uint32_t> d_idx;  // (let go at the return, behind the stream sync)
    hipStream_t ls = nullptr;
    const char* what = "ws_pointcloud_create_subset: allocation / copy";
    int rc = d_idx.alloc(n);
    hipError_t e = hipSuccess;
    if (rc == WS_OK) e = hipStreamCreateWithFlags(&ls, hipStreamNonBlocking);
    if (rc == WS_OK && e == hipSuccess) e = hipMemcpyAsync(d_idx.get(), indices, (size_t)n * 4, hipMemcpyHostToDevice, ls);
    if (rc == WS_OK && e == hipSuccess) {
        if (!src->compressed) {
            rc = alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), what);
            if (rc == WS_OK)
                rc = launch_pc_gather(reinterpret_cast<const uint32_t*>(src->planes.get()), reinterpret_cast<uint32_t*>(pc->planes.get()), d_idx.get(),
                                      src->num_points, n, PC_PLANES, 4, ls);
        } else {
            rc = alloc_as(pc->gaussians_c.alloc((size_t)n * 24), what);
            if (rc == WS_OK) rc = alloc_as(pc->sh_bytes.alloc(src->sh_bytes.count()), what);
            if (rc == WS_OK) rc = alloc_as(pc->covars.alloc(src->covars.count()), what);
            if (rc == WS_OK) e = hipMemcpyAsync(pc->sh_bytes.get(), src->sh_bytes.get(), src->sh_bytes.bytes(), hipMemcpyDeviceToDevice, ls);
            if (rc == WS_OK && e == hipSuccess) e = hipMemcpyAsync(pc->covars.get(), src->covars.get(), src->covars.bytes(), hipMemcpyDeviceToDevice, ls);
            if (rc == WS_OK && e == hipSuccess)
                rc = launch_pc_gather(reinterpret_cast<const uint32_t*>(src->gaussians_c.get()), reinterpret_cast<uint32_t*>(pc->gaussians_c.get()), d_idx.get(),
                                      src->num_points, n, 1, 6, ls);
        }
    }
    if (e != hipSuccess && rc == WS_OK) rc = hip_fail(e, what);
    if (ls) {
        const hipError_t se = hipStreamSynchronize(ls);
        if (se != hipSuccess && rc == WS_OK) rc = hip_fail(se, "ws_pointcloud_create_subset: gather");
        (void)hipStreamDestroy(ls);
    }
    if (rc) return rc;
    *out = pc.release();
    return WS_OK;
}

void ws_pointcloud_destroy(ws_pointcloud* pc) { delete pc; }

uint32_t ws_pointcloud_num_points(const ws_pointcloud* pc) { return pc ? pc->num_points : 0; }
uint32_t ws_pointcloud_sh_deg(const ws_pointcloud* pc) { return pc ? pc->sh_deg : 0; }
int ws_pointcloud_compressed(const ws_pointcloud* pc) { return pc && pc->compressed ? 1 : 0; }
int ws_pointcloud_bbox(const ws_pointcloud* pc, ws_aabb* out) {
    if (!pc || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_bbox: null argument");
    *out = pc->bbox;
    return WS_OK;
}
int ws_pointcloud_center(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_center: null argument");
    std::memcpy(out, pc->center, 12);
    return WS_OK;
}
int ws_pointcloud_up(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !pc->has_up) return 0;
    if (out) std::memcpy(out, pc->up, 12);
    return 1;
}
int ws_pointcloud_mip_splatting(const ws_pointcloud* pc, int32_t* out) {
    if (!pc || !pc->has_mip) return 0;
    if (out) *out = pc->mip ? 1 : 0;
    return 1;
}
int ws_pointcloud_kernel_size(const ws_pointcloud* pc, float* out) {
    if (!pc || !pc->has_kernel_size) return 0;
    if (out) *out = pc->kernel_size;
    return 1;
}
int ws_pointcloud_background_color(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !pc->has_background) return 0;
    if (out) std::memcpy(out, pc->background, 12);
    return 1;
}

// ---- GaussianRenderer --------------------------------------------------------------------------------
int ws_renderer_create(ws_context* ctx, ws_color_format format, uint32_t sh_deg, int compressed, ws_renderer** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_renderer_create: null argument");
    *out = nullptr;
    if (sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_renderer_create: sh_deg > 3");
    if (format != WS_FORMAT_RGBA8_UNORM && format != WS_FORMAT_RGBA16_FLOAT && format != WS_FORMAT_RGBA32_FLOAT)
        return fail(WS_ERR_INVALID, "ws_renderer_create: unknown colour format");
    ws_renderer* r = new (std::nothrow) ws_renderer();
    if (!r) return fail(WS_ERR_OOM, "ws_renderer_create: host allocation failed");
    r->ctx = ctx;
    r->format = format;
    r->sh_deg = sh_deg;
    r->compressed = compressed != 0;
    r->capture = ctx->capture;
    for (auto& e : r->ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            ws_renderer_destroy(r);
            return fail(WS_ERR_HIP, "ws_renderer_create: hipEventCreate failed");
        }
    }
    if (r->sticky.alloc(2) != WS_OK || hipMemset(r->sticky.get(), 0, r->sticky.bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        ws_renderer_destroy(r);
        return fail(WS_ERR_HIP, "ws_renderer_create: error word allocation failed");
    }
    // the demand mailbox (optional: without pinned memory the capacity still grows through ws_renderer_errors)
    if (hipHostMalloc(reinterpret_cast<void**>(&r->demand_mailbox), 4 * sizeof(uint32_t), hipHostMallocMapped) == hipSuccess) {
        r->demand_mailbox[0] = r->demand_mailbox[1] = r->demand_mailbox[2] = r->demand_mailbox[3] = 0u;
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&r->demand_mailbox_dev), r->demand_mailbox, 0) != hipSuccess) {
            (void)hipHostFree(r->demand_mailbox);
            r->demand_mailbox = r->demand_mailbox_dev = nullptr;
        }
    } else {
        r->demand_mailbox = nullptr;
    }
    (void)hipGetLastError();
    *out = r;
    return WS_OK;
}

void ws_renderer_destroy(ws_renderer* r) {
    if (!r) return;
    (void)hipDeviceSynchronize();
    renderer_free_graph(r);
    if (r->demand_mailbox) (void)hipHostFree(r->demand_mailbox);
    for (auto& e : r->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : r->ev_group)
        if (e) (void)hipEventDestroy(e);
    r->marks.destroy();
    delete r;
}

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
        if (r->timers) WS_HIP(hipEventRecord(r->ev[0], stream));
        if ((rc = launch_preprocess(kp, kb, pc->compressed, plan.footprint_mode, stream, r->frame.k1_depths))) return rc;
        km_mark(km, pc->compressed ? "k_preprocess<compressed>" : "k_preprocess");
        if (r->timers) WS_HIP(hipEventRecord(r->ev[1], stream));
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
    if (r->timers) WS_HIP(hipEventRecord(r->ev[2], stream));
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
        WS_HIP(hipEventRecord(r->ev[3], stream));
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
    q.span_class = renderer_span_class(r);
    q.graph_depth_bits = r->fg.depth_bits;
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
    ws_renderer::FrameGraph& g = r->fg;
    if (!(g.valid && g.pc == pc && g.generation == r->scratch_generation && g.order_mode == r->order_mode)) {
        renderer_free_graph(r);  // (with it the digit width it kept: this capture's depth sort chooses its own)
        WS_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        rc = enqueue_frame(r, pc, kp, kb, stream);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            r->frame = PreparedFrame();
            return rc;
        }
        if (ce != hipSuccess || !graph) return hip_fail(ce, "ws_renderer_prepare: stream capture");
        g.graph = graph;
        // K1's node: the one kernel node whose function is the preprocess kernel
        size_t nn = 0;
        WS_HIP(hipGraphGetNodes(graph, nullptr, &nn));
        std::vector<hipGraphNode_t> nodes(nn);
        WS_HIP(hipGraphGetNodes(graph, nodes.data(), &nn));
        const void* k1_func = preprocess_kernel_func(pc->compressed, r->plan.footprint_mode, r->frame.k1_depths != nullptr);
        for (size_t i = 0; i < nn && !g.k1_node; ++i) {
            hipGraphNodeType ty;
            if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
            hipKernelNodeParams kn;
            if (hipGraphKernelNodeGetParams(nodes[i], &kn) != hipSuccess) continue;
            if (kn.func == k1_func) {
                g.k1_node = nodes[i];
                g.k1_params = kn;
            }
        }
        if (!g.k1_node) {
            renderer_free_graph(r);
            return fail(WS_ERR_HIP, "ws_renderer_prepare: the preprocess kernel was not found in the captured frame graph");
        }
        for (int i = 0; i < ws_renderer::GRAPH_RING; ++i) {
            WS_HIP(hipGraphInstantiate(&g.exec[i], graph, nullptr, nullptr, 0));
            WS_HIP(hipEventCreateWithFlags(&g.done[i], hipEventDisableTiming));
        }
        g.pc = pc;
        g.generation = r->scratch_generation;
        g.arrays = r->frame.arrays;  // (with: did the captured frame run k_blend_order?)
        g.order_mode = r->order_mode;
        g.depth_bits = r->plan.depth_digit_bits;
        g.valid = true;
    }
    const int slot = (int)(g.next++ % ws_renderer::GRAPH_RING);
    if (g.used[slot]) WS_HIP(hipEventSynchronize(g.done[slot]));  // an earlier launch of this executable graph must have run
    // (the DEPTH form of K1 takes the z plane as a third argument; toggling depth re-captures: ws_renderer_enable_depth)
    float* k1_depths = r->frame.k1_depths;
    void* k1_args[3] = {const_cast<K1Params*>(&kp), const_cast<K1Buffers*>(&kb), &k1_depths};
    hipKernelNodeParams np = g.k1_params;
    np.kernelParams = k1_args;
    np.extra = nullptr;
    WS_HIP(hipGraphExecKernelNodeSetParams(g.exec[slot], g.k1_node, &np));
    WS_HIP(hipGraphLaunch(g.exec[slot], stream));
    WS_HIP(hipEventRecord(g.done[slot], stream));
    g.used[slot] = true;
    r->frame.arrays = g.arrays;  // what THIS graph's frames write, whatever a launch-by-launch frame left behind
    r->frame.depth = r->frame.k1_depths != nullptr;
    return frame_prepared(r, pc, stream);
}

}  // extern "C"

uint32_t ws_internal_renderer_frames_enqueued(const ws_renderer* r) { return r ? r->frames_enqueued : 0u; }
bool ws_internal_renderer_progress(const ws_renderer* r, uint32_t* started_seq) {
    if (!r || !r->demand_mailbox) return false;
    *started_seq = *reinterpret_cast<volatile const uint32_t*>(r->demand_mailbox + 1);
    return true;
}
void ws_internal_renderer_set_throughput_mode(ws_renderer* r, bool on) {
    if (r) r->throughput_mode = on;
}

uint32_t ws_internal_renderer_demand(const ws_renderer* r) {
    if (!r) return 0u;
    uint32_t d = r->needed_seen;
    if (r->demand_mailbox) d = std::max(d, (uint32_t)*reinterpret_cast<volatile const uint32_t*>(r->demand_mailbox));
    return d;
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
            if (!rs[i]->ev_group[e]) WS_HIP(hipEventCreateWithFlags(&rs[i]->ev_group[e], hipEventDisableTiming));
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
            WS_HIP(hipEventRecord(rs[i]->ev_group[0], streams[i]));
            WS_HIP(hipStreamWaitEvent(streams[0], rs[i]->ev_group[0], 0));
        }
    }
    if ((rc = launch_preprocess_multi(kp, kb, n, pc->compressed, rs[0]->plan.footprint_mode, streams[0]))) return rc;
    WS_HIP(hipEventRecord(rs[0]->ev_group[1], streams[0]));
    // (Measured and removed: starting the frames of a group one after another behind events, so that they do not run the
    // same stage in lock-step -- 3781 instead of 5155 frames/s; every cross-stream wait costs more than the lock-step does.)
    for (uint32_t i = 0; i < n; ++i) {
        if (i > 0) WS_HIP(hipStreamWaitEvent(streams[i], rs[0]->ev_group[1], 0));
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
    bp.demand_mailbox = r->demand_mailbox_dev;
    bp.progress_mailbox = r->demand_mailbox_dev ? r->demand_mailbox_dev + 1 : nullptr;
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
    if (r->timers) WS_HIP(hipEventRecord(r->ev[4], stream));
    if (r->ctx->debug_cut >= 1 && r->ctx->debug_cut <= 4) return WS_OK;  // analysis only
    int rc = launch_blend(bp, form.variant, stream, planes, comp);
    if (rc) return rc;
    r->frames_enqueued = bp.frame_seq;
    km_mark(km, fr.target_precision ? "k_blend_strict" : "k_blend");
    if (r->timers) {
        WS_HIP(hipEventRecord(r->ev[5], stream));
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
    WS_HIP(hipStreamSynchronize(r->last_stream));
    FrameCounters fc;
    WS_TRY(copy_d2h(&fc, r->scratch.counters(), offsetof(FrameCounters, tile_sums), r->last_stream));
    out->num_visible = fc.num_visible;
    out->num_tile_entries = fc.num_entries;
    out->tile_entries_capacity = r->plan.entry_cap;
    out->overflow = fc.overflow;
    return WS_OK;
}

// Number of tile LISTS of the last prepared frame and the shift from blend tiles to binning tiles: the device decides per
// frame (bin_shift_decide, k_bin_prefix) whether a list serves one blend tile or a 2x2 block of them.
static int frame_list_counts(ws_renderer* r, uint32_t* shift, uint32_t* lists_x, uint32_t* lists_y) {
    WS_HIP(hipStreamSynchronize(r->last_stream));
    FrameCounters fc;
    WS_TRY(copy_d2h(&fc, r->scratch.counters(), offsetof(FrameCounters, tile_sums), r->last_stream));
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
    WS_HIP(hipEventSynchronize(r->ev[3]));
    WS_HIP(hipEventElapsedTime(&out->preprocess_ms, r->ev[0], r->ev[1]));
    WS_HIP(hipEventElapsedTime(&out->sorting_ms, r->ev[1], r->ev[2]));
    WS_HIP(hipEventElapsedTime(&out->binning_ms, r->ev[2], r->ev[3]));
    if (r->ev_render_valid) {
        WS_HIP(hipEventSynchronize(r->ev[5]));
        WS_HIP(hipEventElapsedTime(&out->rasterization_ms, r->ev[4], r->ev[5]));
    }
    return WS_OK;
}

int ws_renderer_kernel_times(ws_renderer* r, uint32_t capacity, ws_kernel_time* out, uint32_t* count) {
    if (!r || !count) return fail(WS_ERR_INVALID, "ws_renderer_kernel_times: null argument");
    if (!r->marks.active) return fail(WS_ERR_STATE, "ws_renderer_kernel_times: needs ws_renderer_enable_timers(r, 2)");
    const KernelMarks& km = r->marks;
    *count = (uint32_t)km.n;
    if (km.n == 0) return WS_OK;
    WS_HIP(hipEventSynchronize(km.ev[km.n]));
    for (int i = 0; i < km.n && (uint32_t)i < capacity && out; ++i) {
        std::memset(&out[i], 0, sizeof out[i]);
        std::strncpy(out[i].name, km.label[i] ? km.label[i] : "?", sizeof(out[i].name) - 1);
        WS_HIP(hipEventElapsedTime(&out[i].ms, km.ev[i], km.ev[i + 1]));
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
        for (uint32_t i = 0; i < nt; ++i) list_len[i] = rg[i].y ? rg[i].y - (0xFFFFFFFFu - rg[i].x) : 0u;
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
            if (begin) begin[i] = rg[i].y ? 0xFFFFFFFFu - rg[i].x : 0u;
            if (end) end[i] = rg[i].y;
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

// ---- GPURSSorter ---------------------------------------------------------------------------------------
int ws_sorter_create(ws_context* ctx, uint32_t max_n, ws_sorter** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_sorter_create: null argument");
    *out = nullptr;
    if (max_n == 0 || max_n >= (1u << 30)) return fail(WS_ERR_INVALID, "ws_sorter_create: max_n out of range");
    std::unique_ptr<ws_sorter, SyncedDelete> s(new (std::nothrow) ws_sorter());
    if (!s) return fail(WS_ERR_OOM, "ws_sorter_create: host allocation failed");
    s->ctx = ctx;
    const SortShape shape = sort_shape(max_n, 0, 512);  // (512 count rows: 9-bit digits)
    WS_TRY(s->keys_alt.alloc((size_t)max_n + 4));
    WS_TRY(s->vals_alt.alloc((size_t)max_n + 4));
    WS_TRY(s->tile_sums.alloc(shape.sum_words));
    WS_TRY(s->zero.alloc(1));
    WS_TRY(s->aux_alt.alloc((size_t)max_n + 4));
    if (hipDeviceSynchronize() != hipSuccess) return fail(WS_ERR_HIP, "ws_sorter_create: device sync failed");
    SorterZero* const zero = s->zero.get();
    s->sc = sort_view(shape, s->keys_alt.get(), s->vals_alt.get(), zero->hist, 512, s->tile_sums.get(), nullptr);
    if (ctx->depth_sort_mode == DS_ONESWEEP || ctx->depth_sort_mode == DS_COOP) {
        WS_TRY(s->fat_status.alloc(fat_sort_status_words()));
        if (hipMemset(s->fat_status.get(), 0, s->fat_status.bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return fail(WS_ERR_HIP, "ws_sorter_create: look-back word initialisation failed");
        FatSortScratch& fs = s->fat;
        fs.cap = max_n, fs.status = s->fat_status.get(), fs.grid_request = ctx->dsort_fat_grid;
        fs.keys_alt = s->keys_alt.get(), fs.vals_alt = s->vals_alt.get(), fs.aux_alt = s->aux_alt.get();
        fs.hist = zero->hist, fs.tickets = zero->tickets, fs.barrier = zero->fat_barrier, fs.error = &zero->error;
    }
    *out = s.release();
    return WS_OK;
}

void ws_sorter_destroy(ws_sorter* s) { SyncedDelete()(s); }

int ws_sorter_sort(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, const uint32_t* d_count, uint32_t n,
                   void* stream_v) {
    if (!s || !d_keys || !d_payload) return fail(WS_ERR_INVALID, "ws_sorter_sort: null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    s->folded = false;  // (the memset below clears what a ws_sorter_sort_depth decided)
    WS_HIP(hipMemsetAsync(s->zero.get(), 0, sizeof(SorterZero), stream));
    SortJob job;
    job.keys = d_keys, job.vals = d_payload, job.d_count = d_count, job.n = n;
    SortResult res;
    WS_TRY(launch_sort_pairs(s->sc, job, stream, nullptr, &res));
    if (res.keys != d_keys) return fail(WS_ERR_STATE, "ws_sorter_sort: internal ping-pong parity error");
    return WS_OK;
}

// The renderer's depth sort as a stand-alone call: the same result as ws_sorter_sort (stable ascending on the full
// 32-bit keys) by the kernels a frame's depth sort runs -- the generic sorter with a companion value, or, in a context
// created with WS_DEPTH_SORT=onesweep | coop and for inputs within its capacity, the fat-tile one-sweep (sort.hip);
// `d_aux` (may be null) is a 4-byte companion value that travels with the payload.  Four passes: keys, payload and
// companion are sorted in place.
int ws_sorter_sort_depth(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, uint32_t* d_aux, const uint32_t* d_count,
                         uint32_t n, void* stream_v) {
    if (!s || !d_keys || !d_payload) return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: null argument");
    if (n > s->sc.cap) return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: n exceeds the sorter's capacity");
    // the histogram kernels read the keys 16 bytes at a time: the same alignment ws_sorter_sort asks for
    if ((reinterpret_cast<uintptr_t>(d_keys) & 15u) != 0)
        return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: keys must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (++s->epoch == 0) {  // epoch-tagged count rows of the fat-tile form: re-zeroed on wrap-around
        if (s->fat_status.get()) WS_HIP(hipMemsetAsync(s->fat_status.get(), 0, s->fat_status.bytes(), stream));
        s->epoch = 1;
    }
    s->folded = false;
    s->last_stream = stream;
    WS_HIP(hipMemsetAsync(s->zero.get(), 0, sizeof(SorterZero), stream));
    const bool fat = n != 0 && s->fat.status && fat_sort_grid(n, s->ctx->num_cus, s->fat.grid_request) != 0u;
    // the frame's form (ws_renderer_prepare): the first histogram kernel reports the key range, the column scan behind it decides
    // the base of passes 1..3 and whether the fourth pass runs (depth_range_decide)
    FrameCounters* skip_top = (s->ctx->depth_skip_top && !fat) ? &s->zero.get()->counters : nullptr;
    s->folded = skip_top != nullptr;
    if (n == 0) return WS_OK;
    SortResult res;
    if (fat)
        return launch_depth_sort_fat(s->fat, d_keys, d_payload, d_aux, d_count, n, false, s->ctx->depth_sort_mode == DS_COOP,
                                     s->epoch, s->ctx->num_cus, stream, nullptr, &res);
    SortJob job;
    job.kind = SORT_DEPTH;
    job.keys = d_keys, job.vals = d_payload, job.d_count = d_count, job.n = n;
    job.digit_bits = depth_sort_digit_bits(s->ctx->depth_digit_bits, false, 0u, 0);  // (no previous frame, no graph: forced, or the default)
    job.aux = d_aux, job.aux_alt = d_aux ? s->aux_alt.get() : nullptr;
    job.skip_top = skip_top;
    job.kpt9 = s->ctx->depth_tile_kpt ? s->ctx->depth_tile_kpt : 8;
    WS_TRY(launch_sort_pairs(s->sc, job, stream, nullptr, &res));
    if (res.keys != d_keys) return fail(WS_ERR_STATE, "ws_sorter_sort_depth: internal ping-pong parity error");
    if (!skip_top) return WS_OK;
    // three passes when the fourth was skipped: the result is in the scratch partners -> back in place
    if (res.keys_skipped != s->sc.keys_alt || res.vals_skipped != s->sc.vals_alt)
        return fail(WS_ERR_STATE, "ws_sorter_sort_depth: internal ping-pong parity error (skipped pass)");
    return launch_depth_copy_back(&skip_top->depth_skip_top, d_count, n, res.keys_skipped, res.vals_skipped, res.aux_skipped, d_keys,
                                  d_payload, d_aux, stream);
}

int ws_sorter_depth_range(ws_sorter* s, uint32_t* base, uint32_t* skip, uint32_t* span_class) {
    if (!s || !base || !skip || !span_class) return fail(WS_ERR_INVALID, "ws_sorter_depth_range: null argument");
    if (!s->folded)
        return fail(WS_ERR_STATE, "ws_sorter_depth_range: the last ws_sorter_sort_depth did not fold its key range "
                                  "(the context's depth_skip_top is 0, the fat-tile form ran, or no such call)");
    uint32_t w[3];  // depth_skip_top, depth_key_base, depth_span_class: adjacent words of the counters' second line
    static_assert(offsetof(FrameCounters, depth_key_base) == offsetof(FrameCounters, depth_skip_top) + 4 &&
                      offsetof(FrameCounters, depth_span_class) == offsetof(FrameCounters, depth_skip_top) + 8,
                  "FrameCounters layout");
    WS_TRY(copy_d2h(w, &s->zero.get()->counters.depth_skip_top, sizeof w, s->last_stream));
    *skip = w[0];
    *base = w[1];
    *span_class = w[2];
    return WS_OK;
}

int ws_sort_selftest(ws_context* ctx, int* passed) {
    if (!ctx || !passed) return fail(WS_ERR_INVALID, "ws_sort_selftest: null argument");
    *passed = 0;
    const uint32_t n = 8192;  // gpu_rs.rs:297
    std::vector<float> scrambled(n), expect(n);
    std::vector<uint32_t> payload(n);
    for (uint32_t i = 0; i < n; ++i) {
        scrambled[i] = (float)(n - 1 - i);
        expect[i] = (float)i;
        payload[i] = i;
    }
    ws_sorter* sorter = nullptr;
    WS_TRY(ws_sorter_create(ctx, n, &sorter));
    DeviceBuf<uint32_t> dk, dv;  // (declared first: let go after the sorter's destroyer has waited for the device)
    const std::unique_ptr<ws_sorter, SyncedDelete> s(sorter);
    WS_TRY(dk.alloc(n));
    WS_TRY(dv.alloc(n));
    hipError_t e = hipMemcpy(dk.get(), scrambled.data(), n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dv.get(), payload.data(), n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "ws_sort_selftest: upload");
    WS_TRY(ws_sorter_sort(s.get(), dk.get(), dv.get(), nullptr, n, nullptr));
    std::vector<float> got(n);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(got.data(), dk.get(), n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "ws_sort_selftest: download");
    *passed = std::memcmp(got.data(), expect.data(), n * 4) == 0 ? 1 : 0;
    return WS_OK;
}

}  // extern "C"
