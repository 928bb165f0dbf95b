// ws_api.cpp -- the C ABI (include/websplat.h), the part every handle stands on: the error state, the runtime behind the owners
// (device_buf.h, hip_handles.h), the context, device memory and the ws_debug_* hooks.  One unit per handle beside it:
// api_pointcloud.cpp, api_renderer.cpp (the frame) with api_readback.cpp (what is read back from it), api_sorter.cpp; the passes
// that only read a prepared frame, and the objects they fill, are in api_attrib.cpp, api_metrics.cpp and api_refit.cpp.
//
// Mirrors the reference's object model: WGPUContext (lib.rs:57-125) -> ws_context,
// PointCloud (pointcloud.rs:72-222) -> ws_pointcloud, GaussianRenderer (renderer.rs:17-283) -> ws_renderer,
// GPURSSorter + PointCloudSortStuff (gpu_rs.rs:23-175, 865-884) -> ws_sorter.
#include <algorithm>
#include <cstring>
#include <new>

#include "ws_internal.h"

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

// The runtime behind the owners of hip_handles.h: the only place where the library creates or destroys an event, a stream, a
// graph, an executable graph or pinned memory.
int event_create(hipEvent_t* e, bool timing) {
    if (timing) WS_HIP(hipEventCreate(e));
    else WS_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return WS_OK;
}
void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
int stream_create(hipStream_t* s) {
    WS_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    return WS_OK;
}
void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
int graph_end_capture(hipGraph_t* g, hipStream_t capturing) {
    const hipError_t e = hipStreamEndCapture(capturing, g);
    if (e == hipSuccess && *g) return WS_OK;
    if (*g) (void)hipGraphDestroy(*g);
    *g = nullptr;
    return hip_fail(e, "ws_renderer_prepare: stream capture");
}
void graph_destroy(hipGraph_t g) { (void)hipGraphDestroy(g); }
int graph_exec_create(hipGraphExec_t* x, hipGraph_t graph) {
    WS_HIP(hipGraphInstantiate(x, graph, nullptr, nullptr, 0));
    return WS_OK;
}
void graph_exec_destroy(hipGraphExec_t x) { (void)hipGraphExecDestroy(x); }
int pinned_words_create(uint32_t** host, uint32_t** dev, size_t count) {
    *host = *dev = nullptr;
    uint32_t* h = nullptr;
    WS_HIP(hipHostMalloc(reinterpret_cast<void**>(&h), count * sizeof(uint32_t), hipHostMallocMapped));
    std::memset(h, 0, count * sizeof(uint32_t));
    const hipError_t e = hipHostGetDevicePointer(reinterpret_cast<void**>(dev), h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        *dev = nullptr;
        return hip_fail(e, "hipHostGetDevicePointer");
    }
    *host = h;
    return WS_OK;
}
void pinned_words_destroy(uint32_t* host) { (void)hipHostFree(host); }

}  // namespace ws

using namespace ws;

// depth sort of a context that does not say otherwise (WS_DEPTH_SORT): decided by measurement, profiles/r04/
#ifndef WS_DEPTH_SORT_DEFAULT
#define WS_DEPTH_SORT_DEFAULT DS_SCAN
#endif

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

}  // extern "C"
