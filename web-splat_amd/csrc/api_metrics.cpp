// api_metrics.cpp -- the C ABI's image comparisons (include/websplat.h "Image metrics", "Gradients of an image loss"; metrics.hip;
// DESIGN.md 3.4e): the ws_metrics accumulator of per-image records, the error plane and the loss gradient of two images.
#include <cmath>
#include <new>
#include <vector>

#include "api_state.h"
#include "metrics.h"
using namespace ws;

struct ws_metrics {
    ws_context* ctx = nullptr;
    uint32_t max_images = 0;
    uint32_t count = 0;                  // records added (host counter)
    DeviceBuf<MetricsRecord> records;    // [max_images]
    DeviceBuf<MetricsPartial> slab;      // one partial record per workgroup of the add in flight; shared by the adds of one stream
    hipStream_t last_stream = nullptr;
};

void ws_internal_metrics_truncate(ws_metrics* m, uint32_t count) {
    if (m && count < m->count) m->count = count;
}

namespace {
int metrics_view(const ws_image_view* v, uint32_t width, const char* which, MetricsView* out, const char* fn = "ws_metrics_add") {
    const std::string who = std::string(fn) + ": image " + which;
    if (!v->d_pixels) return fail(WS_ERR_INVALID, who + ": null pixels");
    size_t texel;
    switch (v->format) {
        case WS_FORMAT_RGBA8_UNORM: texel = 4; break;
        case WS_FORMAT_RGBA16_FLOAT: texel = 8; break;
        case WS_FORMAT_RGBA32_FLOAT: texel = 16; break;
        default: return fail(WS_ERR_INVALID, who + ": unknown colour format");
    }
    if (v->row_pitch_bytes < texel * width) return fail(WS_ERR_INVALID, who + ": row pitch below the row");
    if (v->row_pitch_bytes % texel != 0 || reinterpret_cast<uintptr_t>(v->d_pixels) % texel != 0)
        return fail(WS_ERR_INVALID, who + ": pointer and row pitch must be multiples of the texel size");
    out->pixels = v->d_pixels;
    out->pitch = v->row_pitch_bytes;
    out->format = (int)v->format;
    out->over_bg = v->over_background != 0;
    for (int i = 0; i < 3; ++i) out->bg[i] = v->background[i];
    return WS_OK;
}

// ws_image_error_plane and ws_image_error_gradient: one judgement of the two images; out is an f32 plane, or with `gradient` a
// float4 plane (k_image_error_grad), which has no quantised form
int image_error(const char* fn, const ws_context* ctx, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height,
                int kind, uint32_t flags, float* d_out, size_t pitch, bool gradient, void* stream_v) {
    const std::string who(fn);
    const size_t texel = gradient ? 16 : 4;
    if (!ctx || !a || !b || !d_out) return fail(WS_ERR_INVALID, who + ": null argument");
    if (width == 0 || height == 0) return fail(WS_ERR_INVALID, who + ": empty image");
    if (width > 65536u || height > 65536u) return fail(WS_ERR_INVALID, who + ": image larger than 65536 pixels on a side");
    if (gradient && (flags & WS_METRICS_QUANTIZE_U8)) return fail(WS_ERR_INVALID, who + ": WS_METRICS_QUANTIZE_U8 has no gradient");
    if (flags & ~WS_METRICS_QUANTIZE_U8) return fail(WS_ERR_INVALID, who + ": unknown flag bits");
    if (kind != WS_ERROR_SQ && kind != WS_ERROR_ABS) return fail(WS_ERR_INVALID, who + ": kind must be WS_ERROR_SQ or WS_ERROR_ABS");
    ImageErrorParams p;
    int rc = metrics_view(a, width, "a", &p.a, fn);
    if (rc == WS_OK) rc = metrics_view(b, width, "b", &p.b, fn);
    if (rc) return rc;
    if (pitch < (size_t)width * texel || pitch % texel != 0 || reinterpret_cast<uintptr_t>(d_out) % texel != 0)
        return fail(WS_ERR_INVALID, who + (gradient ? ": gradient pitch below 16 x width, or gradient pointer / pitch not 16-B aligned"
                                                    : ": plane pitch below 4 x width, or plane pointer / pitch not 4-B aligned"));
    p.width = width;
    p.height = height;
    p.flags = flags;
    p.kind = kind;
    p.plane = d_out;
    p.plane_pitch = pitch;
    p.gradient = gradient;
    return launch_image_error(p, static_cast<hipStream_t>(stream_v));
}
}  // namespace

extern "C" {

int ws_metrics_create(ws_context* ctx, uint32_t max_images, ws_metrics** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_metrics_create: null argument");
    *out = nullptr;
    if (max_images == 0) return fail(WS_ERR_INVALID, "ws_metrics_create: no images");
    ws_metrics* m = new (std::nothrow) ws_metrics();
    if (!m) return fail(WS_ERR_OOM, "ws_metrics_create: host allocation failed");
    m->ctx = ctx;
    m->max_images = max_images;
    const int rc = m->records.alloc(max_images);
    if (rc != WS_OK) {
        delete m;
        return rc;
    }
    *out = m;
    return WS_OK;
}

void ws_metrics_destroy(ws_metrics* m) { SyncedDelete()(m); }

int ws_metrics_reset(ws_metrics* m, void* stream_v) {
    if (!m) return fail(WS_ERR_INVALID, "ws_metrics_reset: null accumulator");
    // records are written whole by the add that owns them: emptying is the host counter
    m->count = 0;
    m->last_stream = static_cast<hipStream_t>(stream_v);
    return WS_OK;
}

uint32_t ws_metrics_count(const ws_metrics* m) { return m ? m->count : 0u; }

int ws_metrics_add(ws_metrics* m, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, uint32_t flags,
                   float* d_ssim_map, size_t map_pitch_bytes, void* stream_v) {
    if (!m || !a || !b) return fail(WS_ERR_INVALID, "ws_metrics_add: null argument");
    if (width == 0 || height == 0) return fail(WS_ERR_INVALID, "ws_metrics_add: empty image");
    if (width > 65536u || height > 65536u) return fail(WS_ERR_INVALID, "ws_metrics_add: image larger than 65536 pixels on a side");
    if (flags & ~WS_METRICS_QUANTIZE_U8) return fail(WS_ERR_INVALID, "ws_metrics_add: unknown flag bits");
    MetricsParams p;
    int rc = metrics_view(a, width, "a", &p.a);
    if (rc == WS_OK) rc = metrics_view(b, width, "b", &p.b);
    if (rc) return rc;
    if (d_ssim_map && (map_pitch_bytes < (size_t)width * 4 || map_pitch_bytes % 4 != 0 || reinterpret_cast<uintptr_t>(d_ssim_map) % 4 != 0))
        return fail(WS_ERR_INVALID, "ws_metrics_add: map pitch below 4 x width, or map pointer / pitch not 4-B aligned");
    if (m->count >= m->max_images) return fail(WS_ERR_OVERFLOW, "ws_metrics_add: the accumulator is full");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const uint32_t tiles = metrics_num_tiles(width, height);
    // (alloc frees the old slab first, and hipFree waits for the adds that still use it)
    if (tiles > m->slab.count() && (rc = m->slab.alloc(tiles))) return rc;
    p.width = width;
    p.height = height;
    p.flags = flags;
    p.map = d_ssim_map;
    p.map_pitch = map_pitch_bytes;
    p.slab = m->slab.get();
    if ((rc = launch_image_metrics(p, m->records.get() + m->count, stream))) return rc;
    ++m->count;
    m->last_stream = stream;
    return WS_OK;
}

int ws_image_error_plane(ws_context* ctx, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, int kind,
                         uint32_t flags, float* d_plane, size_t plane_pitch_bytes, void* stream) {
    return image_error("ws_image_error_plane", ctx, a, b, width, height, kind, flags, d_plane, plane_pitch_bytes, false, stream);
}

int ws_image_error_gradient(ws_context* ctx, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, int kind,
                            uint32_t flags, float* d_grad, size_t grad_pitch_bytes, void* stream) {
    return image_error("ws_image_error_gradient", ctx, a, b, width, height, kind, flags, d_grad, grad_pitch_bytes, true, stream);
}

int ws_metrics_download(ws_metrics* m, uint32_t capacity, ws_image_metrics* out, uint32_t* count) {
    if (!m) return fail(WS_ERR_INVALID, "ws_metrics_download: null accumulator");
    if (count) *count = m->count;
    if (!out) {  // (the count alone)
        WS_HIP(hipStreamSynchronize(m->last_stream));
        return WS_OK;
    }
    if (capacity < m->count) return fail(WS_ERR_INVALID, "ws_metrics_download: capacity smaller than the number of records");
    std::vector<MetricsRecord> recs;
    try {
        recs.resize(m->count);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_metrics_download: host allocation failed");
    }
    WS_HIP(hipStreamSynchronize(m->last_stream));
    const int rc = copy_d2h(recs.data(), m->records.get(), (size_t)m->count * sizeof(MetricsRecord), m->last_stream);
    if (rc) return rc;
    for (uint32_t i = 0; i < m->count; ++i) {
        const MetricsRecord& r = recs[i];
        ws_image_metrics& o = out[i];
        const double n = 3.0 * (double)r.width * (double)r.height;
        o.mse = (r.flags & WS_METRICS_QUANTIZE_U8) ? (double)r.sse_u8 / (255.0 * 255.0 * n) : r.sse / n;
        o.psnr = o.mse == 0.0 ? (double)INFINITY : -10.0 * std::log10(o.mse);
        o.ssim = r.ssim_sum / n;
        o.sse_u8 = r.sse_u8;
        o.width = r.width;
        o.height = r.height;
        o.flags = r.flags;
        o.reserved = 0;
    }
    return WS_OK;
}

}  // extern "C"
