// metrics.h -- PSNR / SSIM between two resident images (metrics.hip k_image_metrics + k_metrics_finalize).  Internal: the ABI
// and the bit-level definition are in include/websplat.h, "Image metrics"; DESIGN.md 3.4e.
#pragma once

#include "ws_internal.h"

namespace ws {

// the output tile of one workgroup of k_image_metrics, and the SSIM window's reach on every side of it
constexpr uint32_t METRICS_TILE_W = 32, METRICS_TILE_H = 16, METRICS_HALO = 5;

// one image as the metrics see it: texels of `format` (ws_color_format), rows of `pitch` bytes; over_bg: the premultiplied
// texel goes over bg[3] first
struct MetricsView {
    const void* pixels;
    size_t pitch;
    int format;
    int over_bg;
    float bg[3];
};

// what one workgroup leaves of its tile, and -- summed over the slab in index order -- the record of one image pair
struct MetricsPartial {
    double sse;                  // sum of e = d * d (e in f32) over the tile's pixels and three channels
    double ssim_sum;             // sum of the SSIM map over the same
    unsigned long long sse_u8;   // sum of (qx - qy)^2; 0 without WS_METRICS_QUANTIZE_U8
};
struct MetricsRecord {
    double sse, ssim_sum;
    unsigned long long sse_u8;
    uint32_t width, height, flags, reserved;
};

struct MetricsParams {
    MetricsView a, b;
    uint32_t width, height, flags;
    float* map;                  // W x H plane of the per-pixel mean of the three channel maps, or nullptr
    size_t map_pitch;            // bytes
    MetricsPartial* slab;        // [metrics_num_tiles(width, height)]
};

inline uint32_t metrics_num_tiles(uint32_t w, uint32_t h) {
    return ((w + METRICS_TILE_W - 1) / METRICS_TILE_W) * ((h + METRICS_TILE_H - 1) / METRICS_TILE_H);
}
// k_image_error: plane[p] = the mean over the three colour channels of e = d * d (WS_ERROR_SQ) or |d| (WS_ERROR_ABS), d = x - y on
// the PIXEL VALUES k_image_metrics compares (the same device function), ((e_r + e_g) + e_b) / 3.0f in f32, one thread per pixel
// k_image_error_grad (gradient != 0): per pixel the float4 (g_r, g_g, g_b, 0), g_ch the derivative of that plane's value with
// respect to a's pixel value: d = x - y; (2 * d) / 3.0f (SQ: one rounded multiply, IEEE division) or copysign(1 / 3.0f, d), 0 at
// d == 0 (ABS); 0 where a's value before the clamp lay outside [0, 1] or was NaN.  No quantisation.
struct ImageErrorParams {
    MetricsView a, b;
    uint32_t width, height, flags;
    int kind;                    // WS_ERROR_SQ / WS_ERROR_ABS
    float* plane;                // W x H
    size_t plane_pitch;          // bytes
    int gradient = 0;            // k_image_error_grad instead: plane holds one float4 per pixel
};
int launch_image_error(const ImageErrorParams& p, hipStream_t stream);

// k_image_metrics over the pair, then the one-workgroup sum of its slab into *record, both on `stream`
int launch_image_metrics(const MetricsParams& p, MetricsRecord* record, hipStream_t stream);

}  // namespace ws
