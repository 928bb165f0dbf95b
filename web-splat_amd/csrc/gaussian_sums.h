// gaussian_sums.h -- the store under the per-Gaussian accumulators of the ABI (ws_contrib, ws_grad, ws_shgrad, ws_geomgrad): a device array
// of 64-bit sums, so many words per Gaussian, with the frames added and the stream of the last launch, and the three things every
// accumulator does with it.  Host only; the functions are defined in api_attrib.cpp beside the handles' entry points.  They take
// the handle as the ABI got it and the entry point's name: "<who>: null accumulator" is the first refusal of each.
#pragma once

#include <functional>

#include "ws_internal.h"

namespace ws {

struct __attribute__((visibility("hidden"))) GaussianSums {  // (between the ABI's units: not among the library's dynamic symbols)
    ws_context* ctx = nullptr;
    uint32_t num_points = 0;
    DeviceBuf<unsigned long long> sums;  // words per point x num_points; which of the two is the outer index is the handle's
    uint32_t frames = 0;
    hipStream_t last_stream = nullptr;
    // what a handle with a plane of its own merges: (the device copy of the uploaded words or nullptr, the last stream) -> status
    using Merge = std::function<int(const unsigned long long*, hipStream_t)>;

    void launched(hipStream_t stream) { ++frames, last_stream = stream; }  // a launch on `stream` added a frame
    static int reset(GaussianSums* s, const char* who, hipStream_t stream);  // zeros and no frames; `stream` becomes the last stream
    // Refuses a capacity below num_points when the caller gave an array to fill (`wanted`: dst, or another where the handle has
    // more), waits for the last stream -- also with nothing to fill -- and copies every word to dst (nullptr: none).  Never on the
    // legacy NULL stream: see copy_d2h (api_state.h).
    static int download_words(GaussianSums* s, const char* who, uint32_t capacity, bool wanted, void* dst);
    // Refuses n below num_points; with neither host_words nor `merge` it then returns without touching the device.  Else
    // host_words go to a temporary device buffer, `merge` (default: k_grad_merge over every word, sums += host_words) launches
    // on the last stream, and the stream is waited for whatever came of it.
    static int merge_words(GaussianSums* s, const char* who, uint32_t n, const void* host_words, const Merge& merge = nullptr);
};

}  // namespace ws

// ---- per-Gaussian contributions (include/websplat.h; contrib.hip) ----------------------------------------
struct ws_contrib : ws::GaussianSums {   // sums: [num_points] q32
    ws::DeviceBuf<uint32_t> max_bits;    // [num_points] bits of the largest weight (non-negative floats order as their bits)
};
// ---- gradients of an image loss (include/websplat.h "Gradients of an image loss"; gradient.hip) ----------------
struct ws_grad : ws::GaussianSums {};    // sums: [num_points][WS_GRAD_CHANNELS] two's-complement q32 sums
// ---- SH gradients (include/websplat.h "SH gradients"; sh_gradient.hip) ----
struct ws_shgrad : ws::GaussianSums {    // sums: [3 ncoef + 1][num_points]: one plane per element, the opacity's last
    uint32_t sh_deg = 0, ncoef = 1;
    ws::DeviceBuf<unsigned long long> scratch;  // [num_points][WS_GRAD_CHANNELS]: one frame's sums, zero between the calls
};
// ---- geometry gradients (include/websplat.h "Geometry gradients"; geometry.hip, geometry_spread.hip) ----
struct ws_geomgrad : ws::GaussianSums {  // sums: [11][num_points]: ten planes of f64 bits (position 3, covariance 6, screen_norm), then seen
    ws::DeviceBuf<unsigned long long> scratch;  // [num_points][5] int64: one frame's screen-space sums, zero between the calls
};

// ---- a gradient pass over a prepared frame (ws_internal_gradient_passes: ws_internal.h, api_attrib.cpp), as its callers describe it
namespace ws {

// Where the pass adds: one of the three gradient accumulators, as the store every one of them is.  acc may be null (the ABI's
// caller passed it so): the pass refuses that in its turn.
enum GradKind { GRAD_COLOUR = 0, GRAD_SH = 1, GRAD_GEOMETRY = 2 };
struct GradTarget {
    GradKind kind;
    GaussianSums* acc;
    GradTarget(ws_grad* g) : kind(GRAD_COLOUR), acc(g) {}
    GradTarget(ws_shgrad* g) : kind(GRAD_SH), acc(g) {}
    GradTarget(ws_geomgrad* g) : kind(GRAD_GEOMETRY), acc(g) {}
    ws_shgrad* sh() const { return kind == GRAD_SH ? static_cast<ws_shgrad*>(acc) : nullptr; }
    ws_geomgrad* geo() const { return kind == GRAD_GEOMETRY ? static_cast<ws_geomgrad*>(acc) : nullptr; }
};

// Which launches, the same for every target.  A frame is counted by the step that completes it: a ws_grad's by GRAD_SUMS, a
// target's with a spread by GRAD_SPREAD.
enum GradSteps : unsigned {
    GRAD_BASE = 1u,    // k_removal_base: the base image (F, T_end)
    GRAD_SUMS = 2u,    // the walk, k_gradient or k_geometry, into a ws_grad's sums or the target's scratch
    GRAD_SPREAD = 4u,  // k_sh_spread or k_geom_spread from the scratch into the sums; nothing for a ws_grad
    GRAD_ALL = 7u,
};

// What ws_gradient_params and ws_geometry_params say, under one set of names
struct GradDesc {
    float background[3] = {0.0f, 0.0f, 0.0f};
    float scale = 1.0f;
    float second_scale = 1.0f;  // opacity_scale; geometry_scale for a GRAD_GEOMETRY target
    const float* d_grad = nullptr;
    size_t grad_pitch_bytes = 0;
    float* d_base = nullptr;  // may be null: the renderer's scratch plane
    size_t base_pitch_bytes = 0;
};

}  // namespace ws
