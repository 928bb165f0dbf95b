// removal.hip -- what deleting each Gaussian alone would do to a prepared frame (include/websplat.h, "Removal effect"; DESIGN.md
// 3.4h).  With F the FAST blend's image of the frame's pairs over a background and splat i taken out, every weight behind i at
// pixel p grows by 1 / (1 - b_i) and nothing in front moves: the pixel changes by d = r (F - P_i) - w c_i, r = w / T_after_i, P_i
// the colour accumulated near -> far through i.  Two sinks of tile::walk_weights (weight_walk.h), the walk k_contrib runs:
//
//   k_removal_base : F and the final T per pixel -- k_values with the colour taken from the Splat record.  Every lane keeps
//                    acc = sum of w c and its own copy of T; no atomics, no wave reductions; empty tiles get (background, 1).
//   k_removal      : per walked pair the lane's v = min(scale * mean_ch e(d), 1 - 2^-24) (times E of a weight plane), into the
//                    per-Gaussian accumulator k_contrib feeds with its weights (accum_q32.h).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "removal.h"

namespace ws {

namespace {

// Pass 1 (removal.h): F = sum of w c + T_end * background, and T_end.
struct RemovalBaseSink {
    static constexpr bool WRITES_EMPTY_TILES = true;  // the lanes of a tile with nothing listed store (background, 1)
    static constexpr bool PAIR_IS_WAVE_WIDE = false;
    const RemovalParams& p;
    uint2* s_col;
    float T = 0.0f;  // the walk's T again: the same start, the same subtractions of the same rounded weights
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;

    __device__ __forceinline__ void begin(uint32_t, uint32_t, bool inside) { T = inside ? 1.0f : 0.0f; }
    __device__ __forceinline__ bool idle() const { return false; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        if (live) s_col[tid] = splat_colour_words(p.frame.splats, idx);
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool) {  // (kept pairs only)
        const f16x4_t c = staged_colour(s_col, off);
        acc0 = fmaf(wgt, (float)c.x, acc0);
        acc1 = fmaf(wgt, (float)c.y, acc1);
        acc2 = fmaf(wgt, (float)c.z, acc2);
        T -= wgt;
    }
    __device__ __forceinline__ void flush(int, uint32_t) {}
    __device__ __forceinline__ void finish(uint32_t px, uint32_t py, bool inside) {
        if (!inside) return;
        const float4 out = make_float4(fmaf(T, p.background[0], acc0), fmaf(T, p.background[1], acc1), fmaf(T, p.background[2], acc2), T);
        *reinterpret_cast<float4*>(reinterpret_cast<char*>(p.base) + (size_t)py * p.base_pitch + (size_t)px * 16) = out;
    }
};

template <int QW, int QH>
__global__ __launch_bounds__(64 * QW * QH) void k_removal_base(const RemovalParams p) {
    __shared__ uint2 s_col[tile::Geometry<QW, QH>::STAGE];
    RemovalBaseSink sink{p, s_col};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

constexpr float V_CAP = 0x1.fffffep-1f;  // the largest f32 below 1: v * 2^32 fits 32 bits

// Pass 2 (removal.h): v per walked pair, into the accumulator (accum_q32.h).  LDS per staged record: its colour words beside the
// accumulator's partials.
template <bool WEIGHTED, int KIND>
struct RemovalSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;
    const RemovalParams& p;
    uint2* s_col;
    AccumQ32 acc;
    float F0 = 0.0f, F1 = 0.0f, F2 = 0.0f;  // base(p)
    float P0 = 0.0f, P1 = 0.0f, P2 = 0.0f;  // the colour accumulated through the pair at hand
    float T = 0.0f;                         // the walk's T again
    PlaneValue<WEIGHTED> plane;

    __device__ __forceinline__ void begin(uint32_t px, uint32_t py, bool inside) {
        if (inside) {
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.base) + (size_t)py * p.base_pitch + (size_t)px * 16);
            F0 = b.x, F1 = b.y, F2 = b.z;
            T = 1.0f;
            plane.load(p.acc, px, py);
        }
        plane.vote();
    }
    __device__ __forceinline__ bool idle() const { return plane.idle(); }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        acc.clear(tid);
        if (live) s_col[tid] = splat_colour_words(p.frame.splats, idx);
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool kept) {
        float v = 0.0f;
        {
#pragma clang fp contract(off)  // every step below is the separately rounded operation removal.h names; the fmaf calls stay fused
            const float Tb = T;
            T = Tb - wgt;
            if (kept) {
                const f16x4_t c16 = staged_colour(s_col, off);
                const float c0 = (float)c16.x, c1 = (float)c16.y, c2 = (float)c16.z;
                P0 = fmaf(wgt, c0, P0);
                P1 = fmaf(wgt, c1, P1);
                P2 = fmaf(wgt, c2, P2);
                if (wgt > 0.0f && Tb >= T_MIN) {  // (T > 0: b <= 0.99)
                    const float r = wgt / T;
                    const float d0 = fmaf(r, F0 - P0, -(wgt * c0));
                    const float d1 = fmaf(r, F1 - P1, -(wgt * c1));
                    const float d2 = fmaf(r, F2 - P2, -(wgt * c2));
                    const float e0 = KIND == WS_ERROR_SQ ? d0 * d0 : fabsf(d0);
                    const float e1 = KIND == WS_ERROR_SQ ? d1 * d1 : fabsf(d1);
                    const float e2 = KIND == WS_ERROR_SQ ? d2 * d2 : fabsf(d2);
                    const float m = ((e0 + e1) + e2) / 3.0f;
                    const float sm = p.scale * m;
                    v = (sm != sm) ? 0.0f : fminf(sm, V_CAP);
                    if constexpr (WEIGHTED) v = v * plane.E;
                }
            }
        }
        acc.add(off, v);
    }
    __device__ __forceinline__ void flush(int tid, uint32_t idx) { acc.flush(p.frame.src_index, tid, idx); }
    __device__ __forceinline__ void finish(uint32_t, uint32_t, bool) {}
};

template <int QW, int QH, bool WEIGHTED, int KIND>
__global__ __launch_bounds__(64 * QW * QH) void k_removal(const RemovalParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ uint2 s_col[STAGE];
    __shared__ unsigned long long s_sum[STAGE];
    __shared__ uint32_t s_max[STAGE];
    RemovalSink<WEIGHTED, KIND> sink{p, s_col, {p.acc, s_sum, s_max}};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

}  // namespace

int launch_removal_base(const RemovalParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        hipLaunchKernelGGL((k_removal_base<QW, QH>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_removal_base: tile shape");
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_removal(const RemovalParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    if (const int rc = launch_removal_base(p, stream)) return rc;
    const bool weighted = p.acc.plane != nullptr;
    const bool sq = p.kind == WS_ERROR_SQ;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        const dim3 g(grid), b(64 * QW * QH);
        if (weighted && sq) hipLaunchKernelGGL((k_removal<QW, QH, true, WS_ERROR_SQ>), g, b, 0, stream, p);
        else if (weighted) hipLaunchKernelGGL((k_removal<QW, QH, true, WS_ERROR_ABS>), g, b, 0, stream, p);
        else if (sq) hipLaunchKernelGGL((k_removal<QW, QH, false, WS_ERROR_SQ>), g, b, 0, stream, p);
        else hipLaunchKernelGGL((k_removal<QW, QH, false, WS_ERROR_ABS>), g, b, 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_removal: tile shape");
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
