// values.hip -- a caller's per-Gaussian values drawn to pixel planes through a prepared frame's weights, and the id of the
// heaviest Gaussian per pixel (include/websplat.h, "Rendering per-Gaussian values").
//
//   k_values : a sink of tile::walk_weights (weight_walk.h), the walk k_contrib runs -- one workgroup per blend tile, one wave
//              per 8x8-pixel quadrant, the tile's binned list staged through LDS near -> far -- plus one 16-B record of values
//              (and the source index) per staged entry.  Every lane keeps what k_contrib reduces away: out(p) = sum of
//              w * f[src], and the src of its largest w.  No atomics, no wave reductions.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "values.h"

namespace ws {

namespace {

constexpr uint32_t NO_WINNER = 0xFFFFFFFFu;

// What k_values does with the walk's weights (weight_walk.h).  LDS per staged record: the values of its source Gaussian, and
// (WINNER) its index in the point cloud.
template <bool WINNER>
struct ValuesSink {
    static constexpr bool WRITES_EMPTY_TILES = true;  // the lanes of a tile with nothing listed store 0.0f and NO_WINNER
    static constexpr bool PAIR_IS_WAVE_WIDE = false;
    const ValuesParams& p;
    float4* s_val;
    uint32_t* s_src;
    float best_w = 0.0f;  // (the winner's two before the sums: the other way round the sums' registers end up rotated against
    uint32_t best_id = NO_WINNER;  //  the LDS read's and every kept pair pays four moves)
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;

    __device__ __forceinline__ void begin(uint32_t, uint32_t, bool) {}
    __device__ __forceinline__ bool idle() const { return false; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        if (!live) return;
        const uint32_t src = p.frame.src_index[idx];
        const float* f = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.values) + (size_t)src * p.stride);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (p.channels > 0u) v.x = f[0];
        if (p.channels > 1u) v.y = f[1];
        if (p.channels > 2u) v.z = f[2];
        if (p.channels > 3u) v.w = f[3];
        s_val[tid] = v;
        if constexpr (WINNER) s_src[tid] = src;
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool) {  // (kept pairs only: one outside the cut-off multiplies nothing)
        const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_val) + off);
        acc0 = fmaf(wgt, v.x, acc0);
        acc1 = fmaf(wgt, v.y, acc1);
        acc2 = fmaf(wgt, v.z, acc2);
        acc3 = fmaf(wgt, v.w, acc3);
        if constexpr (WINNER) {
            if (wgt > best_w) {  // strict: the nearest of equal weights stays, a weight of 0 never wins
                best_w = wgt;
                best_id = s_src[off >> 4];
            }
        }
    }
    __device__ __forceinline__ void flush(int, uint32_t) {}
    __device__ __forceinline__ void finish(uint32_t px, uint32_t py, bool inside) {
        if (!inside) return;
        const size_t x4 = (size_t)px * 4;
        if (p.plane[0]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[0]) + (size_t)py * p.pitch[0] + x4) = acc0;
        if (p.plane[1]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[1]) + (size_t)py * p.pitch[1] + x4) = acc1;
        if (p.plane[2]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[2]) + (size_t)py * p.pitch[2] + x4) = acc2;
        if (p.plane[3]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[3]) + (size_t)py * p.pitch[3] + x4) = acc3;
        if constexpr (WINNER) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(p.winner) + (size_t)py * p.winner_pitch + x4) = best_id;
    }
};

template <int QW, int QH, bool WINNER>
__global__ __launch_bounds__(64 * QW * QH) void k_values(const ValuesParams p) {
    using G = tile::Geometry<QW, QH>;
    __shared__ float4 s_val[G::SLOTS];
    __shared__ uint32_t s_src[WINNER ? G::STAGE : 1];
    ValuesSink<WINNER> sink{p, s_val, s_src};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

}  // namespace

int launch_values(const ValuesParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        if (p.winner) hipLaunchKernelGGL((k_values<QW, QH, true>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
        else hipLaunchKernelGGL((k_values<QW, QH, false>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_values: tile shape");
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
