// removal.hip -- what deleting each Gaussian alone would do to a prepared frame (include/websplat.h, "Removal effect"; DESIGN.md
// 3.4h).  With F the FAST blend's image of the frame's pairs over a background and splat i taken out, every weight behind i at
// pixel p grows by 1 / (1 - b_i) and nothing in front moves: the pixel changes by d = r (F - P_i) - w c_i, r = w / T_after_i, P_i
// the colour accumulated near -> far through i.  Two sinks of tile::walk_weights (weight_walk.h), the walk k_contrib runs:
//
//   k_removal_base : F and the final T per pixel -- k_values with the colour taken from the Splat record.  Every lane keeps
//                    acc = sum of w c and its own copy of T; no atomics, no wave reductions; empty tiles get (background, 1).
//   k_removal      : per walked pair the lane's v = min(scale * mean_ch e(d), 1 - 2^-24) (times E of a weight plane), reduced
//                    exactly as k_contrib reduces its weights: q32 = (uint32_t)(v 2^32), DPP wave sums of the split q32 and a DPP
//                    max of the bits, one ds_add_u64 + one ds_max_u32 per (wave, record), and behind the batch's walk one 64-bit
//                    add and one 32-bit max per (tile, entry) with a non-zero sum, through K1's src_index.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "removal.h"

namespace ws {

namespace {

typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

// Words 3 and 4 of the 20-B Splat record: the f16 colour (r, g | b) and opacity.  Kept raw in LDS, 8 B per slot: decoded float4s
// would take the 4x4 tile's static LDS to 64.6 KB of 64 (profiles/removal/resources.txt).
__device__ __forceinline__ uint2 splat_colour_words(const uint8_t* splats, uint32_t idx) {
    const char* sp = reinterpret_cast<const char*>(splats) + (size_t)idx * SPLAT_STRIDE + 12;
    uint2 c;
    __builtin_memcpy(&c.x, sp, 4);
    __builtin_memcpy(&c.y, sp + 4, 4);
    return c;
}
__device__ __forceinline__ f16x4_t staged_colour(const uint2* s_col, uint32_t off) {  // off = slot * 16
    return *reinterpret_cast<const f16x4_t*>(reinterpret_cast<const char*>(s_col) + (off >> 1));
}

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

// Wave reductions over 64 lanes with DPP, result in lane 63 (contrib.hip's, copied: that file's code object stays as it is).
// row_shr 1 / 2 / 4 / 8 leave every row's total in its lane 15, row_bcast:15 adds it into the next row (rows 1 and 3),
// row_bcast:31 adds lane 31 into rows 2 and 3.  Lanes a step does not reach read 0, the identity of unsigned add and max.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) {
    v += dpp0<0x111, 0xF>(v);
    v += dpp0<0x112, 0xF>(v);
    v += dpp0<0x114, 0xF>(v);
    v += dpp0<0x118, 0xF>(v);
    v += dpp0<0x142, 0xA>(v);
    v += dpp0<0x143, 0xC>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = umax(v, dpp0<0x111, 0xF>(v));
    v = umax(v, dpp0<0x112, 0xF>(v));
    v = umax(v, dpp0<0x114, 0xF>(v));
    v = umax(v, dpp0<0x118, 0xF>(v));
    v = umax(v, dpp0<0x142, 0xA>(v));
    v = umax(v, dpp0<0x143, 0xC>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

constexpr float V_CAP = 0x1.fffffep-1f;  // the largest f32 below 1: v * 2^32 fits 32 bits

// Pass 2 (removal.h).  LDS per staged record: its colour words, the sum of q32 over the tile's pixels and the bits of its largest v.
template <bool WEIGHTED, int KIND>
struct RemovalSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;  // the DPP reductions must not sit under a divergent branch
    const RemovalParams& p;
    uint2* s_col;
    unsigned long long* s_sum;
    uint32_t* s_max;
    const int lane = threadIdx.x & 63;
    float F0 = 0.0f, F1 = 0.0f, F2 = 0.0f;  // base(p)
    float P0 = 0.0f, P1 = 0.0f, P2 = 0.0f;  // the colour accumulated through the pair at hand
    float T = 0.0f;                         // the walk's T again
    float E = 0.0f;                         // WEIGHTED: the lane's value of the plane, loaded once
    bool none = false;                      // wave-uniform: nothing but zeros -- no walk to do

    __device__ __forceinline__ void begin(uint32_t px, uint32_t py, bool inside) {
        if (inside) {
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.base) + (size_t)py * p.base_pitch + (size_t)px * 16);
            F0 = b.x, F1 = b.y, F2 = b.z;
            T = 1.0f;
        }
        if constexpr (WEIGHTED) {
            if (inside) {
                const float e = fmaf(p.plane_scale, *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.plane) + (size_t)py * p.plane_pitch + (size_t)px * 4), p.plane_bias);
                E = (e != e) ? 0.0f : fminf(fmaxf(e, 0.0f), 1.0f);
            }
            none = __ballot(E > 0.0f) == 0ull;
        }
    }
    __device__ __forceinline__ bool idle() const { return WEIGHTED && none; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        s_sum[tid] = 0ull;
        s_max[tid] = 0u;
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
                    if constexpr (WEIGHTED) v = v * E;
                }
            }
        }
        // v < 1: v * 2^32 is exact in f32 and below 2^32; the conversion truncates.  A pair whose v truncates to 0 counts in
        // neither result: sum == 0 <=> max == 0.
        const uint32_t q32 = (uint32_t)(v * 4294967296.0f);
        const uint32_t mb = q32 ? __float_as_uint(v) : 0u;
        // 64 values below 2^32 sum to less than 2^38: the low 26 bits and the high 6 bits as two 32-bit sums
        const uint32_t lo = wave_add_u32(q32 & 0x03FFFFFFu), hi6 = wave_add_u32(q32 >> 26), mx = wave_max_u32(mb);
        const unsigned long long sum = (unsigned long long)lo + ((unsigned long long)hi6 << 26);
        if (sum != 0ull && lane == 0) {  // (sum is wave-uniform)
            atomicAdd(&s_sum[off >> 4], sum);
            atomicMax(&s_max[off >> 4], mx);
        }
    }
    // one add + one max per (tile, entry) with any effect, into the accumulators of its source Gaussian
    __device__ __forceinline__ void flush(int tid, uint32_t idx) {
        const unsigned long long s = s_sum[tid];
        if (s != 0ull) {
            const uint32_t src = p.frame.src_index[idx];
            atomicAdd(p.sum_q32 + src, s);
            atomicMax(p.max_bits + src, s_max[tid]);
        }
    }
    __device__ __forceinline__ void finish(uint32_t, uint32_t, bool) {}
};

template <int QW, int QH, bool WEIGHTED, int KIND>
__global__ __launch_bounds__(64 * QW * QH) void k_removal(const RemovalParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ uint2 s_col[STAGE];
    __shared__ unsigned long long s_sum[STAGE];
    __shared__ uint32_t s_max[STAGE];
    RemovalSink<WEIGHTED, KIND> sink{p, s_col, s_sum, s_max};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

}  // namespace

int launch_removal(const RemovalParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool weighted = p.plane != nullptr;
    const bool sq = p.kind == WS_ERROR_SQ;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        const dim3 g(grid), b(64 * QW * QH);
        hipLaunchKernelGGL((k_removal_base<QW, QH>), g, b, 0, stream, p);
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
