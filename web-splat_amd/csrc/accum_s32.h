// accum_s32.h -- the SIGNED per-Gaussian accumulator of the gradient kernel (gradient.hip): what k_gradient does with four values
// v_ch in (-1, 1) per (pixel, record) pair of tile::walk_weights (weight_walk.h).  A ws_grad holds, per Gaussian, four 64-bit
// two's-complement fixed-point sums.  The rounding rule is written once, here; gradient.h says only what the four v are.
//
// TO THE BIT.  Per walked pair and channel, with the sink's v in (-1, 1):
//   q = (int64_t)(v * 2^32)          exact product (a power of two), |q| < 2^32; the conversion truncates TOWARD ZERO: formed as
//                                    m = (uint32_t)(|v| * 2^32) and q = v < 0 ? -m : m, so v and -v give exactly negated q
// and sum[j][ch] += q over the pairs of Gaussian j.  A pair whose |v| < 2^-32 adds nothing.  Integer sums commute: the result
// does not depend on the order of anything.
//
// THE WAVE SUM.  accum_q32.h's DPP sums are unsigned, so every lane's q is biased by 2^32 first (idle lanes included: their q is
// 0): u = q + 2^32 lies in (0, 2^33), and a wave's 64 values of u sum to (sum of q) + 2^38.  The low 26 bits of u go through one
// 32-bit DPP wave sum per channel (64 x 2^26 = 2^32: no carry is lost); the high 7 bits of two channels share one word, 16 bits
// apart (64 x 2^7 = 2^13 per half): six wave sums per pair for four channels.  Lane-uniform behind them:
//   sum = lo + (hi << 26) - 2^38     in 64-bit two's complement
// The tile's waves meet in LDS, one ds_add_u64 per (wave, record, channel) with a non-zero sum, and behind the batch's walk the
// staging threads flush: one 64-bit global add per (tile, entry, channel) with a non-zero partial, through K1's src_index.
#pragma once

#include "accum_q32.h"

namespace ws {

constexpr int GRAD_CHANNELS = 4;  // colour r, g, b; ln-opacity
constexpr int GEOM_CHANNELS = 5;  // m0, m1, S00, S01, S11 (geometry.h)

}  // namespace ws

#if defined(__HIPCC__)
namespace ws {

// u = q + 2^32 of one lane's v, as (bit 32, low word)
struct BiasedQ {
    uint32_t lo, hi;
    __device__ __forceinline__ uint32_t lo26() const { return lo & 0x03FFFFFFu; }
    __device__ __forceinline__ uint32_t hi7() const { return (hi << 6) | (lo >> 26); }
};
__device__ __forceinline__ BiasedQ biased_q(float v) {
    const uint32_t m = (uint32_t)(fabsf(v) * 4294967296.0f);  // truncates |v| 2^32: toward zero for either sign
    const bool neg = v < 0.0f && m != 0u;
    return {neg ? 0u - m : m, neg ? 0u : 1u};  // 2^32 + m | 2^32 - m
}

// A member of a sink of tile::walk_weights that accumulates signed values (GradientSink).  The sink's stage() calls clear(), its
// pair() add() with its four v, its flush() this one's; it has WRITES_EMPTY_TILES = false and PAIR_IS_WAVE_WIDE = true (the DPP
// reductions must not sit under a divergent branch).  LDS per staged record: four sums of q over the tile's pixels, s_sum[ch][slot].
template <int STAGE>
struct AccumS32 {
    unsigned long long* sums;   // [num_points][GRAD_CHANNELS], two's complement
    unsigned long long* s_sum;  // [GRAD_CHANNELS][STAGE]
    const int lane = threadIdx.x & 63;

    __device__ __forceinline__ void clear(int tid) {
#pragma unroll
        for (int ch = 0; ch < GRAD_CHANNELS; ++ch) s_sum[ch * STAGE + tid] = 0ull;
    }
    __device__ __forceinline__ void add(uint32_t off, float v0, float v1, float v2, float v3) {  // off = slot * 16; every lane of the wave
        const BiasedQ u0 = biased_q(v0), u1 = biased_q(v1), u2 = biased_q(v2), u3 = biased_q(v3);
        const uint32_t l0 = wave_add_u32(u0.lo26()), l1 = wave_add_u32(u1.lo26()), l2 = wave_add_u32(u2.lo26()), l3 = wave_add_u32(u3.lo26());
        const uint32_t h01 = wave_add_u32(u0.hi7() | (u1.hi7() << 16)), h23 = wave_add_u32(u2.hi7() | (u3.hi7() << 16));
        constexpr unsigned long long BIAS = 1ull << 38;  // 64 lanes x 2^32
        const unsigned long long s0 = (unsigned long long)l0 + ((unsigned long long)(h01 & 0xFFFFu) << 26) - BIAS;
        const unsigned long long s1 = (unsigned long long)l1 + ((unsigned long long)(h01 >> 16) << 26) - BIAS;
        const unsigned long long s2 = (unsigned long long)l2 + ((unsigned long long)(h23 & 0xFFFFu) << 26) - BIAS;
        const unsigned long long s3 = (unsigned long long)l3 + ((unsigned long long)(h23 >> 16) << 26) - BIAS;
        if ((s0 | s1 | s2 | s3) != 0ull && lane == 0) {  // (the sums are wave-uniform)
            unsigned long long* s = s_sum + (off >> 4);
            if (s0 != 0ull) atomicAdd(s, s0);
            if (s1 != 0ull) atomicAdd(s + STAGE, s1);
            if (s2 != 0ull) atomicAdd(s + 2 * STAGE, s2);
            if (s3 != 0ull) atomicAdd(s + 3 * STAGE, s3);
        }
    }
    __device__ __forceinline__ void flush(const uint32_t* src_index, int tid, uint32_t idx) {
        unsigned long long s[GRAD_CHANNELS];
#pragma unroll
        for (int ch = 0; ch < GRAD_CHANNELS; ++ch) s[ch] = s_sum[ch * STAGE + tid];
        if ((s[0] | s[1] | s[2] | s[3]) != 0ull) {
            unsigned long long* g = sums + (size_t)src_index[idx] * GRAD_CHANNELS;
#pragma unroll
            for (int ch = 0; ch < GRAD_CHANNELS; ++ch)
                if (s[ch] != 0ull) atomicAdd(g + ch, s[ch]);
        }
    }
};

// The five-channel sibling (geometry.hip, GeometrySink): the same q, the same bias, the same three meeting points.  Five low words
// and three words of high parts (channels 0|1, 2|3, 4): eight wave sums per pair.  AccumS32 above is left as it was, so that
// k_gradient's code does not depend on this one.
template <int STAGE>
struct AccumS32x5 {
    unsigned long long* sums;   // [num_points][GEOM_CHANNELS], two's complement
    unsigned long long* s_sum;  // [GEOM_CHANNELS][STAGE]
    const int lane = threadIdx.x & 63;

    __device__ __forceinline__ void clear(int tid) {
#pragma unroll
        for (int ch = 0; ch < GEOM_CHANNELS; ++ch) s_sum[ch * STAGE + tid] = 0ull;
    }
    __device__ __forceinline__ void add(uint32_t off, const float (&v)[GEOM_CHANNELS]) {  // off = slot * 16; every lane of the wave
        BiasedQ u[GEOM_CHANNELS];
        uint32_t l[GEOM_CHANNELS];
#pragma unroll
        for (int ch = 0; ch < GEOM_CHANNELS; ++ch) u[ch] = biased_q(v[ch]);
#pragma unroll
        for (int ch = 0; ch < GEOM_CHANNELS; ++ch) l[ch] = wave_add_u32(u[ch].lo26());
        const uint32_t h01 = wave_add_u32(u[0].hi7() | (u[1].hi7() << 16)), h23 = wave_add_u32(u[2].hi7() | (u[3].hi7() << 16));
        const uint32_t h4 = wave_add_u32(u[4].hi7());
        constexpr unsigned long long BIAS = 1ull << 38;  // 64 lanes x 2^32
        const uint32_t h[GEOM_CHANNELS] = {h01 & 0xFFFFu, h01 >> 16, h23 & 0xFFFFu, h23 >> 16, h4};
        unsigned long long s[GEOM_CHANNELS], any = 0ull;
#pragma unroll
        for (int ch = 0; ch < GEOM_CHANNELS; ++ch) {
            s[ch] = (unsigned long long)l[ch] + ((unsigned long long)h[ch] << 26) - BIAS;
            any |= s[ch];
        }
        if (any != 0ull && lane == 0) {  // (the sums are wave-uniform)
            unsigned long long* d = s_sum + (off >> 4);
#pragma unroll
            for (int ch = 0; ch < GEOM_CHANNELS; ++ch)
                if (s[ch] != 0ull) atomicAdd(d + ch * STAGE, s[ch]);
        }
    }
    __device__ __forceinline__ void flush(const uint32_t* src_index, int tid, uint32_t idx) {
        unsigned long long s[GEOM_CHANNELS], any = 0ull;
#pragma unroll
        for (int ch = 0; ch < GEOM_CHANNELS; ++ch) any |= (s[ch] = s_sum[ch * STAGE + tid]);
        if (any != 0ull) {
            unsigned long long* g = sums + (size_t)src_index[idx] * GEOM_CHANNELS;
#pragma unroll
            for (int ch = 0; ch < GEOM_CHANNELS; ++ch)
                if (s[ch] != 0ull) atomicAdd(g + ch, s[ch]);
        }
    }
};

}  // namespace ws
#endif  // __HIPCC__
