// accum_q32.h -- the per-Gaussian accumulator of the attribution kernels: what k_contrib (contrib.hip) and k_removal
// (removal.hip) do with a value v per (pixel, record) pair of tile::walk_weights (weight_walk.h).  A ws_contrib holds, per
// Gaussian, a 64-bit fixed-point sum of every v it was given and the bits of the largest one.  Each rounding rule below is
// written once, here; contrib.h and removal.h say only what their v is.
//
// TO THE BIT.  Before the batch loop every lane inside the viewport loads its pixel's value of the caller's plane once,
//   E = fminf(fmaxf(fmaf(scale, plane[p], bias), 0.0f), 1.0f), NaN -> 0;
// a lane outside the viewport loads nothing and has E = 0; nothing past a row's width-th value is read; without a plane nothing
// is loaded and no E is used.  A wave whose 64 values of E are all 0 adds nothing whatever it walks: it skips its walk, keeps
// staging and meeting the barriers, and votes "done" -- the other waves' walks are private to them, and the batch loop ends early
// only when every wave has nothing left to add.  Per walked pair, with the sink's v in [0, 1) (or negative: counted as 0):
//   q32 = (uint32_t)(v * 2^32)       exact product (a power of two), below 2^32; the conversion truncates
//   mb  = q32 ? bits(v) : 0          non-negative floats order as their bits
// A pair whose v truncates to 0 (v < 2^-32) counts in neither result: sum == 0 <=> max == 0.  A wave's 64 values of q32 sum to
// less than 2^38: their low 26 bits and their high 6 bits go through two 32-bit DPP wave sums, mb through a DPP wave max.  The
// tile's waves meet in LDS, one ds_add_u64 + one ds_max_u32 per (wave, record) with a non-zero sum, and behind the batch's walk
// the staging threads flush: one 64-bit add and one 32-bit max per (tile, entry) with a non-zero sum, through K1's src_index,
// into the accumulators.  Integer sums and maxima commute: the result does not depend on the order of anything.
#pragma once

#include <cstddef>

#include "ws_internal.h"

namespace ws {

// The accumulator as a kernel argument: the tail of ContribParams and RemovalParams.
struct Accum {
    unsigned long long* sum_q32;  // [num_points]
    uint32_t* max_bits;           // [num_points] bits of the largest v
    const float* plane;           // f32 per viewport pixel; nullptr: every pair counts in full, and nothing below is read
    size_t plane_pitch;           // bytes
    float scale, bias;
};
static_assert(sizeof(Accum) == 40, "the kernels read their own arguments at the offsets they always had");

}  // namespace ws

#if defined(__HIPCC__)
namespace ws {

// Wave reductions over 64 lanes with DPP, result in lane 63: row_shr 1 / 2 / 4 / 8 leave every row's total in its lane 15,
// row_bcast:15 adds it into the next row (rows 1 and 3), row_bcast:31 adds lane 31 into rows 2 and 3.  Lanes a step does not
// reach read 0, the identity of both operations (unsigned add, unsigned max).
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

// Two members of a sink of tile::walk_weights that accumulates (ContribSink, RemovalSink).  The first: the lane's value E of the
// plane and its wave's vote.  The sink's begin() calls load() under its own `if (inside)` -- one branch for all a lane loads there
// -- and then vote(); its idle() is this one's.  WEIGHTED: the launch has a plane.
template <bool WEIGHTED>
struct PlaneValue {
    float E = 0.0f;     // WEIGHTED: loaded once
    bool none = false;  // wave-uniform: nothing but zeros -- no walk to do

    __device__ __forceinline__ void load(const Accum& arg, uint32_t px, uint32_t py) {  // the lanes inside the viewport only
        if constexpr (WEIGHTED) {
            const float e = fmaf(arg.scale, *reinterpret_cast<const float*>(reinterpret_cast<const char*>(arg.plane) + (size_t)py * arg.plane_pitch + (size_t)px * 4), arg.bias);
            E = (e != e) ? 0.0f : fminf(fmaxf(e, 0.0f), 1.0f);
        }
    }
    __device__ __forceinline__ void vote() {  // every lane, behind load()
        if constexpr (WEIGHTED) none = __ballot(E > 0.0f) == 0ull;
    }
    __device__ __forceinline__ bool idle() const { return WEIGHTED && none; }
};

// The second: the sums and maxima.  The sink's stage() calls clear(), its pair() add() with its v, its flush() this one's; it has
// WRITES_EMPTY_TILES = false and PAIR_IS_WAVE_WIDE = true (the DPP reductions must not sit under a divergent branch).  LDS per
// staged record: the sum of q32 over the tile's pixels and the bits of its largest v.
struct AccumQ32 {
    const Accum& arg;
    unsigned long long* s_sum;
    uint32_t* s_max;
    const int lane = threadIdx.x & 63;

    __device__ __forceinline__ void clear(int tid) {
        s_sum[tid] = 0ull;
        s_max[tid] = 0u;
    }
    __device__ __forceinline__ void add(uint32_t off, float v) {  // off = slot * 16; every lane of the wave
        const uint32_t q32 = (uint32_t)(v * 4294967296.0f);
        const uint32_t mb = q32 ? __float_as_uint(v) : 0u;
        const uint32_t lo = wave_add_u32(q32 & 0x03FFFFFFu), hi6 = wave_add_u32(q32 >> 26), mx = wave_max_u32(mb);
        const unsigned long long sum = (unsigned long long)lo + ((unsigned long long)hi6 << 26);
        if (sum != 0ull && lane == 0) {  // (sum is wave-uniform)
            atomicAdd(&s_sum[off >> 4], sum);
            atomicMax(&s_max[off >> 4], mx);
        }
    }
    __device__ __forceinline__ void flush(const uint32_t* src_index, int tid, uint32_t idx) {
        const unsigned long long s = s_sum[tid];
        if (s != 0ull) {
            const uint32_t src = src_index[idx];
            atomicAdd(arg.sum_q32 + src, s);
            atomicMax(arg.max_bits + src, s_max[tid]);
        }
    }
};

}  // namespace ws
#endif  // __HIPCC__
