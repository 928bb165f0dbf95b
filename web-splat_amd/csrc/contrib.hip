// contrib.hip -- what each Gaussian of the resident scene did to a prepared frame (include/websplat.h, "Per-Gaussian
// contributions"), and the device gather of ws_pointcloud_create_subset.
//
//   k_contrib       : a sink of tile::walk_weights (weight_walk.h) -- one workgroup per blend tile, one wave per 8x8-pixel
//                     quadrant, the tile's binned list staged through LDS near -> far by the calls k_blend stages it with
//                     (blend_tile.h: batches, decode + quadrant masks, per-wave compaction).  No pixel is written: per staged record every lane converts its weight w = b T to
//                     q32 = (uint32_t)(w 2^32), the wave reduces sum and max as INTEGERS (DPP), the tile's waves meet in LDS
//                     (one ds_add_u64 + one ds_max_u32 per (wave, record)), and after the batch's walk the staging threads
//                     flush: one 64-bit add and one 32-bit max per (tile, entry) with a non-zero sum, through K1's
//                     src_index, into the accumulators.  Integer sums and maxima commute: the result does not depend on
//                     the order of anything.  WEIGHTED (contrib.h): every weight is multiplied by the lane's value E of a
//                     caller's f32 plane before the conversion; T, the kept pairs and the early exits do not see E.
//   k_contrib_merge : accumulator += host arrays of another accumulator (ws_contrib_add)
//   k_pc_gather     : the kept Gaussians' records, plane by plane
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "contrib.h"

namespace ws {

namespace {

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

// What k_contrib does with the walk's weights (weight_walk.h).  LDS per staged record: the sum of q32 over the tile's pixels and
// the bits of its largest weight.
template <bool WEIGHTED>
struct ContribSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;  // the DPP reductions must not sit under a divergent branch
    const ContribParams& p;
    unsigned long long* s_sum;
    uint32_t* s_max;
    const int lane = threadIdx.x & 63;
    float E = 0.0f;     // WEIGHTED: the lane's value of the plane, loaded once
    bool none = false;  // wave-uniform: nothing but zeros -- no walk to do

    __device__ __forceinline__ void begin(uint32_t px, uint32_t py, bool inside) {
        if constexpr (WEIGHTED) {
            if (inside) {
                const float e = fmaf(p.scale, *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.plane) + (size_t)py * p.plane_pitch + (size_t)px * 4), p.bias);
                E = (e != e) ? 0.0f : fminf(fmaxf(e, 0.0f), 1.0f);
            }
            none = __ballot(E > 0.0f) == 0ull;
        }
    }
    __device__ __forceinline__ bool idle() const { return WEIGHTED && none; }
    __device__ __forceinline__ void stage(int tid, uint32_t, bool) {
        s_sum[tid] = 0ull;
        s_max[tid] = 0u;
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool) {
        // w < 1: w * 2^32 is exact in f32 and below 2^32; the conversion truncates (and takes anything negative to 0).
        // A pair whose weight truncates to 0 (w < 2^-32) counts in neither result: sum == 0 <=> max == 0.
        if constexpr (WEIGHTED) {
#pragma clang fp contract(off)  // v = w E, one rounded multiply of the rounded w (T has already moved on by w itself)
            wgt = wgt * E;
        }
        const uint32_t q32 = (uint32_t)(wgt * 4294967296.0f);
        const uint32_t mb = q32 ? __float_as_uint(wgt) : 0u;
        // 64 values below 2^32 sum to less than 2^38: the low 26 bits and the high 6 bits as two 32-bit sums
        const uint32_t lo = wave_add_u32(q32 & 0x03FFFFFFu), hi6 = wave_add_u32(q32 >> 26), mx = wave_max_u32(mb);
        const unsigned long long sum = (unsigned long long)lo + ((unsigned long long)hi6 << 26);
        if (sum != 0ull && lane == 0) {  // (sum is wave-uniform)
            atomicAdd(&s_sum[off >> 4], sum);
            atomicMax(&s_max[off >> 4], mx);
        }
    }
    // one add + one max per (tile, entry) that drew anything, into the accumulators of its source Gaussian
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

template <int QW, int QH, bool WEIGHTED>
__global__ __launch_bounds__(64 * QW * QH) void k_contrib(const ContribParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ unsigned long long s_sum[STAGE];
    __shared__ uint32_t s_max[STAGE];
    ContribSink<WEIGHTED> sink{p, s_sum, s_max};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

constexpr int SMALL_THREADS = 256;

__global__ __launch_bounds__(SMALL_THREADS) void k_contrib_merge(unsigned long long* __restrict__ sum, uint32_t* __restrict__ max_bits,
                                                                 const unsigned long long* __restrict__ add_sum,
                                                                 const uint32_t* __restrict__ add_max, uint32_t n) {
    const uint32_t i = blockIdx.x * SMALL_THREADS + threadIdx.x;
    if (i >= n) return;
    if (add_sum) sum[i] += add_sum[i];
    if (add_max) max_bits[i] = umax(max_bits[i], add_max[i]);
}

// thread t copies 32-bit word t % words of record t / words of plane blockIdx.y
__global__ __launch_bounds__(SMALL_THREADS) void k_pc_gather(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                             const uint32_t* __restrict__ indices, uint32_t n_src, uint32_t n,
                                                             uint32_t words) {
    const uint64_t t = (uint64_t)blockIdx.x * SMALL_THREADS + threadIdx.x;
    const uint64_t i = t / words;
    const uint32_t w = (uint32_t)(t % words);
    if (i >= n) return;
    const uint64_t plane = blockIdx.y;
    dst[(plane * n + i) * words + w] = src[(plane * n_src + indices[i]) * words + w];
}

}  // namespace

int launch_contrib(const ContribParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool weighted = p.plane != nullptr;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        if (weighted) hipLaunchKernelGGL((k_contrib<QW, QH, true>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
        else hipLaunchKernelGGL((k_contrib<QW, QH, false>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_contrib: tile shape");
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_contrib_merge(unsigned long long* sum, uint32_t* max_bits, const unsigned long long* add_sum, const uint32_t* add_max,
                         uint32_t n, hipStream_t stream) {
    if (n == 0) return WS_OK;
    hipLaunchKernelGGL(k_contrib_merge, dim3((n + SMALL_THREADS - 1) / SMALL_THREADS), dim3(SMALL_THREADS), 0, stream, sum, max_bits,
                       add_sum, add_max, n);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_pc_gather(const uint32_t* src, uint32_t* dst, const uint32_t* indices, uint32_t n_src, uint32_t n, uint32_t planes,
                     uint32_t words, hipStream_t stream) {
    if (n == 0 || planes == 0) return WS_OK;
    const uint64_t threads = (uint64_t)n * words;
    hipLaunchKernelGGL(k_pc_gather, dim3((uint32_t)((threads + SMALL_THREADS - 1) / SMALL_THREADS), planes), dim3(SMALL_THREADS), 0,
                       stream, src, dst, indices, n_src, n, words);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
