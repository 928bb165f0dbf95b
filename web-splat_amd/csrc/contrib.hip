// contrib.hip -- what each Gaussian of the resident scene did to a prepared frame (include/websplat.h, "Per-Gaussian
// contributions"), and the device gather of ws_pointcloud_create_subset.
//
//   k_contrib       : a sink of tile::walk_weights (weight_walk.h) -- one workgroup per blend tile, one wave per 8x8-pixel
//                     quadrant, the tile's binned list staged through LDS near -> far by the calls k_blend stages it with
//                     (blend_tile.h: batches, decode + quadrant masks, per-wave compaction).  No pixel is written: every
//                     weight w = b T goes into the per-Gaussian accumulator (accum_q32.h: integer sums and maxima, whose
//                     result does not depend on the order of anything).  WEIGHTED (contrib.h): every weight is multiplied by
//                     the lane's value E of a caller's f32 plane first; T, the kept pairs and the early exits do not see E.
//   k_contrib_merge : accumulator += host arrays of another accumulator (ws_contrib_add)
//   k_pc_gather     : the kept Gaussians' records, plane by plane
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "contrib.h"

namespace ws {

namespace {

// What k_contrib does with the walk's weights (weight_walk.h): v = wgt, or wgt * E with a plane, into the accumulator (accum_q32.h).
template <bool WEIGHTED>
struct ContribSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;
    const ContribParams& p;
    AccumQ32 acc;
    PlaneValue<WEIGHTED> plane;

    __device__ __forceinline__ void begin(uint32_t px, uint32_t py, bool inside) {
        if (inside) plane.load(p.acc, px, py);
        plane.vote();
    }
    __device__ __forceinline__ bool idle() const { return plane.idle(); }
    __device__ __forceinline__ void stage(int tid, uint32_t, bool) { acc.clear(tid); }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool) {
        if constexpr (WEIGHTED) {
#pragma clang fp contract(off)  // v = w E, one rounded multiply of the rounded w (T has already moved on by w itself)
            wgt = wgt * plane.E;
        }
        acc.add(off, wgt);
    }
    __device__ __forceinline__ void flush(int tid, uint32_t idx) { acc.flush(p.frame.src_index, tid, idx); }
    __device__ __forceinline__ void finish(uint32_t, uint32_t, bool) {}
};

template <int QW, int QH, bool WEIGHTED>
__global__ __launch_bounds__(64 * QW * QH) void k_contrib(const ContribParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ unsigned long long s_sum[STAGE];
    __shared__ uint32_t s_max[STAGE];
    ContribSink<WEIGHTED> sink{p, {p.acc, s_sum, s_max}};
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
    const bool weighted = p.acc.plane != nullptr;
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
