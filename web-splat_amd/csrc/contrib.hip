// contrib.hip -- what each Gaussian of the resident scene did to a prepared frame (include/websplat.h, "Per-Gaussian
// contributions"), and the device gather of ws_pointcloud_create_subset.
//
//   k_contrib       : one workgroup per blend tile, one wave per 8x8-pixel quadrant, the tile's binned list staged through
//                     LDS near -> far by the calls k_blend stages it with (blend_tile.h: batches, decode + quadrant masks,
//                     per-wave compaction).  No pixel is written: per staged record every lane converts its weight w = b T to
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

#include "blend_tile.h"
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

template <int QW, int QH, bool WEIGHTED>
__global__ __launch_bounds__(64 * QW * QH) void k_contrib(const ContribParams p) {
    using G = tile::Geometry<QW, QH>;
    constexpr int NW = G::NW, NT = G::NT, STAGE = G::STAGE, SLOTS = G::SLOTS, LCAP = G::LCAP, TW = G::TW, TH = G::TH;

    __shared__ float4 s_rec[2 * SLOTS];                                  // the two planes of 16-B records (blend_tile.h)
    __shared__ __attribute__((aligned(16))) uint16_t s_m[STAGE];        // quadrant masks, transposed per sub-round
    __shared__ __attribute__((aligned(16))) uint32_t s_list[NW][LCAP];  // per wave: byte offsets of the records that reach it
    __shared__ unsigned long long s_sum[STAGE];                          // per staged record: sum of q32 over the tile's pixels
    __shared__ uint32_t s_max[STAGE];                                    //   and the bits of its largest weight

    // No blend need follow (ws_scene_accumulate_contrib): the frame's error bits reach the renderer's sticky words from here too
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.sticky) tile::fold_frame_errors(p.counters, p.sticky, p.demand_mailbox);
    const uint32_t tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;  // (the grid is tiles_x * tiles_y)
    const int tid = threadIdx.x;
    const tile::Quadrant me = tile::quadrant<QW>(tid);
    const int wave = me.wave, lane = me.lane;
    const float lx = me.lx, ly = me.ly;
    const bool stager = NT == STAGE || tid < STAGE;  // wave-uniform
    // the binned list of this tile: its own, or -- the frame binned at twice the blend's tile size -- its 2 x 2 block's
    uint2 range = p.tile_ranges[tile::list_index(tx, ty, p.counters->bin_shift, p.tiles_x, 0u)];
    range.x = tile::range_begin(range.x, range.y);
    if (range.y <= range.x) return;  // block-uniform: nothing listed
    const uint32_t px = me.px(tx * TW), py = me.py(ty * TH);
    // pixels outside the viewport start with T = 0: every weight is 0 and they count as saturated
    float T = (px < p.width && py < p.height) ? 1.0f : 0.0f;
    const float W = (float)p.width, H = (float)p.height;
    const float tile_x0 = (float)(tx * TW), tile_y0 = (float)(ty * TH);
    uint32_t* my_list = s_list[wave];
    // WEIGHTED: the lane's value of the plane, loaded once; a wave with nothing but zeros has no walk to do
    float E = 0.0f;
    bool idle = false;  // wave-uniform
    if constexpr (WEIGHTED) {
        if (px < p.width && py < p.height) {
            const float e = fmaf(p.scale, *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.plane) + (size_t)py * p.plane_pitch + (size_t)px * 4), p.bias);
            E = (e != e) ? 0.0f : fminf(fmaxf(e, 0.0f), 1.0f);
        }
        idle = __ballot(E > 0.0f) == 0ull;
    }

    uint32_t hi = range.y;
    while (hi > range.x) {
        const uint32_t nb = tile::batch_len<STAGE>(range.x, hi);
        uint32_t idx = 0u;
        if (stager) {
            uint32_t mask = 0u;
            idx = tile::entry_idx<STAGE>(p.entry_vals, range, hi, tid);
            if ((uint32_t)tid < nb) mask = tile::stage_store<QW, QH, SLOTS>(s_rec, tid, tile::gather(p.splats, idx), W, H, tile_x0, tile_y0);
            s_m[tile::mask_slot<LCAP>((uint32_t)tid, (uint32_t)lane)] = (uint16_t)mask;
            s_sum[tid] = 0ull;
            s_max[tid] = 0u;
        }
        __syncthreads();
        // a wave whose 64 pixels are saturated only keeps staging
        for (uint32_t sub = 0; sub < nb && !(WEIGHTED && idle) && __ballot(T >= T_MIN) != 0ull; sub += (uint32_t)LCAP) {
            // wave-private compaction: records whose kept ellipse reaches this quadrant, near -> far
            const uint32_t n = tile::compact<LCAP, true>(s_m, my_list, sub, nb, lane, me.bit, tile::list_value(sub + (uint32_t)lane));
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t off = __builtin_amdgcn_readfirstlane(my_list[i]);  // byte offset of the record: slot * 16
                const char* base = reinterpret_cast<const char*>(s_rec) + off;
                const float4 g = *reinterpret_cast<const float4*>(base);
                const float4 h = *reinterpret_cast<const float4*>(base + SLOTS * 16);
                // one (pixel, splat) pair: k_blend's arithmetic (raster.hip blend_composite), FAST form
                const float p0 = fmaf(g.x, lx, fmaf(g.y, ly, g.z));
                const float p1 = fmaf(g.w, lx, fmaf(h.x, ly, h.y));
                const float a = fmaf(p0, p0, p1 * p1);
                float wgt = 0.0f;
                if (a <= tile::CUT_A2) {
#pragma clang fp contract(off)  // T <- T - w with the ROUNDED w = b T, the value that is summed (no fma(-b, T, T))
                    const float b = tile::opacity_at(a, h.w);
                    wgt = b * T;
                    T -= wgt;
                }
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
                // the quadrant is saturated: nothing behind can add more than T_MIN
                if ((i & 3u) == 3u && __ballot(T >= T_MIN) == 0ull) break;
            }
        }
        const int all_done = __syncthreads_and((WEIGHTED && idle) || T < T_MIN ? 1 : 0);  // (also: every wave's LDS atomics of this batch are done)
        // flush: one add + one max per (tile, entry) that drew anything, into the accumulators of its source Gaussian
        if (stager && (uint32_t)tid < nb) {
            const unsigned long long s = s_sum[tid];
            if (s != 0ull) {
                const uint32_t src = p.src_index[idx];
                atomicAdd(p.sum_q32 + src, s);
                atomicMax(p.max_bits + src, s_max[tid]);
            }
        }
        hi -= nb;
        // (no barrier here: every wave's walk is behind the vote, and a slot's partials are re-zeroed by the thread that flushed them)
        if (all_done) break;
    }
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
    const uint32_t grid = p.tiles_x * p.tiles_y;
    if (grid == 0) return WS_OK;
    const bool weighted = p.plane != nullptr;
#define WS_CONTRIB_LAUNCH(QW, QH)                                                                              \
    if (weighted) hipLaunchKernelGGL((k_contrib<QW, QH, true>), dim3(grid), dim3(64 * QW * QH), 0, stream, p); \
    else hipLaunchKernelGGL((k_contrib<QW, QH, false>), dim3(grid), dim3(64 * QW * QH), 0, stream, p)
    if (p.qw == 4 && p.qh == 4) { WS_CONTRIB_LAUNCH(4, 4); }
    else if (p.qw == 4 && p.qh == 2) { WS_CONTRIB_LAUNCH(4, 2); }
    else if (p.qw == 2 && p.qh == 2) { WS_CONTRIB_LAUNCH(2, 2); }
    else return fail(WS_ERR_UNSUPPORTED, "launch_contrib: tile shape");
#undef WS_CONTRIB_LAUNCH
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
