// contrib.hip -- what each Gaussian of the resident scene did to a prepared frame (include/websplat.h, "Per-Gaussian
// contributions"), and the device gather of ws_pointcloud_create_subset.
//
//   k_contrib       : one workgroup per blend tile, one wave per 8x8-pixel quadrant, the tile's binned list staged through
//                     LDS near -> far exactly as k_blend stages it (blend_stage.h decode + quadrant masks, per-wave
//                     compaction).  No pixel is written: per staged record every lane converts its weight w = b T to
//                     q32 = (uint32_t)(w 2^32), the wave reduces sum and max as INTEGERS (DPP), the tile's waves meet in LDS
//                     (one ds_add_u64 + one ds_max_u32 per (wave, record)), and after the batch's walk the staging threads
//                     flush: one 64-bit add and one 32-bit max per (tile, entry) with a non-zero sum, through K1's
//                     src_index, into the accumulators.  Integer sums and maxima commute: the result does not depend on
//                     the order of anything.
//   k_contrib_merge : accumulator += host arrays of another accumulator (ws_contrib_add)
//   k_pc_gather     : the kept Gaussians' records, plane by plane
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "blend_stage.h"
#include "contrib.h"

namespace ws {

namespace {

constexpr float CUT_A2 = CUT_A * stage::LOG2E_F;  // gaussian.wgsl:61 cut-off, in the exp2 domain (raster.hip)
constexpr int CONTRIB_STAGE_MAX = 512;            // entries staged per batch, at most (k_blend's WS_BLEND_STAGE_MAX)

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

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

// the entry of slot `tid` of the batch that ends at `hi` (slot 0 = nearest), address clamped into the tile's non-empty range
template <int STAGE>
__device__ __forceinline__ uint32_t contrib_entry_idx(const ContribParams& p, uint2 range, uint32_t hi, int tid) {
    const uint32_t h = hi > range.x ? hi : range.x + 1u;
    const uint32_t nb = (h - range.x) < (uint32_t)STAGE ? (h - range.x) : (uint32_t)STAGE;
    const uint32_t off = (uint32_t)tid < nb ? (uint32_t)tid : nb - 1u;
    return p.entry_vals[h - 1u - off];
}

template <int QW, int QH>
__global__ __launch_bounds__(64 * QW * QH) void k_contrib(const ContribParams p) {
    constexpr int NW = QW * QH;
    constexpr int NT = 64 * NW;
    constexpr int STAGE = NT < CONTRIB_STAGE_MAX ? NT : CONTRIB_STAGE_MAX;
    constexpr int SLOTS = STAGE + 1;
    constexpr int TW = 8 * QW, TH = 8 * QH;
    constexpr int LCAP = STAGE < 512 ? STAGE : 512;
    static_assert(LCAP % 256 == 0 && STAGE % LCAP == 0, "sub-round layout of the quadrant masks");

    __shared__ float4 s_rec[2 * SLOTS];                                  // k_blend's two planes of 16-B records
    __shared__ __attribute__((aligned(16))) uint16_t s_m[STAGE];        // quadrant masks, transposed per sub-round (k_blend)
    __shared__ __attribute__((aligned(16))) uint32_t s_list[NW][LCAP];  // per wave: byte offsets of the records that reach it
    __shared__ unsigned long long s_sum[STAGE];                          // per staged record: sum of q32 over the tile's pixels
    __shared__ uint32_t s_max[STAGE];                                    //   and the bits of its largest weight

    // No blend need follow (ws_scene_accumulate_contrib): the frame's error bits reach the renderer's sticky words from here too
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.sticky) {
        const uint32_t bits = p.counters->overflow;
        if (bits) {
            atomicOr(p.sticky, bits);
            if (bits & 1u) {
                const uint32_t need = p.counters->entries_needed;
                const uint32_t before = atomicMax(p.sticky + 1, need);
                if (p.demand_mailbox) __hip_atomic_store(p.demand_mailbox, need > before ? need : before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    const uint32_t tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;  // (the grid is tiles_x * tiles_y)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int qx = wave % QW, qy = wave / QW;
    const float lx = (float)(qx * 8 + (lane & 7)) + 0.5f;  // tile-local pixel centre
    const float ly = (float)(qy * 8 + (lane >> 3)) + 0.5f;
    const uint32_t qbit = 1u << wave;
    const bool stager = NT == STAGE || tid < STAGE;  // wave-uniform
    // the binned list of this tile: its own, or -- the frame binned at twice the blend's tile size -- its 2 x 2 block's
    uint2 range;
    {
        const uint32_t s = p.counters->bin_shift;
        const uint32_t btx = s ? (p.tiles_x + 1u) >> 1 : p.tiles_x;
        range = p.tile_ranges[(ty >> s) * btx + (tx >> s)];
        range.x = range.y ? 0xFFFFFFFFu - range.x : 0u;
    }
    if (range.y <= range.x) return;  // block-uniform: nothing listed
    const uint32_t px = tx * TW + qx * 8 + (lane & 7);
    const uint32_t py = ty * TH + qy * 8 + (lane >> 3);
    // pixels outside the viewport start with T = 0: every weight is 0 and they count as saturated
    float T = (px < p.width && py < p.height) ? 1.0f : 0.0f;
    const float W = (float)p.width, H = (float)p.height;
    const float tile_x0 = (float)(tx * TW), tile_y0 = (float)(ty * TH);
    uint32_t* my_list = s_list[wave];

    uint32_t hi = range.y;
    while (hi > range.x) {
        const uint32_t nb = (hi - range.x) < (uint32_t)STAGE ? (hi - range.x) : (uint32_t)STAGE;
        uint32_t idx = 0u;
        if (stager) {
            uint32_t mask = 0u;
            idx = contrib_entry_idx<STAGE>(p, range, hi, tid);
            if ((uint32_t)tid < nb) {
                const char* sp = reinterpret_cast<const char*>(p.splats) + (size_t)idx * SPLAT_STRIDE;
                u32x4_t a;
                uint32_t w4;
                __builtin_memcpy(&a, sp, 16);
                __builtin_memcpy(&w4, sp + 16, 4);
                const stage::Staged s = stage::decode<QW, QH>(a.x, a.y, a.z, a.w, w4, W, H, tile_x0, tile_y0, CUT_A2);
                mask = s.mask;
                s_rec[tid] = make_float4(s.i00, s.i01, s.c0, s.i10);
                s_rec[SLOTS + tid] = make_float4(s.i11, s.c1, __uint_as_float(a.w), __uint_as_float(w4));
            }
            s_m[((uint32_t)tid / LCAP) * LCAP + ((uint32_t)tid & 63u) * (LCAP / 64) + (((uint32_t)tid % LCAP) >> 6)] = (uint16_t)mask;
            s_sum[tid] = 0ull;
            s_max[tid] = 0u;
        }
        __syncthreads();
        // a wave whose 64 pixels are saturated only keeps staging
        for (uint32_t sub = 0; sub < nb && __ballot(T >= T_MIN) != 0ull; sub += (uint32_t)LCAP) {
            // wave-private compaction: records whose kept ellipse reaches this quadrant, near -> far (k_blend's)
            const uint2* mp = reinterpret_cast<const uint2*>(s_m + sub + (uint32_t)lane * (LCAP / 64));
            uint32_t n = 0;
            const uint32_t slot16 = (sub + (uint32_t)lane) * 16u;
#pragma unroll
            for (int h = 0; h < LCAP / 256; ++h) {
                if (h > 0 && nb - sub <= (uint32_t)(h * 256)) break;
                const uint2 mm = mp[h];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = h * 4 + q;
                    const uint32_t word = (q & 2) ? mm.y : mm.x;
                    const bool t = (word & (qbit << ((q & 1) * 16))) != 0u;
                    const unsigned long long bal = __ballot(t);
                    const uint32_t pos = n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    if (t) my_list[pos] = slot16 + (uint32_t)r * 1024u;
                    n += (uint32_t)__popcll(bal);
                }
            }
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
                if (a <= CUT_A2) {
#pragma clang fp contract(off)  // T <- T - w with the ROUNDED w = b T, the value that is summed (no fma(-b, T, T))
                    float b;
                    asm("v_exp_f32_e64 %0, -%1\n\ts_nop 0\n\t"
                        "v_fma_mix_f32 %0, %0, %2, 0 op_sel:[0,1,0] op_sel_hi:[0,1,0]\n\t"
                        "v_min_f32_e32 %0, 0x3f7d70a4, %0"
                        : "=&v"(b)
                        : "v"(a), "v"(h.w));
                    wgt = b * T;
                    T -= wgt;
                }
                // w < 1: w * 2^32 is exact in f32 and below 2^32; the conversion truncates (and takes anything negative to 0).
                // A pair whose weight truncates to 0 (w < 2^-32) counts in neither result: sum == 0 <=> max == 0.
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
        const int all_done = __syncthreads_and(T < T_MIN ? 1 : 0);  // (also: every wave's LDS atomics of this batch are done)
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
    if (p.qw == 4 && p.qh == 4) hipLaunchKernelGGL((k_contrib<4, 4>), dim3(grid), dim3(1024), 0, stream, p);
    else if (p.qw == 4 && p.qh == 2) hipLaunchKernelGGL((k_contrib<4, 2>), dim3(grid), dim3(512), 0, stream, p);
    else if (p.qw == 2 && p.qh == 2) hipLaunchKernelGGL((k_contrib<2, 2>), dim3(grid), dim3(256), 0, stream, p);
    else return fail(WS_ERR_UNSUPPORTED, "launch_contrib: tile shape");
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
