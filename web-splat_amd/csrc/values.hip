// values.hip -- a caller's per-Gaussian values drawn to pixel planes through a prepared frame's weights, and the id of the
// heaviest Gaussian per pixel (include/websplat.h, "Rendering per-Gaussian values").
//
//   k_values : one workgroup per blend tile, one wave per 8x8-pixel quadrant, the tile's binned list staged through LDS
//              near -> far by the calls k_contrib stages it with (blend_tile.h: batches, decode + quadrant masks, per-wave
//              compaction), plus one 16-B record of values (and the source index) per staged entry.  The walk is k_contrib's
//              to the token -- the same pairs, the same weights w = b T, the same stops -- and every lane keeps what k_contrib
//              reduces away: out(p) = sum of w * f[src], and the src of its largest w.  No atomics, no wave reductions.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "blend_tile.h"
#include "values.h"

namespace ws {

namespace {

constexpr uint32_t NO_WINNER = 0xFFFFFFFFu;

template <int QW, int QH, bool WINNER>
__global__ __launch_bounds__(64 * QW * QH) void k_values(const ValuesParams p) {
    using G = tile::Geometry<QW, QH>;
    constexpr int NW = G::NW, NT = G::NT, STAGE = G::STAGE, SLOTS = G::SLOTS, LCAP = G::LCAP, TW = G::TW, TH = G::TH;

    __shared__ float4 s_rec[2 * SLOTS];                                  // the two planes of 16-B records (blend_tile.h)
    __shared__ __attribute__((aligned(16))) uint16_t s_m[STAGE];        // quadrant masks, transposed per sub-round
    __shared__ __attribute__((aligned(16))) uint32_t s_list[NW][LCAP];  // per wave: byte offsets of the records that reach it
    __shared__ float4 s_val[SLOTS];                                      // per staged record: the values of its source Gaussian
    __shared__ uint32_t s_src[WINNER ? STAGE : 1];                       //   and its index in the point cloud

    // No blend need follow: the frame's error bits reach the renderer's sticky words from here too
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
    const uint32_t px = me.px(tx * TW), py = me.py(ty * TH);
    const bool inside = px < p.width && py < p.height;
    // pixels outside the viewport start with T = 0: every weight is 0 and they count as saturated
    float T = inside ? 1.0f : 0.0f;
    const float W = (float)p.width, H = (float)p.height;
    const float tile_x0 = (float)(tx * TW), tile_y0 = (float)(ty * TH);
    uint32_t* my_list = s_list[wave];
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
    float best_w = 0.0f;
    uint32_t best_id = NO_WINNER;

    uint32_t hi = range.y;  // (block-uniform: a tile with nothing listed only stores)
    while (hi > range.x) {
        const uint32_t nb = tile::batch_len<STAGE>(range.x, hi);
        if (stager) {
            uint32_t mask = 0u;
            const uint32_t idx = tile::entry_idx<STAGE>(p.entry_vals, range, hi, tid);
            if ((uint32_t)tid < nb) {
                mask = tile::stage_store<QW, QH, SLOTS>(s_rec, tid, tile::gather(p.splats, idx), W, H, tile_x0, tile_y0);
                const uint32_t src = p.src_index[idx];
                const float* f = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.values) + (size_t)src * p.stride);
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p.channels > 0u) v.x = f[0];
                if (p.channels > 1u) v.y = f[1];
                if (p.channels > 2u) v.z = f[2];
                if (p.channels > 3u) v.w = f[3];
                s_val[tid] = v;
                if constexpr (WINNER) s_src[tid] = src;
            }
            s_m[tile::mask_slot<LCAP>((uint32_t)tid, (uint32_t)lane)] = (uint16_t)mask;
        }
        __syncthreads();
        // a wave whose 64 pixels are saturated only keeps staging
        for (uint32_t sub = 0; sub < nb && __ballot(T >= T_MIN) != 0ull; sub += (uint32_t)LCAP) {
            // wave-private compaction: records whose kept ellipse reaches this quadrant, near -> far
            const uint32_t n = tile::compact<LCAP, true>(s_m, my_list, sub, nb, lane, me.bit, tile::list_value(sub + (uint32_t)lane));
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t off = __builtin_amdgcn_readfirstlane(my_list[i]);  // byte offset of the record: slot * 16
                const char* base = reinterpret_cast<const char*>(s_rec) + off;
                const float4 g = *reinterpret_cast<const float4*>(base);
                const float4 h = *reinterpret_cast<const float4*>(base + SLOTS * 16);
                // one (pixel, splat) pair: k_contrib's arithmetic (contrib.hip), which is k_blend's FAST form
                const float p0 = fmaf(g.x, lx, fmaf(g.y, ly, g.z));
                const float p1 = fmaf(g.w, lx, fmaf(h.x, ly, h.y));
                const float a = fmaf(p0, p0, p1 * p1);
                if (a <= tile::CUT_A2) {
                    float wgt;
                    {
#pragma clang fp contract(off)  // T <- T - w with the ROUNDED w = b T, the value that is drawn (no fma(-b, T, T))
                        const float b = tile::opacity_at(a, h.w);
                        wgt = b * T;
                        T -= wgt;
                    }
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
                // the quadrant is saturated: nothing behind can add more than T_MIN
                if ((i & 3u) == 3u && __ballot(T >= T_MIN) == 0ull) break;
            }
        }
        const int all_done = __syncthreads_and(T < T_MIN ? 1 : 0);  // (also: every wave's walk of this batch is behind it)
        hi -= nb;
        if (all_done) break;
    }

    if (inside) {
        const size_t x4 = (size_t)px * 4;
        if (p.plane[0]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[0]) + (size_t)py * p.pitch[0] + x4) = acc0;
        if (p.plane[1]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[1]) + (size_t)py * p.pitch[1] + x4) = acc1;
        if (p.plane[2]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[2]) + (size_t)py * p.pitch[2] + x4) = acc2;
        if (p.plane[3]) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane[3]) + (size_t)py * p.pitch[3] + x4) = acc3;
        if constexpr (WINNER) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(p.winner) + (size_t)py * p.winner_pitch + x4) = best_id;
    }
}

}  // namespace

int launch_values(const ValuesParams& p, hipStream_t stream) {
    const uint32_t grid = p.tiles_x * p.tiles_y;
    if (grid == 0) return WS_OK;
#define WS_VALUES_LAUNCH(QW, QH)                                                                                \
    if (p.winner) hipLaunchKernelGGL((k_values<QW, QH, true>), dim3(grid), dim3(64 * QW * QH), 0, stream, p); \
    else hipLaunchKernelGGL((k_values<QW, QH, false>), dim3(grid), dim3(64 * QW * QH), 0, stream, p)
    if (p.qw == 4 && p.qh == 4) { WS_VALUES_LAUNCH(4, 4); }
    else if (p.qw == 4 && p.qh == 2) { WS_VALUES_LAUNCH(4, 2); }
    else if (p.qw == 2 && p.qh == 2) { WS_VALUES_LAUNCH(2, 2); }
    else return fail(WS_ERR_UNSUPPORTED, "launch_values: tile shape");
#undef WS_VALUES_LAUNCH
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
