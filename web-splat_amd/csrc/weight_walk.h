// weight_walk.h -- the weights of a prepared frame, w = b T pair by pair, near -> far, once: what a launch over the frame's binned
// lists reads (FrameLists) and the walk of one tile's list through the staged batches of blend_tile.h (tile::walk_weights).
// k_contrib (contrib.hip), k_values (values.hip), k_removal_base and k_removal (removal.hip) are four sinks of this one function:
// in one context they see the same pairs, the same weights and the same stops because there is no second copy of the arithmetic.
// What k_contrib and k_removal do with a value per pair is accum_q32.h's.  k_blend (raster.hip) keeps its own walk.
#pragma once

#include <type_traits>

#include "ws_internal.h"

namespace ws {

// A prepared frame's binned, depth-ordered tile lists, as a kernel argument.  ContribParams, ValuesParams and RemovalParams start with it.
struct FrameLists {
    const uint8_t* splats;        // [V] x SPLAT_STRIDE
    const uint32_t* entry_vals;   // sorted by tile, far -> near inside a tile (store indices)
    const uint2* tile_ranges;     // (0xFFFFFFFF - begin, end) per binning tile, (0, 0) = empty
    const uint32_t* src_index;    // [V] store slot -> index into the point cloud (K1, contributions enabled)
    uint32_t width, height, tiles_x, tiles_y;
    uint32_t qw, qh;
    const FrameCounters* counters;  // bin_shift of the frame; its error bits are folded into *sticky (no blend need follow)
    uint32_t* sticky;
    uint32_t* demand_mailbox;
};
static_assert(sizeof(FrameLists) == 80, "the kernels read their own arguments at the offsets they always had");

// f(std::integral_constant<int, QW>, std::integral_constant<int, QH>) for the tile shapes the walk is built for; false: none of them
template <class F>
inline bool with_tile_shape(uint32_t qw, uint32_t qh, F&& f) {
    if (qw == 4 && qh == 4) f(std::integral_constant<int, 4>(), std::integral_constant<int, 4>());
    else if (qw == 4 && qh == 2) f(std::integral_constant<int, 4>(), std::integral_constant<int, 2>());
    else if (qw == 2 && qh == 2) f(std::integral_constant<int, 2>(), std::integral_constant<int, 2>());
    else return false;
    return true;
}

}  // namespace ws

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>

#include "blend_tile.h"

namespace ws {
namespace tile {

// One workgroup per blend tile, one wave per 8x8-pixel quadrant: the tile's list staged near -> far in batches, every wave
// compacting and walking the records that reach its quadrant.  Per (pixel, record) pair, k_blend's FAST arithmetic:
//   p0, p1, a;  kept = a <= CUT_A2;  kept: b = opacity_at(a), wgt = b * T (rounded), T <- T - wgt;  else wgt = 0
// A wave stops walking a batch once its 64 pixels are below T_MIN (looked at after every fourth record of its list); the batch
// loop ends when every wave is there.  Pixels outside the viewport start with T = 0.
//
// Sink (all hooks __device__ __forceinline__):
//   static constexpr bool WRITES_EMPTY_TILES   false: a tile with nothing listed returns before any other load
//   begin(px, py, inside)        once, before the first batch
//   idle()                       wave-uniform: this wave has nothing to add whatever it walks; it keeps staging and votes "done"
//   stage(tid, idx, live)        every staging thread, once per batch, before the barrier; live: slot tid holds entry idx
//   static constexpr bool PAIR_IS_WAVE_WIDE    true: pair() holds wave-wide operations and is called by ALL lanes for every walked
//                                record, with wgt = 0 and kept = false where the pair is outside the cut-off; false: only the
//                                lanes of kept pairs call it, inside the branch that made wgt
//   pair(off, wgt, kept)         one (pixel, record) pair; off = slot * 16
//   static constexpr bool WANTS_COORDS         optional; true: the call is pair(off, wgt, kept, p0, p1) with the walk's own p0, p1
//                                (a' = p0^2 + p1^2, formed for every walked pair, kept or not).  A sink without the member is
//                                called as before: the choice is made at compile time and leaves no trace in its code
//   flush(tid, idx)              live staging threads, behind the batch's vote (every wave's pair() calls of the batch are done)
//   finish(px, py, inside)       once, behind the last batch
template <class Sink, class = void>
struct wants_coords : std::false_type {};
template <class Sink>
struct wants_coords<Sink, std::void_t<decltype(Sink::WANTS_COORDS)>> : std::integral_constant<bool, Sink::WANTS_COORDS> {};

template <int QW, int QH, class Sink>
__device__ __forceinline__ void walk_weights(const FrameLists& p, Sink& sink) {
    using G = Geometry<QW, QH>;
    constexpr int NW = G::NW, NT = G::NT, STAGE = G::STAGE, SLOTS = G::SLOTS, LCAP = G::LCAP, TW = G::TW, TH = G::TH;

    __shared__ float4 s_rec[2 * SLOTS];                                  // the two planes of 16-B records (blend_tile.h)
    __shared__ __attribute__((aligned(16))) uint16_t s_m[STAGE];        // quadrant masks, transposed per sub-round
    __shared__ __attribute__((aligned(16))) uint32_t s_list[NW][LCAP];  // per wave: byte offsets of the records that reach it

    // No blend need follow: the frame's error bits reach the renderer's sticky words from here too
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.sticky) fold_frame_errors(p.counters, p.sticky, p.demand_mailbox);
    const uint32_t tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;  // (the grid is tiles_x * tiles_y)
    const int tid = threadIdx.x;
    const Quadrant me = quadrant<QW>(tid);
    const int wave = me.wave, lane = me.lane;
    const float lx = me.lx, ly = me.ly;
    const bool stager = NT == STAGE || tid < STAGE;  // wave-uniform
    // the binned list of this tile: its own, or -- the frame binned at twice the blend's tile size -- its 2 x 2 block's
    uint2 range = p.tile_ranges[list_index(tx, ty, p.counters->bin_shift, p.tiles_x, 0u)];
    range.x = range_begin(range.x, range.y);
    if (!Sink::WRITES_EMPTY_TILES && range.y <= range.x) return;  // block-uniform: nothing listed
    const uint32_t px = me.px(tx * TW), py = me.py(ty * TH);
    const bool inside = px < p.width && py < p.height;
    // pixels outside the viewport start with T = 0: every weight is 0 and they count as saturated
    float T = inside ? 1.0f : 0.0f;
    const float W = (float)p.width, H = (float)p.height;
    const float tile_x0 = (float)(tx * TW), tile_y0 = (float)(ty * TH);
    uint32_t* my_list = s_list[wave];
    sink.begin(px, py, inside);

    uint32_t hi = range.y;
    while (hi > range.x) {
        const uint32_t nb = batch_len<STAGE>(range.x, hi);
        uint32_t idx = 0u;
        if (stager) {
            uint32_t mask = 0u;
            idx = entry_idx<STAGE>(p.entry_vals, range, hi, tid);
            const bool live = (uint32_t)tid < nb;
            if (live) mask = stage_store<QW, QH, SLOTS>(s_rec, tid, gather(p.splats, idx), W, H, tile_x0, tile_y0);
            sink.stage(tid, idx, live);
            s_m[mask_slot<LCAP>((uint32_t)tid, (uint32_t)lane)] = (uint16_t)mask;
        }
        __syncthreads();
        // a wave whose 64 pixels are saturated only keeps staging
        for (uint32_t sub = 0; sub < nb && !sink.idle() && __ballot(T >= T_MIN) != 0ull; sub += (uint32_t)LCAP) {
            // wave-private compaction: records whose kept ellipse reaches this quadrant, near -> far
            const uint32_t n = compact<LCAP, true>(s_m, my_list, sub, nb, lane, me.bit, list_value(sub + (uint32_t)lane));
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t off = __builtin_amdgcn_readfirstlane(my_list[i]);  // byte offset of the record: slot * 16
                const char* base = reinterpret_cast<const char*>(s_rec) + off;
                const float4 g = *reinterpret_cast<const float4*>(base);
                const float4 h = *reinterpret_cast<const float4*>(base + SLOTS * 16);
                // one (pixel, splat) pair: k_blend's arithmetic (raster.hip blend_composite), FAST form
                const float p0 = fmaf(g.x, lx, fmaf(g.y, ly, g.z));
                const float p1 = fmaf(g.w, lx, fmaf(h.x, ly, h.y));
                const float a = fmaf(p0, p0, p1 * p1);
                const bool kept = a <= CUT_A2;
                float wgt = 0.0f;
                if (kept) {
#pragma clang fp contract(off)  // T <- T - w with the ROUNDED w = b T, the value the sink gets (no fma(-b, T, T))
                    const float b = opacity_at(a, h.w);
                    wgt = b * T;
                    T -= wgt;
                    // (inside the branch the sink's LDS reads issue beside the exp; behind it they wait for the branch to rejoin)
                    if constexpr (!Sink::PAIR_IS_WAVE_WIDE) {
                        if constexpr (wants_coords<Sink>::value) sink.pair(off, wgt, true, p0, p1);
                        else sink.pair(off, wgt, true);
                    }
                }
                if constexpr (Sink::PAIR_IS_WAVE_WIDE) {
                    if constexpr (wants_coords<Sink>::value) sink.pair(off, wgt, kept, p0, p1);
                    else sink.pair(off, wgt, kept);
                }
                // the quadrant is saturated: nothing behind can add more than T_MIN
                if ((i & 3u) == 3u && __ballot(T >= T_MIN) == 0ull) break;
            }
        }
        const int all_done = __syncthreads_and(sink.idle() || T < T_MIN ? 1 : 0);  // (also: every wave's walk of this batch is behind it)
        if (stager && (uint32_t)tid < nb) sink.flush(tid, idx);
        hi -= nb;
        // (no barrier here: every wave's walk is behind the vote, and what flush read of a slot is rewritten by the same thread's stage)
        if (all_done) break;
    }
    sink.finish(px, py, inside);
}

}  // namespace tile
}  // namespace ws
#endif  // __HIPCC__
