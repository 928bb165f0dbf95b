// blend_tile.h -- the staged-batch protocol of the compositing kernels, once: how a tile's binned list is cut into batches, where
// a staged record and its quadrant mask go in LDS, and how a wave reads the masks back into its near -> far list.  Owner of that
// layout for k_blend (raster.hip), k_contrib (contrib.hip) and k_blend2 (experimental/blend_async.hip); k_blend_strict, k_blend_q
// and k_blend_order take the range decode and the error fold from here.
//
//   layout layer : plain C++ (WS_HD of blend_stage.h) -- tests/test_blend_tile.py compiles it with g++ and walks it on the CPU
//   device layer : the same steps on pointers and values (no BlendParams / ContribParams), hipcc only
//
// A batch is the next (at most) STAGE entries from the near end of the tile's range [begin, end) of the entry list: slot 0 is the
// nearest.  Thread `slot` decodes its entry (blend_stage.h) into two planes of 16-B records, s_rec[slot] and s_rec[SLOTS + slot],
// and stores the record's 16-bit quadrant mask TRANSPOSED per sub-round of LCAP slots: the masks of slots lane, lane + 64, ... sit
// side by side, so a wave's compaction reads all of them with one or two wide LDS loads instead of one dependent load per 64
// records.  Each wave then lists the byte offsets (slot * 16) of the records that reach its quadrant, in slot order.
#pragma once

#include "blend_stage.h"

// entries staged per batch, at most (measured at 4x4: 256 -> blend +8 % on c2, +17 % on c3; 1024 does not leave LDS
// for two workgroups per CU)
#ifndef WS_BLEND_STAGE_MAX
#define WS_BLEND_STAGE_MAX 512
#endif

namespace ws {
namespace tile {

// ---- layout layer ----------------------------------------------------------------------------------------------------------
// One workgroup per tile of QW x QH quadrants of 8x8 pixels, one wave per quadrant.
// (a wave compacts and walks a staged batch in sub-rounds of at most LCAP records, so the lists stay small when the
// batch is large: -DWS_BLEND_STAGE_MAX=1024 halves the per-batch barriers and still leaves LDS for two workgroups)
template <int QW, int QH, int STAGE_MAX = WS_BLEND_STAGE_MAX>
struct Geometry {
    static constexpr int NW = QW * QH;  // waves = quadrants
    static constexpr int NT = 64 * NW;
    static constexpr int STAGE = NT < STAGE_MAX ? NT : STAGE_MAX;  // entries staged per batch
    static constexpr int SLOTS = STAGE + 1;                        // (slot STAGE: the null record that pads the lists)
    static constexpr int LCAP = STAGE < 512 ? STAGE : 512;
    static constexpr int TW = 8 * QW, TH = 8 * QH;
    static_assert(LCAP % 256 == 0, "sub-round layout of the quadrant masks: four 16-bit masks per 64-bit piece");
    static_assert(STAGE % LCAP == 0, "a batch is a whole number of sub-rounds");
};

// where the mask of slot `slot` is stored (index into the uint16_t plane).  (A kernel that already holds lane = slot & 63 passes
// it: lane * (LCAP / 64) is also the compaction's read base, and the compiler shares the two only when it sees the same value.)
template <int LCAP>
WS_HD constexpr uint32_t mask_slot(uint32_t slot, uint32_t lane) {
    return (slot / LCAP) * LCAP + lane * (LCAP / 64) + ((slot % LCAP) >> 6);
}
template <int LCAP>
WS_HD constexpr uint32_t mask_slot(uint32_t slot) { return mask_slot<LCAP>(slot, slot & 63u); }
// ... and how the compaction of the sub-round that starts at slot `sub` reads them back: lane `lane` owns the LCAP / 64 adjacent
// masks from mask_read_base, in 64-bit pieces h of four quarters q; quarter q of piece h is the mask of slot compact_slot, and
// what the list holds for a slot is the byte offset of its record.  Quarters in order, lanes in order within a quarter = slot order.
template <int LCAP>
WS_HD constexpr uint32_t mask_read_base(uint32_t sub, uint32_t lane) { return sub + lane * (LCAP / 64); }
WS_HD constexpr uint32_t compact_slot(uint32_t sub, uint32_t lane, int h, int q) { return sub + lane + (uint32_t)(h * 4 + q) * 64u; }
WS_HD constexpr uint32_t list_value(uint32_t slot) { return slot * 16u; }
// (WS_BLEND_COMPACT_SKIP) a batch with at most h * 256 entries left in the sub-round has nothing in piece h: slots past nb hold 0
WS_HD constexpr bool piece_empty(uint32_t nb, uint32_t sub, int h) { return h > 0 && nb - sub <= (uint32_t)(h * 256); }

// entries of the batch that ends at `hi` in the list [begin, ...)
template <int STAGE>
WS_HD constexpr uint32_t batch_len(uint32_t begin, uint32_t hi) { return (hi - begin) < (uint32_t)STAGE ? (hi - begin) : (uint32_t)STAGE; }
// position in the entry list of slot `tid` of that batch (slot 0 = nearest).  Clamped into the tile's (non-empty) range, also for
// tid >= nb and for hi == begin: the load never depends on a branch and can be issued batches ahead.
template <int STAGE>
WS_HD constexpr uint32_t entry_pos(uint32_t begin, uint32_t hi, uint32_t tid) {
    const uint32_t h = hi > begin ? hi : begin + 1u;
    const uint32_t nb = batch_len<STAGE>(begin, h);
    const uint32_t off = tid < nb ? tid : nb - 1u;
    return h - 1u - off;
}

// tile_ranges holds (0xFFFFFFFF - begin, end) per binned list, (0, 0) = empty: begin of [begin, end)
WS_HD constexpr uint32_t range_begin(uint32_t x, uint32_t y) { return y ? 0xFFFFFFFFu - x : 0u; }
// Index of the binned list blend tile (tx, ty) composites: its own, the binning tile's it is a half of (split mode:
// range_row_shift 1), or -- when the frame binned at twice the blend's tile size (bin_shift 1) -- the 2 x 2 block's it belongs to.
WS_HD constexpr uint32_t list_index(uint32_t tx, uint32_t ty, uint32_t bin_shift, uint32_t bin_tiles_x, uint32_t range_row_shift) {
    const uint32_t btx = bin_shift ? (bin_tiles_x + 1u) >> 1 : bin_tiles_x;
    return ((ty >> range_row_shift) >> bin_shift) * btx + (tx >> bin_shift);
}

}  // namespace tile
}  // namespace ws

// ---- device layer ----------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "ws_internal.h"

namespace ws {
namespace tile {

constexpr float CUT_A2 = CUT_A * stage::LOG2E_F;  // gaussian.wgsl:61 cut-off, in the exp2 domain

// The last kernel of a frame folds the frame's error bits (per-frame zero arena) into the renderer's sticky words, which no
// per-frame memset clears: [0] the bits, [1] the largest entry demand of an overflowed frame.  The demand is ALSO posted --
// a plain system-scope store by this one thread -- to a host-visible mailbox word (pinned, mapped memory) that the next
// prepare() reads without any device synchronisation: a renderer whose frames overflow its entry list grows the list by
// itself, whether or not its caller ever polls ws_renderer_errors.
__device__ __forceinline__ void fold_frame_errors(const FrameCounters* counters, uint32_t* sticky, uint32_t* demand_mailbox) {
    const uint32_t bits = counters->overflow;
    if (!bits) return;
    atomicOr(sticky, bits);
    if (bits & 1u) {
        const uint32_t need = counters->entries_needed;
        const uint32_t before = atomicMax(sticky + 1, need);  // what a retry (or the next prepare) allocates
        if (demand_mailbox) __hip_atomic_store(demand_mailbox, need > before ? need : before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// This lane's place in a tile of QW quadrants per row: wave = quadrant (wave-uniform: lives in an SGPR), lane = pixel.
struct Quadrant {
    int wave, lane, qx, qy;
    float lx, ly;   // tile-local pixel centre
    uint32_t bit;   // this quadrant's bit of a record's mask
    __device__ __forceinline__ uint32_t px(uint32_t tile_px0) const { return tile_px0 + qx * 8 + (lane & 7); }
    __device__ __forceinline__ uint32_t py(uint32_t tile_py0) const { return tile_py0 + qy * 8 + (lane >> 3); }
};
template <int QW>
__device__ __forceinline__ Quadrant quadrant(int tid) {
    Quadrant q;
    q.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    q.lane = tid & 63;
    q.qx = q.wave % QW;
    q.qy = q.wave / QW;
    q.lx = (float)(q.qx * 8 + (q.lane & 7)) + 0.5f;
    q.ly = (float)(q.qy * 8 + (q.lane >> 3)) + 0.5f;
    q.bit = 1u << q.wave;
    return q;
}

// raw words of one staged entry: the 20-B Splat record (pointcloud.rs:352-358)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
struct RawSplat {
    u32x4_t a;    // words 0..3: kept as ONE 128-bit value from the load to the decode (see gather)
    uint32_t w4;
};
// The Splat index of slot `tid` of the batch that ends at `hi`
template <int STAGE>
__device__ __forceinline__ uint32_t entry_idx(const uint32_t* entry_vals, uint2 range, uint32_t hi, int tid) {
    return entry_vals[entry_pos<STAGE>(range.x, hi, (uint32_t)tid)];
}
// The 20-B Splat record.  One dwordx4 + one dword, and the four words stay a single 128-bit value until the decode: as
// five scalars the compiler parked three of them in other registers right behind the load (s_waitcnt vmcnt + v_mov: the
// gather of the next batch never overlapped the walk of the current one); five separate dword loads fix that too but cost
// 2.5x the address lookups of a random gather (measured: blend +35 % on hd1m, +29 % on c3).
__device__ __forceinline__ RawSplat gather(const uint8_t* splats, uint32_t idx) {
    const char* sp = reinterpret_cast<const char*>(splats) + (size_t)idx * SPLAT_STRIDE;
    RawSplat r;
    __builtin_memcpy(&r.a, sp, 16);
    __builtin_memcpy(&r.w4, sp + 16, 4);
    return r;
}

// Decode `raw` for the tile whose top-left pixel is (tile_x0, tile_y0) into slot `tid` of the two planes; returns its quadrant
// mask.  The colour and opacity stay the f16 pairs of the Splat record (words 3 and 4, copied verbatim).
template <int QW, int QH, int SLOTS>
__device__ __forceinline__ uint32_t stage_store(float4* s_rec, int tid, const RawSplat& raw, float W, float H, float tile_x0, float tile_y0) {
    const stage::Staged s = stage::decode<QW, QH>(raw.a.x, raw.a.y, raw.a.z, raw.a.w, raw.w4, W, H, tile_x0, tile_y0, CUT_A2);
    s_rec[tid] = make_float4(s.i00, s.i01, s.c0, s.i10);
    s_rec[SLOTS + tid] = make_float4(s.i11, s.c1, __uint_as_float(raw.a.w), __uint_as_float(raw.w4));
    return s.mask;
}
// Wave-private compaction of the sub-round at `sub` of a batch of nb entries: the records whose kept ellipse reaches this wave's
// quadrant, near -> far, as slot16 + list_value(slot - sub - lane) -- slot16 is the caller's value for the lane's round-0 slot,
// list_value(sub + lane) plus whatever constant its walk wants folded in.  Returns the list's length.
template <int LCAP, bool SKIP>
__device__ __forceinline__ uint32_t compact(const uint16_t* s_m, uint32_t* my_list, uint32_t sub, uint32_t nb, int lane, uint32_t qbit,
                                            uint32_t slot16) {
    const uint2* mp = reinterpret_cast<const uint2*>(s_m + mask_read_base<LCAP>(sub, (uint32_t)lane));
    uint32_t n = 0;
#pragma unroll
    for (int h = 0; h < LCAP / 256; ++h) {
        // (a batch of at most 256 entries -- the median hd1m tile stages 197 -- has nothing in its upper slots: a scalar branch
        //  saves their mask load and four ballots)
        if (SKIP && piece_empty(nb, sub, h)) break;
        const uint2 mm = mp[h];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t word = (q & 2) ? mm.y : mm.x;
            const bool t = (word & (qbit << ((q & 1) * 16))) != 0u;
            const unsigned long long bal = __ballot(t);
            const uint32_t pos = n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (t) my_list[pos] = slot16 + list_value(compact_slot(0u, 0u, h, q));
            n += (uint32_t)__popcll(bal);
        }
    }
    return n;
}

// b = min(0.99, 2^-a' * alpha), alpha = high half of w4 (f16).  One asm block: gfx950 needs one wait state between
// a transcendental's result and a VALU instruction reading it, and the compiler does not look inside asm.
__device__ __forceinline__ float opacity_at(float a, float w4) {
    float b;
    asm("v_exp_f32_e64 %0, -%1\n\ts_nop 0\n\t"
        "v_fma_mix_f32 %0, %0, %2, 0 op_sel:[0,1,0] op_sel_hi:[0,1,0]\n\t"
        "v_min_f32_e32 %0, 0x3f7d70a4, %0"
        : "=&v"(b)
        : "v"(a), "v"(w4));
    return b;
}


}  // namespace tile
}  // namespace ws
#endif  // __HIPCC__
