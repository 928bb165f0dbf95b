// removal.h -- what deleting each Gaussian alone would do to a prepared frame (removal.hip k_removal_base, k_removal).  Internal:
// the ABI is include/websplat.h, "Removal effect"; DESIGN.md 3.4h.
#pragma once

#include <cstddef>

#include "accum_q32.h"
#include "weight_walk.h"

namespace ws {

// Two launches over a prepared frame's binned, depth-ordered tile lists, both sinks of tile::walk_weights: siblings of k_contrib
// and k_values, one workgroup per blend tile (qw x qh quadrants, one wave each).
struct RemovalParams {
    FrameLists frame;             // (its counters' error bits are folded into *sticky: no blend need follow)
    float4* base;                 // pass 1 writes, pass 2 reads: (F_r, F_g, F_b, T_end) per viewport pixel
    size_t base_pitch;            // bytes, a multiple of 16
    float background[3];
    float scale;                  // of the effect: v = min(scale * m, 1 - 2^-24)
    int kind;                     // WS_ERROR_SQ | WS_ERROR_ABS
    Accum acc;                    // acc.plane: the weight plane; nullptr: every pair counts in full
};
static_assert(offsetof(RemovalParams, base) == 80, "the frame's lists first, as in ContribParams and ValuesParams");
static_assert(offsetof(RemovalParams, acc) == 120 && sizeof(RemovalParams) == 160, "kernarg segment of k_removal: 416 B");

// k_removal_base<qw, qh>, then k_removal<qw, qh, acc.plane != nullptr, kind> on the same stream.
//
// TO THE BIT.  The pairs, the weights wgt = b * T and the stops are tile::walk_weights' (weight_walk.h), the one function k_contrib
// and k_values run: nothing here influences them.  The staging thread of a slot also copies words 3 and 4 of its Splat record
// (the f16 colour and opacity) into a third plane of 8-B records; c_ch below is that f16 colour taken to f32.
//
// Pass 1 (every viewport pixel, empty tiles included).  acc_ch = 0, T = 1; per kept pair, near -> far:
//   acc_ch = fmaf(wgt, c_ch, acc_ch);  T = T - wgt                     (the walk's own subtraction of its rounded wgt)
// and at the end base(p) = (fmaf(T, background_ch, acc_ch), T): (background, 1) where nothing is listed.
//
// Pass 2.  Every lane inside the viewport loads base(p) = (F, .) and, with a plane, the accumulator's E(p) (accum_q32.h);
// P_ch = 0, T = 1 (0 outside the viewport).  Per walked pair:
//   Tb = T;  T = Tb - wgt                                              (wgt == 0 for a pair outside the cut-off)
//   kept:  P_ch = fmaf(wgt, c_ch, P_ch)
//   counted = kept && wgt > 0 && Tb >= 2^-14;  not counted: v = 0
//   r    = wgt / T                                                     IEEE division
//   s_ch = F_ch - P_ch                                                 one rounded subtraction
//   t_ch = wgt * c_ch                                                  one rounded multiply
//   d_ch = fmaf(r, s_ch, -t_ch)                                        one fused multiply-add
//   e_ch = d_ch * d_ch (SQ) | fabsf(d_ch) (ABS)                        one rounded multiply
//   m    = ((e_r + e_g) + e_b) / 3.0f                                  two rounded additions, IEEE division
//   v    = fminf(scale * m, 0x1.fffffep-1f), NaN -> 0                  one rounded multiply
//   plane:  v = v * E                                                  one rounded multiply
// and everything from v on is the accumulator's (accum_q32.h), the one k_contrib feeds too.  A wave whose 64 values of E are
// all 0 skips its walk there; pass 1 never does.
int launch_removal(const RemovalParams& p, hipStream_t stream);

// Pass 1 alone: k_removal_base<qw, qh>.  Reads frame, base, base_pitch and background of p and nothing else -- the launch the
// gradient's pass 1 makes too (gradient.h).
int launch_removal_base(const RemovalParams& p, hipStream_t stream);

}  // namespace ws

#if defined(__HIPCC__)
namespace ws {

// The staged colours of k_removal_base, k_removal and k_gradient (gradient.hip).
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

}  // namespace ws
#endif  // __HIPCC__
