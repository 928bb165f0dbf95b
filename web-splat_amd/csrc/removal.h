// removal.h -- what deleting each Gaussian alone would do to a prepared frame (removal.hip k_removal_base, k_removal).  Internal:
// the ABI is include/websplat.h, "Removal effect"; DESIGN.md 3.4h.
#pragma once

#include <cstddef>

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
    unsigned long long* sum_q32;  // [num_points]
    uint32_t* max_bits;           // [num_points] bits of the largest v
    const float* plane;           // the weight plane, f32 per viewport pixel; nullptr: E = 1, and nothing below is read
    size_t plane_pitch;           // bytes
    float plane_scale, plane_bias;
};
static_assert(offsetof(RemovalParams, base) == 80, "the frame's lists first, as in ContribParams and ValuesParams");

// k_removal_base<qw, qh>, then k_removal<qw, qh, plane != nullptr, kind> on the same stream.
//
// TO THE BIT.  The pairs, the weights wgt = b * T and the stops are tile::walk_weights' (weight_walk.h), the one function k_contrib
// and k_values run: nothing here influences them.  The staging thread of a slot also copies words 3 and 4 of its Splat record
// (the f16 colour and opacity) into a third plane of 8-B records; c_ch below is that f16 colour taken to f32.
//
// Pass 1 (every viewport pixel, empty tiles included).  acc_ch = 0, T = 1; per kept pair, near -> far:
//   acc_ch = fmaf(wgt, c_ch, acc_ch);  T = T - wgt                     (the walk's own subtraction of its rounded wgt)
// and at the end base(p) = (fmaf(T, background_ch, acc_ch), T): (background, 1) where nothing is listed.
//
// Pass 2.  Every lane inside the viewport loads base(p) = (F, .) and, with a plane, E(p) exactly as k_contrib's weighted form
// does (contrib.h); P_ch = 0, T = 1 (0 outside the viewport).  Per walked pair:
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
//   q32 = (uint32_t)(v * 2^32)  exact product, truncating;  mb = q32 ? bits(v) : 0
// and q32 / mb go the way k_contrib's go: DPP wave reductions, LDS partials per staged record, one 64-bit add and one 32-bit max
// per (tile, entry) with a non-zero sum, through src_index.  A wave whose 64 values of E are all 0 skips its walk (as in
// k_contrib); pass 1 never does.
int launch_removal(const RemovalParams& p, hipStream_t stream);

}  // namespace ws
