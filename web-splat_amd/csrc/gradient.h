// gradient.h -- the colour and ln-opacity gradients of an image loss, per Gaussian, over a prepared frame (gradient.hip
// k_gradient; pass 1 is removal.hip's k_removal_base).  Internal: the ABI is include/websplat.h, "Gradients of an image loss";
// DESIGN.md 3.4i.
#pragma once

#include <cstddef>

#include "accum_s32.h"
#include "removal.h"

namespace ws {

// One launch over a prepared frame's binned, depth-ordered tile lists: the fifth sink of tile::walk_weights, a sibling of
// k_contrib, k_values, k_removal_base and k_removal, one workgroup per blend tile (qw x qh quadrants, one wave each).
struct GradientParams {
    FrameLists frame;             // (its counters' error bits are folded into *sticky: no blend need follow)
    const float4* base;           // pass 1 wrote it (launch_removal_base): (F_r, F_g, F_b, T_end) per viewport pixel
    size_t base_pitch;            // bytes, a multiple of 16
    const float4* grad;           // the caller's plane: (dL/dF_r, dL/dF_g, dL/dF_b, dL/dT_end) per viewport pixel
    size_t grad_pitch;            // bytes, a multiple of 16
    float scale;                  // of the plane: G = clamp(scale * g, -1, 1)
    float opacity_scale;          // of the opacity value: v_o = -clamp(opacity_scale * a, +-(1 - 2^-24))
    unsigned long long* sums;     // [num_points][GRAD_CHANNELS] two's-complement q32 sums
};
static_assert(offsetof(GradientParams, base) == 80, "the frame's lists first, as in ContribParams, ValuesParams and RemovalParams");
static_assert(sizeof(GradientParams) == 128, "kernarg segment of k_gradient");

// k_gradient<qw, qh> on the stream, behind launch_removal_base on the same stream with the same frame and base plane.
//
// TO THE BIT.  The pairs, the weights wgt = b * T and the stops are tile::walk_weights' (weight_walk.h), the one function
// k_contrib, k_values and k_removal run: nothing here influences them.  The staging thread of a slot also copies words 3 and 4 of
// its Splat record (the f16 colour and opacity) into a third plane of 8-B records, as k_removal does; c_ch below is that f16
// colour taken to f32.
//
// Every lane inside the viewport loads base(p) = (F, T_end) and g(p) as one float4 each and forms, per component k,
//   G_k = fminf(fmaxf(scale * g_k, -1), 1), NaN -> 0                   one rounded multiply
// a lane outside the viewport loads nothing and has G = 0; nothing past a row's width-th float4 is read.  A wave whose 64 x 4
// values of G are all 0 skips its walk (PlaneValue::idle's rule, accum_q32.h).  P_ch = 0, T = 1 (0 outside the viewport).  Per
// walked pair, removal.h's pass 2 as far as it goes:
//   Tb = T;  T = Tb - wgt                                              (wgt == 0 for a pair outside the cut-off)
//   kept:  P_ch = fmaf(wgt, c_ch, P_ch)
//   colour, per ch, counted iff kept && wgt > 0 && c_ch > 0:
//     v_ch = wgt * G_ch                                                one rounded multiply; |v_ch| < 1 (b <= 0.99)
//   opacity, counted iff kept && wgt > 0 && Tb >= 2^-14 && wgt != 0x1.fae148p-1f * Tb (one rounded multiply: b on the 0.99 clamp):
//     r, s_ch, t_ch, d_ch                                              removal.h's, the same operations in the same order
//     a = G_r * d_r;  a = fmaf(G_g, d_g, a);  a = fmaf(G_b, d_b, a)    one rounded multiply, two fused multiply-adds
//     u = r * T_end;  a = fmaf(G_T, u, a)                              one rounded multiply, one fused multiply-add
//     v_o = -fminf(fmaxf(opacity_scale * a, -0x1.fffffep-1f), 0x1.fffffep-1f), NaN -> 0     one rounded multiply
// and everything from the four v on is the signed accumulator's (accum_s32.h).
int launch_gradient(const GradientParams& p, hipStream_t stream);

// sums[i] += other[i] over n 64-bit words (ws_grad_add: two's-complement addition is the merge)
int launch_grad_merge(unsigned long long* sums, const unsigned long long* other, size_t n, hipStream_t stream);

}  // namespace ws
