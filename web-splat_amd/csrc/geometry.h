// geometry.h -- the screen-space geometry sums of an image loss, per Gaussian, over a prepared frame (geometry.hip k_geometry; pass
// 1 is removal.hip's k_removal_base; geometry_spread.h takes the sums on to position and covariance).  Internal: the ABI is
// include/websplat.h, "Geometry gradients"; DESIGN.md 3.4n.
#pragma once

#include <cstddef>

#include "accum_s32.h"
#include "removal.h"

namespace ws {

// One launch over a prepared frame's binned, depth-ordered tile lists: the sixth sink of tile::walk_weights, a sibling of
// k_gradient, one workgroup per blend tile (qw x qh quadrants, one wave each).
struct GeometryParams {
    FrameLists frame;             // (its counters' error bits are folded into *sticky: no blend need follow)
    const float4* base;           // pass 1 wrote it (launch_removal_base): (F_r, F_g, F_b, T_end) per viewport pixel
    size_t base_pitch;            // bytes, a multiple of 16
    const float4* grad;           // the caller's plane: (dL/dF_r, dL/dF_g, dL/dF_b, dL/dT_end) per viewport pixel
    size_t grad_pitch;            // bytes, a multiple of 16
    float scale;                  // of the plane: G = clamp(scale * g, -1, 1)
    float geometry_scale;         // s of the five values: t = s * kappa
    unsigned long long* sums;     // [num_points][GEOM_CHANNELS] two's-complement q32 sums: m0, m1, S00, S01, S11
};
static_assert(offsetof(GeometryParams, base) == 80, "the frame's lists first, as in GradientParams");
static_assert(sizeof(GeometryParams) == 128, "kernarg segment of k_geometry");

// k_geometry<qw, qh> on the stream, behind launch_removal_base on the same stream with the same frame and base plane.
//
// TO THE BIT.  The pairs, the weights and the stops are tile::walk_weights'; p0, p1 are the walk's own values of the pair (its
// WANTS_COORDS hook), the exp2-domain coordinates p = I' (x - mu) with a' = p0^2 + p1^2 <= CUT_A2 on every kept pair.  Per walked
// pair the lane keeps Tb, T, P_ch and forms r, d_ch, u and kappa = a exactly as k_gradient does -- gradient_pair.h is the one copy
// of that arithmetic -- and a pair is counted iff k_gradient counts it for the opacity: kept, wgt > 0, Tb >= 2^-14, b not on the
// 0.99 clamp.  A pair that is not counted has five zeros.  For a counted pair, every multiply rounded by itself:
//   t     = geometry_scale * kappa
//   v_m0  = t * p0              v_m1  = t * p1
//   v_S00 = (t * p0) * p0       v_S01 = (t * p0) * p1       v_S11 = (t * p1) * p1
// each NaN -> 0 and capped silently at +-0x1.fffffep-1f; everything from the five v on is the signed accumulator's (accum_s32.h,
// AccumS32x5).  g and -g give exactly negated values (kappa is odd in G and every later step is a multiply or a clamp).
int launch_geometry(const GeometryParams& p, hipStream_t stream);

}  // namespace ws
