// gradient_pair.h -- what k_gradient (gradient.hip) and k_geometry (geometry.hip) keep per walked pair of tile::walk_weights, once:
// Tb, T, P_ch, r, d_ch, u and the scalar a = G_r d_r + G_g d_g + G_b d_b + G_T r T_end every derivative of the frame with respect to
// a splat's opacity or geometry is a multiple of (gradient.h names every operation; include/websplat.h "Gradients of an image loss").
// The two sinks take the steps of GradPixel in the same order: there is no second copy of this arithmetic, so they agree on the pairs they count to the bit.
#pragma once

#include "removal.h"

#if defined(__HIPCC__)
namespace ws {

constexpr float GRAD_V_CAP = 0x1.fffffep-1f;    // the largest f32 below 1: |v| * 2^32 fits 32 bits
constexpr float GRAD_B_CLAMP = 0x1.fae148p-1f;  // 0.99f, the cap of opacity_at (blend_tile.h)

__device__ __forceinline__ float grad_plane_value(float scale, float g) {
#pragma clang fp contract(off)
    const float e = scale * g;
    return (e != e) ? 0.0f : fminf(fmaxf(e, -1.0f), 1.0f);
}

// The lane's pixel: base(p), the clamped plane at p, and what the walk has accumulated through the pair at hand.
struct GradPixel {
    float F0 = 0.0f, F1 = 0.0f, F2 = 0.0f, Tend = 0.0f;  // base(p)
    float G0 = 0.0f, G1 = 0.0f, G2 = 0.0f, GT = 0.0f;    // the plane at p
    float P0 = 0.0f, P1 = 0.0f, P2 = 0.0f;               // the colour accumulated through the pair at hand
    float T = 0.0f;                                      // the walk's T again
    bool none = false;                                   // wave-uniform: nothing but zeros in the plane -- no walk to do

    // every lane, once, before the first batch: two float4 loads inside the viewport, none outside
    __device__ __forceinline__ void begin(const float4* base, size_t base_pitch, const float4* grad, size_t grad_pitch, float scale,
                                          uint32_t px, uint32_t py, bool inside) {
        if (inside) {
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + (size_t)py * base_pitch + (size_t)px * 16);
            const float4 g = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(grad) + (size_t)py * grad_pitch + (size_t)px * 16);
            F0 = b.x, F1 = b.y, F2 = b.z, Tend = b.w;
            G0 = grad_plane_value(scale, g.x), G1 = grad_plane_value(scale, g.y), G2 = grad_plane_value(scale, g.z), GT = grad_plane_value(scale, g.w);
            T = 1.0f;
        }
        none = __ballot(G0 != 0.0f || G1 != 0.0f || G2 != 0.0f || GT != 0.0f) == 0ull;
    }

    // One walked pair, in the four steps both sinks take in this order (every lane of the wave; wgt == 0 and kept == false outside
    // the cut-off):
    //   Tb = step(wgt)                         every pair
    //   blend_in(s_col, off, wgt, c)           iff kept: the staged f16 colour as f32, P_ch updated
    //   counts(Tb, wgt)                        iff kept and wgt > 0: the pair counts for the opacity and for the geometry
    //   kappa(wgt, c)                          iff it counts: gradient.h's a, before any scale
    // every operation the separately rounded one gradient.h names; the fmaf calls stay fused.
    __device__ __forceinline__ float step(float wgt) {
#pragma clang fp contract(off)
        const float Tb = T;
        T = Tb - wgt;
        return Tb;
    }
    __device__ __forceinline__ void blend_in(const uint2* s_col, uint32_t off, float wgt, float (&c)[3]) {
        const f16x4_t c16 = staged_colour(s_col, off);
        c[0] = (float)c16.x, c[1] = (float)c16.y, c[2] = (float)c16.z;
        P0 = fmaf(wgt, c[0], P0);
        P1 = fmaf(wgt, c[1], P1);
        P2 = fmaf(wgt, c[2], P2);
    }
    __device__ __forceinline__ bool counts(float Tb, float wgt) const {
#pragma clang fp contract(off)
        return Tb >= T_MIN && wgt != GRAD_B_CLAMP * Tb;  // (T > 0: b <= 0.99)
    }
    __device__ __forceinline__ float kappa(float wgt, const float (&c)[3]) const {
#pragma clang fp contract(off)
        const float r = wgt / T;
        const float d0 = fmaf(r, F0 - P0, -(wgt * c[0]));
        const float d1 = fmaf(r, F1 - P1, -(wgt * c[1]));
        const float d2 = fmaf(r, F2 - P2, -(wgt * c[2]));
        float a = G0 * d0;
        a = fmaf(G1, d1, a);
        a = fmaf(G2, d2, a);
        const float u = r * Tend;
        a = fmaf(GT, u, a);
        return a;
    }
};

}  // namespace ws
#endif  // __HIPCC__
