// gradient.hip -- dL/d(colour) and dL/d(ln opacity) of an image loss per Gaussian, over a prepared frame (include/websplat.h,
// "Gradients of an image loss").  The prepared frame F is linear in each splat's colour, dF(p)/dc_i = w_i(p), and
// affine in each splat's per-pixel opacity b_i: b_i dF(p)/db_i = -D_i(p), b_i dT_end(p)/db_i = -r_i T_end(p), with D_i the
// change of the pixel k_removal forms (removal.hip) and r_i = b_i / (1 - b_i).  Pass 1 is removal's base image, launched through
// launch_removal_base; pass 2 is the fifth sink of tile::walk_weights (weight_walk.h):
//
//   k_gradient : per walked pair the lane's four values v = (w G_r, w G_g, w G_b, -(G . D + G_T r T_end)), G the caller's
//                per-pixel loss gradient, into the signed per-Gaussian accumulator (accum_s32.h).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "gradient.h"

namespace ws {

namespace {

constexpr float V_CAP = 0x1.fffffep-1f;    // the largest f32 below 1: |v| * 2^32 fits 32 bits
constexpr float B_CLAMP = 0x1.fae148p-1f;  // 0.99f, the cap of opacity_at (blend_tile.h)

__device__ __forceinline__ float plane_value(float scale, float g) {
#pragma clang fp contract(off)
    const float e = scale * g;
    return (e != e) ? 0.0f : fminf(fmaxf(e, -1.0f), 1.0f);
}

// gradient.h: four v per walked pair, into the accumulator.  LDS per staged record: its colour words beside the accumulator's
// four partials.
template <int STAGE>
struct GradientSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;
    const GradientParams& p;
    uint2* s_col;
    AccumS32<STAGE> acc;
    float F0 = 0.0f, F1 = 0.0f, F2 = 0.0f, Tend = 0.0f;  // base(p)
    float G0 = 0.0f, G1 = 0.0f, G2 = 0.0f, GT = 0.0f;    // the plane at p
    float P0 = 0.0f, P1 = 0.0f, P2 = 0.0f;               // the colour accumulated through the pair at hand
    float T = 0.0f;                                      // the walk's T again
    bool none = false;                                   // wave-uniform: nothing but zeros in the plane -- no walk to do

    __device__ __forceinline__ void begin(uint32_t px, uint32_t py, bool inside) {
        if (inside) {
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.base) + (size_t)py * p.base_pitch + (size_t)px * 16);
            const float4 g = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.grad) + (size_t)py * p.grad_pitch + (size_t)px * 16);
            F0 = b.x, F1 = b.y, F2 = b.z, Tend = b.w;
            G0 = plane_value(p.scale, g.x), G1 = plane_value(p.scale, g.y), G2 = plane_value(p.scale, g.z), GT = plane_value(p.scale, g.w);
            T = 1.0f;
        }
        none = __ballot(G0 != 0.0f || G1 != 0.0f || G2 != 0.0f || GT != 0.0f) == 0ull;
    }
    __device__ __forceinline__ bool idle() const { return none; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        acc.clear(tid);
        if (live) s_col[tid] = splat_colour_words(p.frame.splats, idx);
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool kept) {
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, vo = 0.0f;
        {
#pragma clang fp contract(off)  // every step below is the separately rounded operation gradient.h names; the fmaf calls stay fused
            const float Tb = T;
            T = Tb - wgt;
            if (kept) {
                const f16x4_t c16 = staged_colour(s_col, off);
                const float c0 = (float)c16.x, c1 = (float)c16.y, c2 = (float)c16.z;
                P0 = fmaf(wgt, c0, P0);
                P1 = fmaf(wgt, c1, P1);
                P2 = fmaf(wgt, c2, P2);
                if (wgt > 0.0f) {
                    if (c0 > 0.0f) v0 = wgt * G0;
                    if (c1 > 0.0f) v1 = wgt * G1;
                    if (c2 > 0.0f) v2 = wgt * G2;
                    if (Tb >= T_MIN && wgt != B_CLAMP * Tb) {  // (T > 0: b <= 0.99)
                        const float r = wgt / T;
                        const float d0 = fmaf(r, F0 - P0, -(wgt * c0));
                        const float d1 = fmaf(r, F1 - P1, -(wgt * c1));
                        const float d2 = fmaf(r, F2 - P2, -(wgt * c2));
                        float a = G0 * d0;
                        a = fmaf(G1, d1, a);
                        a = fmaf(G2, d2, a);
                        const float u = r * Tend;
                        a = fmaf(GT, u, a);
                        const float sa = p.opacity_scale * a;
                        vo = (sa != sa) ? 0.0f : -fminf(fmaxf(sa, -V_CAP), V_CAP);
                    }
                }
            }
        }
        acc.add(off, v0, v1, v2, vo);
    }
    __device__ __forceinline__ void flush(int tid, uint32_t idx) { acc.flush(p.frame.src_index, tid, idx); }
    __device__ __forceinline__ void finish(uint32_t, uint32_t, bool) {}
};

template <int QW, int QH>
__global__ __launch_bounds__(64 * QW * QH) void k_gradient(const GradientParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ uint2 s_col[STAGE];
    __shared__ unsigned long long s_sum[GRAD_CHANNELS * STAGE];
    GradientSink<STAGE> sink{p, s_col, {p.sums, s_sum}};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

__global__ __launch_bounds__(256) void k_grad_merge(unsigned long long* sums, const unsigned long long* other, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sums[i] += other[i];
}

}  // namespace

int launch_gradient(const GradientParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        hipLaunchKernelGGL((k_gradient<QW, QH>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_gradient: tile shape");
    // (the 4x4 tile declares 70 KB of LDS, above the 64 KB of every other kernel here: a runtime that refuses it says so now)
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_grad_merge(unsigned long long* sums, const unsigned long long* other, size_t n, hipStream_t stream) {
    if (n == 0) return WS_OK;
    hipLaunchKernelGGL(k_grad_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sums, other, n);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
