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
#include "gradient_pair.h"

namespace ws {

namespace {

// gradient.h: four v per walked pair, into the accumulator.  LDS per staged record: its colour words beside the accumulator's
// four partials.  What is kept per pair and which pairs count is gradient_pair.h's, the one k_geometry runs too.
template <int STAGE>
struct GradientSink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;
    const GradientParams& p;
    uint2* s_col;
    AccumS32<STAGE> acc;
    GradPixel px{};

    __device__ __forceinline__ void begin(uint32_t x, uint32_t y, bool inside) {
        px.begin(p.base, p.base_pitch, p.grad, p.grad_pitch, p.scale, x, y, inside);
    }
    __device__ __forceinline__ bool idle() const { return px.none; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        acc.clear(tid);
        if (live) s_col[tid] = splat_colour_words(p.frame.splats, idx);
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool kept) {
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, vo = 0.0f;
        {
#pragma clang fp contract(off)  // one rounded multiply each
            const float Tb = px.step(wgt);
            if (kept) {
                float c[3];
                px.blend_in(s_col, off, wgt, c);
                if (wgt > 0.0f) {
                    if (c[0] > 0.0f) v0 = wgt * px.G0;
                    if (c[1] > 0.0f) v1 = wgt * px.G1;
                    if (c[2] > 0.0f) v2 = wgt * px.G2;
                    if (px.counts(Tb, wgt)) {
                        const float sa = p.opacity_scale * px.kappa(wgt, c);
                        vo = (sa != sa) ? 0.0f : -fminf(fmaxf(sa, -GRAD_V_CAP), GRAD_V_CAP);
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
