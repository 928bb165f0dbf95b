// geometry.hip -- the five screen-space sums every geometric derivative of an image loss is made of, per Gaussian, over a prepared
// frame (include/websplat.h, "Geometry gradients").  The blend evaluates b = min(0.99, alpha 2^-a'), a' = |p|^2,
// p = I' (x - mu); with kappa = -b dL/db of a pair (k_gradient's a), dL/da' = ln2 kappa, and
//
//   m_k = sum_p kappa p_k,  S_kl = sum_p kappa p_k p_l:   dL/dmu = -2 ln2 I'^T m,   dL/dSigma = -2 (ln2)^2 I'^T S I'
//
// Pass 1 is removal's base image, launched through launch_removal_base; pass 2 is the sixth sink of tile::walk_weights:
//
//   k_geometry : per walked pair the lane's five values s kappa (p0, p1, p0 p0, p0 p1, p1 p1) into the signed per-Gaussian
//                accumulator (accum_s32.h AccumS32x5).  |p|^2 <= CUT_A2 ~ 6.8 on a kept pair: the values are bounded as kappa is.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "geometry.h"
#include "gradient_pair.h"

namespace ws {

namespace {

__device__ __forceinline__ float geom_value(float v) { return (v != v) ? 0.0f : fminf(fmaxf(v, -GRAD_V_CAP), GRAD_V_CAP); }

// geometry.h: five v per walked pair, into the accumulator.  LDS per staged record: its colour words beside the accumulator's five
// partials.
template <int STAGE>
struct GeometrySink {
    static constexpr bool WRITES_EMPTY_TILES = false;
    static constexpr bool PAIR_IS_WAVE_WIDE = true;
    static constexpr bool WANTS_COORDS = true;
    const GeometryParams& p;
    uint2* s_col;
    AccumS32x5<STAGE> acc;
    GradPixel px{};

    __device__ __forceinline__ void begin(uint32_t x, uint32_t y, bool inside) {
        px.begin(p.base, p.base_pitch, p.grad, p.grad_pitch, p.scale, x, y, inside);
    }
    __device__ __forceinline__ bool idle() const { return px.none; }
    __device__ __forceinline__ void stage(int tid, uint32_t idx, bool live) {
        acc.clear(tid);
        if (live) s_col[tid] = splat_colour_words(p.frame.splats, idx);
    }
    __device__ __forceinline__ void pair(uint32_t off, float wgt, bool kept, float p0, float p1) {
        float v[GEOM_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        {
#pragma clang fp contract(off)  // every multiply below is rounded by itself
            const float Tb = px.step(wgt);
            if (kept) {
                float c[3];
                px.blend_in(s_col, off, wgt, c);
                if (wgt > 0.0f && px.counts(Tb, wgt)) {
                    const float t = p.geometry_scale * px.kappa(wgt, c);
                    const float t0 = t * p0, t1 = t * p1;
                    v[0] = geom_value(t0);
                    v[1] = geom_value(t1);
                    v[2] = geom_value(t0 * p0);
                    v[3] = geom_value(t0 * p1);
                    v[4] = geom_value(t1 * p1);
                }
            }
        }
        acc.add(off, v);
    }
    __device__ __forceinline__ void flush(int tid, uint32_t idx) { acc.flush(p.frame.src_index, tid, idx); }
    __device__ __forceinline__ void finish(uint32_t, uint32_t, bool) {}
};

template <int QW, int QH>
__global__ __launch_bounds__(64 * QW * QH) void k_geometry(const GeometryParams p) {
    constexpr int STAGE = tile::Geometry<QW, QH>::STAGE;
    __shared__ uint2 s_col[STAGE];
    __shared__ unsigned long long s_sum[GEOM_CHANNELS * STAGE];
    GeometrySink<STAGE> sink{p, s_col, {p.sums, s_sum}};
    tile::walk_weights<QW, QH>(p.frame, sink);
}

}  // namespace

int launch_geometry(const GeometryParams& p, hipStream_t stream) {
    const uint32_t grid = p.frame.tiles_x * p.frame.tiles_y;
    if (grid == 0) return WS_OK;
    const bool shaped = with_tile_shape(p.frame.qw, p.frame.qh, [&](auto qw, auto qh) {
        constexpr int QW = decltype(qw)::value, QH = decltype(qh)::value;
        hipLaunchKernelGGL((k_geometry<QW, QH>), dim3(grid), dim3(64 * QW * QH), 0, stream, p);
    });
    if (!shaped) return fail(WS_ERR_UNSUPPORTED, "launch_geometry: tile shape");
    // (the 4x4 tile declares 74 KB of LDS, above the 64 KB of most kernels here: a runtime that refuses it says so now)
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
