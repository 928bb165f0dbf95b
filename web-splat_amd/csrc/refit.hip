// refit.hip -- Adam steps on the DC colour and the opacity of a resident, uncompressed cloud, in place (include/websplat.h,
// "Refitting colour and opacity"; refit.h has the step to the bit).  Purely streaming: one thread per Gaussian,
// no LDS, no atomics.  Per Gaussian the step reads the four int64 sums as two 16-B loads and masters, first and second moments as
// one float4 each, writes the three float4 back, and of the planes reads the two 4-B words that also hold bytes of other fields
// and writes 12 B (one word of plane 0, two of plane 2): ~140 B in all, every wave access contiguous in the Gaussian index.
//
// Compiled with -ffp-contract=off (Makefile STRICT): every f32 operation below is rounded by itself.
#include <hip/hip_runtime.h>

#include "refit.h"

namespace ws {

namespace {

__device__ __forceinline__ float half_bits_to_f32(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xFFFFu)); }
__device__ __forceinline__ uint32_t f32_to_half_bits(float x) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)x); }  // nearest even

__device__ __forceinline__ float clamp_to(float x, float lo, float hi) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

struct Adam {
    float beta1, beta2, omb1, omb2, bc1, bc2, eps;
    // one channel: refit.h's m', v', x' before the clamp
    __device__ __forceinline__ float step(float g, float lr, float x, float& m, float& v) const {
        const float m1 = (beta1 * m) + (omb1 * g);
        const float v1 = (beta2 * v) + (omb2 * (g * g));
        const float s = (m1 / bc1) / (sqrtf(v1 / bc2) + eps);
        m = m1;
        v = v1;
        return x - (lr * s);
    }
};

__device__ __forceinline__ float unit_gradient(unsigned long long q, double u) { return (float)((double)(long long)q * u); }

__global__ __launch_bounds__(256) void k_refit_step(const RefitParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    const ulonglong2* sums = reinterpret_cast<const ulonglong2*>(p.sums) + (size_t)i * 2;
    const ulonglong2 q01 = sums[0], q23 = sums[1];
    float4 x = p.master[i], m = p.m[i], v = p.v[i];
    uint32_t* plane0 = reinterpret_cast<uint32_t*>(p.planes) + (size_t)i * 4;
    uint32_t* plane2 = reinterpret_cast<uint32_t*>(p.planes) + ((size_t)2 * p.n + i) * 4;
    const Adam a{p.beta1, p.beta2, p.omb1, p.omb2, p.bc1, p.bc2, p.eps};
    if (p.lr_colour != 0.0f) {
        x.x = clamp_to(a.step(unit_gradient(q01.x, p.u_colour), p.lr_colour, x.x, m.x, v.x), -REFIT_DC_MAX, REFIT_DC_MAX);
        x.y = clamp_to(a.step(unit_gradient(q01.y, p.u_colour), p.lr_colour, x.y, m.y, v.y), -REFIT_DC_MAX, REFIT_DC_MAX);
        x.z = clamp_to(a.step(unit_gradient(q23.x, p.u_colour), p.lr_colour, x.z, m.z, v.z), -REFIT_DC_MAX, REFIT_DC_MAX);
        const uint32_t behind = plane2[1] & 0xFFFF0000u;  // the first half of SH coefficient 1
        const uint2 w = make_uint2(f32_to_half_bits(x.x) | (f32_to_half_bits(x.y) << 16), f32_to_half_bits(x.z) | behind);
        *reinterpret_cast<uint2*>(plane2) = w;
    }
    if (p.lr_opacity != 0.0f) {
        float g = unit_gradient(q23.y, p.u_opacity);
        g = (x.w == 0.0f) ? 0.0f : g / x.w;
        x.w = clamp_to(a.step(g, p.lr_opacity, x.w, m.w, v.w), p.opacity_min, 1.0f);
        plane0[3] = f32_to_half_bits(x.w) | (plane0[3] & 0xFFFF0000u);  // (the loader's padding beside the opacity)
    }
    p.master[i] = x;
    p.m[i] = m;
    p.v[i] = v;
}

__global__ __launch_bounds__(256) void k_refit_init(const uint4* planes, uint32_t n, float4* master, float4* m, float4* v) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t* plane0 = reinterpret_cast<const uint32_t*>(planes) + (size_t)i * 4;
    const uint32_t* plane2 = reinterpret_cast<const uint32_t*>(planes) + ((size_t)2 * n + i) * 4;
    const uint2 dc = *reinterpret_cast<const uint2*>(plane2);
    master[i] = make_float4(half_bits_to_f32(dc.x), half_bits_to_f32(dc.x >> 16), half_bits_to_f32(dc.y), half_bits_to_f32(plane0[3]));
    m[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One thread per (Gaussian, SH plane): blockIdx.y = 0 is plane 2, whose thread also takes the DC triple and the opacity, exactly as
// k_refit_step does.  The thread steps those of the eight halves of its 16-B chunk that are rest elements (3 <= e < 3 ncoef) and
// stores the chunk as one uint4; every other half goes back with the bits it was read with.
__global__ __launch_bounds__(256) void k_refit_step_sh(const RefitShParams sp) {
    const RefitParams& p = sp.base;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    const size_t n = p.n;
    const uint32_t py = blockIdx.y;
    const unsigned long long* q = sp.sh_sums + i;  // element e of this Gaussian: q[e * n]
    const Adam a{p.beta1, p.beta2, p.omb1, p.omb2, p.bc1, p.bc2, p.eps};
    uint4* chunk = p.planes + ((size_t)(2u + py) * n + i);
    const uint4 w = *chunk;
    uint32_t h[8] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16, w.z & 0xFFFFu, w.z >> 16, w.w & 0xFFFFu, w.w >> 16};
    if (py == 0u) {
        float4 x = p.master[i], m = p.m[i], v = p.v[i];
        if (p.lr_colour != 0.0f) {
            x.x = clamp_to(a.step(unit_gradient(q[0], p.u_colour), p.lr_colour, x.x, m.x, v.x), -REFIT_DC_MAX, REFIT_DC_MAX);
            x.y = clamp_to(a.step(unit_gradient(q[n], p.u_colour), p.lr_colour, x.y, m.y, v.y), -REFIT_DC_MAX, REFIT_DC_MAX);
            x.z = clamp_to(a.step(unit_gradient(q[2 * n], p.u_colour), p.lr_colour, x.z, m.z, v.z), -REFIT_DC_MAX, REFIT_DC_MAX);
            h[0] = f32_to_half_bits(x.x);
            h[1] = f32_to_half_bits(x.y);
            h[2] = f32_to_half_bits(x.z);
        }
        if (p.lr_opacity != 0.0f) {
            uint32_t* plane0 = reinterpret_cast<uint32_t*>(p.planes) + (size_t)i * 4;
            float g = unit_gradient(q[(size_t)(3u * sp.ncoef) * n], p.u_opacity);
            g = (x.w == 0.0f) ? 0.0f : g / x.w;
            x.w = clamp_to(a.step(g, p.lr_opacity, x.w, m.w, v.w), p.opacity_min, 1.0f);
            plane0[3] = f32_to_half_bits(x.w) | (plane0[3] & 0xFFFF0000u);  // (the loader's padding beside the opacity)
        }
        if (p.lr_colour != 0.0f || p.lr_opacity != 0.0f) {
            p.master[i] = x;
            p.m[i] = m;
            p.v[i] = v;
        }
    }
    if (sp.lr_sh != 0.0f) {
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t e = py * 8u + j;
            if (e < 3u || e >= 3u * sp.ncoef) continue;  // the DC triple; padding past the cloud's degree
            const size_t at = (size_t)(e - 3u) * n + i;
            float x = sp.sh_master[at], m = sp.sh_m[at], v = sp.sh_v[at];
            x = clamp_to(a.step(unit_gradient(q[(size_t)e * n], sp.u_sh), sp.lr_sh, x, m, v), -REFIT_DC_MAX, REFIT_DC_MAX);
            sp.sh_master[at] = x;
            sp.sh_m[at] = m;
            sp.sh_v[at] = v;
            h[j] = f32_to_half_bits(x);
        }
    }
    if ((py == 0u && p.lr_colour != 0.0f) || sp.lr_sh != 0.0f)
        *chunk = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// masters of the rest elements = their halves widened, m = v = 0: one thread per (Gaussian, SH plane)
__global__ __launch_bounds__(256) void k_refit_init_sh(const uint4* planes, uint32_t n32, uint32_t ncoef, float* master, float* m, float* v) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n32) return;
    const size_t n = n32;
    const uint32_t py = blockIdx.y;
    const uint4 w = planes[(size_t)(2u + py) * n + i];
    const uint32_t h[8] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16, w.z & 0xFFFFu, w.z >> 16, w.w & 0xFFFFu, w.w >> 16};
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t e = py * 8u + j;
        if (e < 3u || e >= 3u * ncoef) continue;
        const size_t at = (size_t)(e - 3u) * n + i;
        master[at] = half_bits_to_f32(h[j]);
        m[at] = 0.0f;
        v[at] = 0.0f;
    }
}

}  // namespace

int launch_refit_step_sh(const RefitShParams& p, hipStream_t stream) {
    if (p.base.n == 0) return WS_OK;
    // a frozen rest group leaves planes 3.. alone: only plane 2's threads have work
    const uint32_t planes = p.lr_sh != 0.0f ? refit_sh_planes(p.ncoef) : 1u;
    hipLaunchKernelGGL(k_refit_step_sh, dim3((p.base.n + 255u) / 256u, planes), dim3(256), 0, stream, p);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_refit_init_sh(const uint4* planes, uint32_t n, uint32_t ncoef, float* master, float* m, float* v, hipStream_t stream) {
    if (n == 0 || ncoef <= 1u) return WS_OK;
    hipLaunchKernelGGL(k_refit_init_sh, dim3((n + 255u) / 256u, refit_sh_planes(ncoef)), dim3(256), 0, stream, planes, n, ncoef, master, m, v);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_refit_step(const RefitParams& p, hipStream_t stream) {
    if (p.n == 0) return WS_OK;
    hipLaunchKernelGGL(k_refit_step, dim3((p.n + 255u) / 256u), dim3(256), 0, stream, p);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_refit_init(const uint4* planes, uint32_t n, float4* master, float4* m, float4* v, hipStream_t stream) {
    if (n == 0) return WS_OK;
    hipLaunchKernelGGL(k_refit_init, dim3((n + 255u) / 256u), dim3(256), 0, stream, planes, n, master, m, v);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
