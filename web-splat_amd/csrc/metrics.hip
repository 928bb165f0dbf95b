// metrics.hip -- PSNR and SSIM between two resident images (include/websplat.h, "Image metrics").
//
//   k_image_metrics    : one fused pass over both images.  A workgroup of 256 threads owns a 32 x 16 output tile.  It loads the
//                        tile plus the window's 5-pixel halo (42 x 26 pixels) of BOTH images once -- one vector load per texel,
//                        a thread's ten loads issued before the first is decoded (one instantiation per format pair: no
//                        branch among them), the pixel value (background, clamp, optional 8-bit quantisation) computed there
//                        and never again -- into six f32 LDS planes (x and y, three channels); pixels outside the image are
//                        stored as 0, which is the zero padding.  Then, per channel: the horizontal 11-tap pass of the five
//                        moment planes (x, y, xx, yy, xy) from those planes into LDS, the vertical pass in registers (a thread
//                        owns two vertically adjacent pixels and shares the 12 rows they read), the SSIM value, and the squared
//                        error of its own pixels.  Moments are taken in f64: g * x and x * x are exact there, so sigma^2 =
//                        E[x^2] - mu^2 loses nothing to the cancellation that costs an f32 evaluation up to 1e-3 of map value
//                        on flat images (tests/metrics_ref.py).
//                        LDS: 6 x 26 x 43 x 4 B (rows padded to an odd stride) + 5 x 26 x 32 x 8 B = 60 112 B, 60 208 B with
//                        the reduction scratch: two workgroups per CU.  Both passes read and write with consecutive lanes on
//                        consecutive words of one row: no bank is hit twice by a lane group.
//   reduction          : no float atomics.  A thread sums its (at most six) values in a fixed order, a wave reduces by shuffles
//                        in a fixed tree, the four waves meet in LDS and thread 0 adds them in wave order and stores ONE
//                        partial record per workgroup with ordinary vector stores.
//   k_image_error      : the per-pixel error plane of ws_image_error_plane: one thread per pixel, the two texels through the same
//                        texel_load / pixel_value, no reduction and no atomics.
//   k_image_error_grad : beside it, the derivative of that plane's value with respect to image a's pixel value, one float4
//                        per pixel (ws_image_error_gradient): the loss gradient k_gradient (gradient.hip) takes.
//   k_metrics_finalize : one workgroup behind it: thread t adds records t, t + 256, ... in index order, the 256 sums are
//                        folded by a fixed tree, and the image's record goes to the accumulator.  Bitwise reproducible.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "metrics.h"

namespace ws {

namespace {

constexpr int TW = (int)METRICS_TILE_W, TH = (int)METRICS_TILE_H, HALO = (int)METRICS_HALO;
constexpr int RW = TW + 2 * HALO, RH = TH + 2 * HALO;  // the region a tile reads: 42 x 26
constexpr int VS = RW + 1;                             // row stride of the value planes, in floats (odd)
constexpr int NT = 256;
static_assert(NT == TW * TH / 2, "a thread owns two vertically adjacent pixels of the tile");

// The 11-tap window g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double and rounded to f32 (websplat.h lists
// the same six values); the 2-D window is the outer product.
__host__ __device__ constexpr double gw(int k) {
    constexpr double g[6] = {0x1.0d956cp-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c4p-3, 0x1.10656p-2};
    return g[k < 6 ? k : 10 - k];
}
constexpr double SSIM_C1 = 0.01 * 0.01, SSIM_C2 = 0.03 * 0.03;

__device__ __forceinline__ float h2f(uint32_t bits) { return __half2float(__ushort_as_half((unsigned short)(bits & 0xFFFFu))); }

// The pixel value of websplat.h, one channel: three separately rounded operations over the background, clamp with NaN -> 0,
// optional quantisation by truncation
__device__ __forceinline__ float channel_over(float c, float a, const MetricsView& v, int ch) {  // (before the clamp)
    float r = c;
    if (v.over_bg) {
        const float k = __fsub_rn(1.0f, a);
        const float t = __fmul_rn(v.bg[ch], k);
        r = __fadd_rn(c, t);
    }
    return r;
}
__device__ __forceinline__ float channel_value(float c, float a, const MetricsView& v, int ch, bool quantize) {
    float r = channel_over(c, a, v, ch);
    r = (r != r) ? 0.0f : fminf(fmaxf(r, 0.0f), 1.0f);
    if (quantize) {
        const uint32_t q = (uint32_t)__fmul_rn(r, 255.0f);  // truncation: ws_download_texture_rgba8's rule
        r = __fdiv_rn((float)q, 255.0f);
    }
    return r;
}

// texel (x, y) of a view as raw words -- one 16 / 8 / 4-B vector load; (x, y) is inside the image: nothing past the row's last
// texel is read -- and its decoding, as k_display decodes it.  Two steps, so that a thread's loads are all in flight before the
// first is used.
template <int FORMAT>
__device__ __forceinline__ uint4 texel_load(const MetricsView& v, int x, int y) {
    const char* row = reinterpret_cast<const char*>(v.pixels) + (size_t)y * v.pitch;
    if constexpr (FORMAT == WS_FORMAT_RGBA32_FLOAT) {
        return reinterpret_cast<const uint4*>(row)[x];
    } else if constexpr (FORMAT == WS_FORMAT_RGBA16_FLOAT) {
        const uint2 t = reinterpret_cast<const uint2*>(row)[x];
        return make_uint4(t.x, t.y, 0u, 0u);
    } else {
        return make_uint4(reinterpret_cast<const uint32_t*>(row)[x], 0u, 0u, 0u);
    }
}
template <int FORMAT>
__device__ __forceinline__ float4 texel_decode(uint4 t) {
    float r, g, b, a;
    if constexpr (FORMAT == WS_FORMAT_RGBA32_FLOAT) {
        r = __uint_as_float(t.x); g = __uint_as_float(t.y); b = __uint_as_float(t.z); a = __uint_as_float(t.w);
    } else if constexpr (FORMAT == WS_FORMAT_RGBA16_FLOAT) {
        r = h2f(t.x); g = h2f(t.x >> 16); b = h2f(t.y); a = h2f(t.y >> 16);
    } else {
        r = (float)(t.x & 255u) / 255.0f; g = (float)((t.x >> 8) & 255u) / 255.0f;
        b = (float)((t.x >> 16) & 255u) / 255.0f; a = (float)(t.x >> 24) / 255.0f;
    }
    return make_float4(r, g, b, a);
}
template <int FORMAT>
__device__ __forceinline__ float3 pixel_value(const MetricsView& v, uint4 t, bool quantize) {
    const float4 c = texel_decode<FORMAT>(t);
    return make_float3(channel_value(c.x, c.w, v, 0, quantize), channel_value(c.y, c.w, v, 1, quantize), channel_value(c.z, c.w, v, 2, quantize));
}

// fixed trees over the wave's 64 lanes: the total ends in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// FA / FB: the ws_color_format of image a / b (nine instantiations: the load phase has no branch on the format)
template <int FA, int FB>
__global__ __launch_bounds__(NT) void k_image_metrics(const MetricsParams p) {
    __shared__ float s_val[6][RH][VS];   // x.r x.g x.b y.r y.g y.b over the region
    __shared__ double s_h[5][RH][TW];    // one channel's horizontally filtered moments: x, y, xx, yy, xy
    __shared__ double s_red[NT / 64][2];
    __shared__ unsigned long long s_redq[NT / 64];

    const int tid = threadIdx.x;
    const int W = (int)p.width, H = (int)p.height;
    const bool quantize = (p.flags & WS_METRICS_QUANTIZE_U8) != 0u;
    const int x0 = (int)blockIdx.x * TW - HALO, y0 = (int)blockIdx.y * TH - HALO;

    // ---- load: the pixel value of both images, once per region pixel; every load of the thread is issued before the first decode
    constexpr int LOADS = (RW * RH + NT - 1) / NT;
    uint4 ta[LOADS], tb[LOADS];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int i = tid + k * NT, ry = i / RW, rx = i - ry * RW;
        const int gx = x0 + rx, gy = y0 + ry;
        ta[k] = tb[k] = make_uint4(0u, 0u, 0u, 0u);
        if (i < RW * RH && gx >= 0 && gy >= 0 && gx < W && gy < H) {
            ta[k] = texel_load<FA>(p.a, gx, gy);
            tb[k] = texel_load<FB>(p.b, gx, gy);
        }
    }
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int i = tid + k * NT, ry = i / RW, rx = i - ry * RW;
        const int gx = x0 + rx, gy = y0 + ry;
        if (i >= RW * RH) break;
        float3 va = make_float3(0.0f, 0.0f, 0.0f), vb = va;
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            va = pixel_value<FA>(p.a, ta[k], quantize);
            vb = pixel_value<FB>(p.b, tb[k], quantize);
        }
        s_val[0][ry][rx] = va.x; s_val[1][ry][rx] = va.y; s_val[2][ry][rx] = va.z;
        s_val[3][ry][rx] = vb.x; s_val[4][ry][rx] = vb.y; s_val[5][ry][rx] = vb.z;
    }
    __syncthreads();

    // this thread's two pixels: column tx, rows 2 tr and 2 tr + 1 of the tile
    const int tx = tid & (TW - 1), tr = tid >> 5;
    const int px = (int)blockIdx.x * TW + tx, py = (int)blockIdx.y * TH + 2 * tr;
    const bool in0 = px < W && py < H, in1 = px < W && py + 1 < H;

    double sse = 0.0, ssim_sum = 0.0, map0 = 0.0, map1 = 0.0;
    unsigned long long sse_u8 = 0ull;

    for (int c = 0; c < 3; ++c) {
        // ---- horizontal pass: 26 region rows x 32 tile columns
        for (int i = tid; i < RH * TW; i += NT) {
            const int r = i >> 5, x = i & (TW - 1);
            const float* xr = &s_val[c][r][x];
            const float* yr = &s_val[3 + c][r][x];
            double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double g = gw(k), a = (double)xr[k], b = (double)yr[k];
                const double ga = g * a, gb = g * b;  // exact: 24 + 24 significant bits
                mx += ga;
                my += gb;
                xx = fma(ga, a, xx);
                yy = fma(gb, b, yy);
                xy = fma(ga, b, xy);
            }
            s_h[0][r][x] = mx; s_h[1][r][x] = my; s_h[2][r][x] = xx; s_h[3][r][x] = yy; s_h[4][r][x] = xy;
        }
        __syncthreads();
        // ---- vertical pass in registers: rows 2 tr .. 2 tr + 11 serve both pixels
        double m0[5], m1[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const double v = s_h[m][2 * tr + j][tx];
                if (j < 11) a0 = fma(gw(j), v, a0);
                if (j > 0) a1 = fma(gw(j - 1), v, a1);
            }
            m0[m] = a0;
            m1[m] = a1;
        }
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const double* m = o ? m1 : m0;
            if (!(o ? in1 : in0)) continue;
            const double mux2 = m[0] * m[0], muy2 = m[1] * m[1], muxy = m[0] * m[1];
            const double sx = m[2] - mux2, sy = m[3] - muy2, sxy = m[4] - muxy;
            const double v = ((2.0 * muxy + SSIM_C1) * (2.0 * sxy + SSIM_C2)) / ((mux2 + muy2 + SSIM_C1) * (sx + sy + SSIM_C2));
            ssim_sum += v;
            if (o) map1 += v; else map0 += v;
            // the squared error of this pixel's channel c
            const float x = s_val[c][2 * tr + o + HALO][tx + HALO], y = s_val[3 + c][2 * tr + o + HALO][tx + HALO];
            const float d = __fsub_rn(x, y);
            sse += (double)__fmul_rn(d, d);
            if (quantize) {
                const int qd = __float2int_rn(__fmul_rn(x, 255.0f)) - __float2int_rn(__fmul_rn(y, 255.0f));  // x = q / 255: q again
                sse_u8 += (unsigned long long)(qd * qd);
            }
        }
        __syncthreads();  // s_h is rewritten by the next channel
    }
    if (p.map) {
        char* at = reinterpret_cast<char*>(p.map) + (size_t)py * p.map_pitch + (size_t)px * 4;
        if (in0) *reinterpret_cast<float*>(at) = (float)(map0 / 3.0);
        if (in1) *reinterpret_cast<float*>(at + p.map_pitch) = (float)(map1 / 3.0);
    }

    // ---- the tile's partial record: shuffles, then the four waves in order
    sse = wave_sum(sse);
    ssim_sum = wave_sum(ssim_sum);
    sse_u8 = wave_sum(sse_u8);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        s_red[wave][0] = sse;
        s_red[wave][1] = ssim_sum;
        s_redq[wave] = sse_u8;
    }
    __syncthreads();
    if (tid == 0) {
        MetricsPartial out;
        out.sse = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
        out.ssim_sum = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
        out.sse_u8 = s_redq[0] + s_redq[1] + s_redq[2] + s_redq[3];
        p.slab[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = out;
    }
}

constexpr int EW = 64, EH = 4;  // the pixels of one workgroup of k_image_error: a wave per row segment

template <int FA, int FB>
__global__ __launch_bounds__(EW * EH) void k_image_error(const ImageErrorParams p) {
    const int x = (int)blockIdx.x * EW + (int)(threadIdx.x & (EW - 1)), y = (int)blockIdx.y * EH + (int)(threadIdx.x / EW);
    if (x >= (int)p.width || y >= (int)p.height) return;
    const bool quantize = (p.flags & WS_METRICS_QUANTIZE_U8) != 0u;
    const uint4 ta = texel_load<FA>(p.a, x, y), tb = texel_load<FB>(p.b, x, y);
    const float3 va = pixel_value<FA>(p.a, ta, quantize), vb = pixel_value<FB>(p.b, tb, quantize);
    const float dr = __fsub_rn(va.x, vb.x), dg = __fsub_rn(va.y, vb.y), db = __fsub_rn(va.z, vb.z);
    const bool sq = p.kind == WS_ERROR_SQ;
    const float er = sq ? __fmul_rn(dr, dr) : fabsf(dr), eg = sq ? __fmul_rn(dg, dg) : fabsf(dg), eb = sq ? __fmul_rn(db, db) : fabsf(db);
    *reinterpret_cast<float*>(reinterpret_cast<char*>(p.plane) + (size_t)y * p.plane_pitch + (size_t)x * 4) =
        __fdiv_rn(__fadd_rn(__fadd_rn(er, eg), eb), 3.0f);
}

// One channel of k_image_error_grad: the derivative of k_image_error's plane value with respect to image a's pixel value
__device__ __forceinline__ float error_grad(float raw, float x, float y, bool sq) {
    if (!(raw >= 0.0f && raw <= 1.0f)) return 0.0f;  // a's value sits on the clamp (or was NaN): it does not move with the texel
    const float d = __fsub_rn(x, y);
    if (sq) return __fdiv_rn(__fmul_rn(2.0f, d), 3.0f);
    return d == 0.0f ? 0.0f : copysignf(__fdiv_rn(1.0f, 3.0f), d);
}

template <int FA, int FB>
__global__ __launch_bounds__(EW * EH) void k_image_error_grad(const ImageErrorParams p) {
    const int x = (int)blockIdx.x * EW + (int)(threadIdx.x & (EW - 1)), y = (int)blockIdx.y * EH + (int)(threadIdx.x / EW);
    if (x >= (int)p.width || y >= (int)p.height) return;
    const uint4 ta = texel_load<FA>(p.a, x, y), tb = texel_load<FB>(p.b, x, y);
    const float4 ca = texel_decode<FA>(ta);
    const float3 va = pixel_value<FA>(p.a, ta, false), vb = pixel_value<FB>(p.b, tb, false);
    const bool sq = p.kind == WS_ERROR_SQ;
    const float4 g = make_float4(error_grad(channel_over(ca.x, ca.w, p.a, 0), va.x, vb.x, sq), error_grad(channel_over(ca.y, ca.w, p.a, 1), va.y, vb.y, sq),
                                 error_grad(channel_over(ca.z, ca.w, p.a, 2), va.z, vb.z, sq), 0.0f);
    *reinterpret_cast<float4*>(reinterpret_cast<char*>(p.plane) + (size_t)y * p.plane_pitch + (size_t)x * 16) = g;
}

__global__ __launch_bounds__(NT) void k_metrics_finalize(const MetricsPartial* __restrict__ slab, uint32_t n,
                                                         MetricsRecord* __restrict__ record, uint32_t width, uint32_t height,
                                                         uint32_t flags) {
    __shared__ double s_a[NT], s_b[NT];
    __shared__ unsigned long long s_q[NT];
    const uint32_t tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    unsigned long long q = 0ull;
    for (uint32_t i = tid; i < n; i += NT) {
        a += slab[i].sse;
        b += slab[i].ssim_sum;
        q += slab[i].sse_u8;
    }
    s_a[tid] = a;
    s_b[tid] = b;
    s_q[tid] = q;
    __syncthreads();
    for (uint32_t s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_a[tid] += s_a[tid + s];
            s_b[tid] += s_b[tid + s];
            s_q[tid] += s_q[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        MetricsRecord r;
        r.sse = s_a[0];
        r.ssim_sum = s_b[0];
        r.sse_u8 = s_q[0];
        r.width = width;
        r.height = height;
        r.flags = flags;
        r.reserved = 0u;
        *record = r;
    }
}

}  // namespace

int launch_image_metrics(const MetricsParams& p, MetricsRecord* record, hipStream_t stream) {
    const uint32_t gx = (p.width + METRICS_TILE_W - 1) / METRICS_TILE_W, gy = (p.height + METRICS_TILE_H - 1) / METRICS_TILE_H;
    if (gx == 0 || gy == 0 || gy > 65535u) return fail(WS_ERR_INVALID, "launch_image_metrics: image size");
    typedef void (*Kernel)(const MetricsParams);
#define WS_METRICS_ROW(FA) \
    {k_image_metrics<FA, WS_FORMAT_RGBA8_UNORM>, k_image_metrics<FA, WS_FORMAT_RGBA16_FLOAT>, k_image_metrics<FA, WS_FORMAT_RGBA32_FLOAT>}
    static const Kernel kernels[3][3] = {WS_METRICS_ROW(WS_FORMAT_RGBA8_UNORM), WS_METRICS_ROW(WS_FORMAT_RGBA16_FLOAT),
                                         WS_METRICS_ROW(WS_FORMAT_RGBA32_FLOAT)};
#undef WS_METRICS_ROW
    if (p.a.format < 0 || p.a.format > 2 || p.b.format < 0 || p.b.format > 2) return fail(WS_ERR_INVALID, "launch_image_metrics: colour format");
    hipLaunchKernelGGL(kernels[p.a.format][p.b.format], dim3(gx, gy), dim3(NT), 0, stream, p);
    WS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_metrics_finalize, dim3(1), dim3(NT), 0, stream, p.slab, gx * gy, record, p.width, p.height, p.flags);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_image_error(const ImageErrorParams& p, hipStream_t stream) {
    const uint32_t gx = (p.width + EW - 1) / EW, gy = (p.height + EH - 1) / EH;
    if (gx == 0 || gy == 0 || gy > 65535u) return fail(WS_ERR_INVALID, "launch_image_error: image size");
    typedef void (*Kernel)(const ImageErrorParams);
#define WS_ERROR_ROW(K, FA) {K<FA, WS_FORMAT_RGBA8_UNORM>, K<FA, WS_FORMAT_RGBA16_FLOAT>, K<FA, WS_FORMAT_RGBA32_FLOAT>}
#define WS_ERROR_TABLE(K) {WS_ERROR_ROW(K, WS_FORMAT_RGBA8_UNORM), WS_ERROR_ROW(K, WS_FORMAT_RGBA16_FLOAT), WS_ERROR_ROW(K, WS_FORMAT_RGBA32_FLOAT)}
    static const Kernel kernels[2][3][3] = {WS_ERROR_TABLE(k_image_error), WS_ERROR_TABLE(k_image_error_grad)};
#undef WS_ERROR_TABLE
#undef WS_ERROR_ROW
    if (p.a.format < 0 || p.a.format > 2 || p.b.format < 0 || p.b.format > 2) return fail(WS_ERR_INVALID, "launch_image_error: colour format");
    hipLaunchKernelGGL(kernels[p.gradient ? 1 : 0][p.a.format][p.b.format], dim3(gx, gy), dim3(EW * EH), 0, stream, p);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
