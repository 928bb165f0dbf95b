// refit.h -- Adam steps on the DC colour and the opacity of a resident, uncompressed cloud (refit.hip k_refit_init, k_refit_step).
// Internal: the ABI is include/websplat.h, "Refitting colour and opacity"; DESIGN.md 3.4j.
#pragma once

#include <cstddef>

#include "ws_internal.h"

namespace ws {

constexpr float REFIT_C0 = 0.28209479177387814f;  // SH_C0 of K1: colour = max(0, 0.5 + C0 * dc + ...)
constexpr double REFIT_C0_F64 = 0.28209479177387814;
constexpr float REFIT_DC_MAX = 65504.0f;          // the largest finite f16: the clamp of the DC masters

// One step over every Gaussian.  The four parameters of Gaussian i, indexed like GRAD_CHANNELS: x[0..2] = the DC triple, the
// first three halves of plane 2's chunk; x[3] = the opacity, the low half of word 3 of plane 0's chunk.
struct RefitParams {
    uint4* planes;                   // the cloud's PC_PLANES planes of n 16-B chunks
    const unsigned long long* sums;  // [n][4] two's-complement q32 sums (ws_grad)
    float4* master;                  // [n] f32 masters
    float4* m;                       // [n] first moments
    float4* v;                       // [n] second moments
    uint32_t n;
    float lr_colour, lr_opacity;     // 0 freezes the group
    float beta1, beta2, omb1, omb2;  // omb = 1.0f - beta, in f32
    float bc1, bc2;                  // (float)(1.0 - beta^steps), the powers kept in double on the host
    float eps, opacity_min;
    double u_colour, u_opacity;      // what one unit of a sum is worth: colour_unit * C0, opacity_unit
};

// TO THE BIT, one thread per Gaussian, per channel k of a group whose rate is not 0 (x, m, v the stored f32 values):
//   g  = (float)((double)(int64_t)q[k] * u)      u = u_colour for k < 3, u_opacity for k = 3; both conversions round to nearest even
//   k = 3:  g = (x == 0) ? 0 : g / x
//   m' = (beta1 * m) + (omb1 * g);   v' = (beta2 * v) + (omb2 * (g * g))
//   s  = (m' / bc1) / (sqrtf(v' / bc2) + eps);   x' = x - (lr * s)
//   k < 3:  x' < -65504 -> -65504, x' > 65504 -> 65504        k = 3:  x' < opacity_min -> opacity_min, x' > 1 -> 1
// every operation a separately rounded IEEE f32 operation (the file is compiled without contraction; division and square root are
// correctly rounded).  x', m', v' are stored, and f16(x'), round to nearest even, into the four halves of the planes.  A frozen
// group's masters, moments and halves are not written.  No other byte of the planes changes: the opacity's word keeps its upper
// half (the loader's padding), the second DC word its upper half (the first half of SH coefficient 1).
// THE EDGES (include/websplat.h has them in full; tests/test_gpu_refit_edges.py holds the kernels to them): denormals are honoured
// in every operation and in both conversions (the file must never be built with a flush-to-zero mode or a fast divide / square
// root); a NaN passes clamp_to -- both of its comparisons are false -- and is stored as a NaN half; +-inf masters are clamped.
// g * g = inf with g finite leaves v' = inf, s = 0 and the parameter unmoved for good; g = +-inf leaves m' = +-inf, s = NaN and a NaN
// master.  Neither can occur while |q * u| < 2^63, for the opacity |q * u / x| < 2^63; nothing here enforces that bound.
int launch_refit_step(const RefitParams& p, hipStream_t stream);

// master[i] = the four halves widened to f32, m[i] = v[i] = 0
int launch_refit_init(const uint4* planes, uint32_t n, float4* master, float4* m, float4* v, hipStream_t stream);

// ---- the rest coefficients (include/websplat.h "SH gradients", ws_refit_step_sh) ----
// Element e = 3 coef + ch of the 96-B SH record is half e % 8 of plane 2 + e / 8.  The planes a cloud of ncoef coefficients needs:
// 1, 2, 4, 6 at degrees 0 .. 3; the last one ends in 5, 4, 5, 0 halves of padding that no step writes.
inline uint32_t refit_sh_planes(uint32_t ncoef) { return (3u * ncoef + 7u) / 8u; }

// One step over every Gaussian from a ws_shgrad's sums.  base.sums is not read: the DC triple takes elements 0 .. 2 of sh_sums, the
// opacity element 3 ncoef.
struct RefitShParams {
    RefitParams base;
    const unsigned long long* sh_sums;  // [3 ncoef + 1][n] two's-complement q32 sums, one plane per element (sh_gradient.h)
    float* sh_master;                   // [3 (ncoef - 1)][n] f32 masters of the rest elements, plane e - 3 for element e;
    float* sh_m;                        //   nullptr with ncoef == 1
    float* sh_v;
    uint32_t ncoef;
    float lr_sh;                        // 0 freezes the rest group
    double u_sh;                        // colour_unit: no C0 here, the basis is in the sum already
};

// TO THE BIT.  k_refit_step_sh, one thread per (Gaussian, SH plane), grid (ceil(n / 256), refit_sh_planes(ncoef)), or one row of
// blocks when lr_sh == 0.  The thread of plane 2 takes channels 0 .. 3 exactly as launch_refit_step does.  A rest element e of a
// group whose rate is not 0 takes the same step with g = (float)((double)(int64_t)q[e] * u_sh), lr = lr_sh and the clamp +-65504;
// x', m', v' go to plane e - 3 of the three arrays, f16(x') to its half.  Each thread loads its 16-B chunk once and, if it stepped
// any of its halves, stores it once as a whole: the halves it did not step (a frozen group's; the first half of coefficient 1
// beside a moving DC; the padding) go back with the bits they were read with -- as integers, never through a float: a signalling
// NaN there stays signalling.  No 2-byte store, no scratch.  The edges of the step above hold for the rest elements word for word.
int launch_refit_step_sh(const RefitShParams& p, hipStream_t stream);

// master[e - 3][i] = half e of Gaussian i widened to f32, m = v = 0, for 3 <= e < 3 ncoef
int launch_refit_init_sh(const uint4* planes, uint32_t n, uint32_t ncoef, float* master, float* m, float* v, hipStream_t stream);

}  // namespace ws
