// sh_gradient.h -- one frame's colour sums of a Gaussian spread over its SH coefficients: dL/d sh[k][ch] = basis_k(dir) * dL/d colour[ch]
// (sh_gradient.hip k_sh_spread behind removal.hip's k_removal_base and gradient.hip's k_gradient).  Internal: the ABI is
// include/websplat.h, "SH gradients"; DESIGN.md 3.4m.
//
// One definition for the kernel and for the host twin (host_math.cpp, ws_sh_spread_rows): the functions below are compiled for both
// sides from this text, without contraction, and use only f32 + - x / sqrt, one f64 multiply, two conversions and comparisons --
// all correctly rounded IEEE operations on both sides, so everything here agrees bit for bit between host and device.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ws_internal.h"

namespace ws {

constexpr uint32_t SH_MAX_COEFS = 16;  // degree 3

// K1's constants (preprocess.hip, preprocess.wgsl:4-23)
constexpr float SHG_C1 = 0.4886025119029199f;
constexpr float SHG_C2_0 = 1.0925484305920792f, SHG_C2_1 = -1.0925484305920792f, SHG_C2_2 = 0.31539156525252005f,
                SHG_C2_3 = -1.0925484305920792f, SHG_C2_4 = 0.5462742152960396f;
constexpr float SHG_C3_0 = -0.5900435899266435f, SHG_C3_1 = 2.890611442640554f, SHG_C3_2 = -0.4570457994644658f,
                SHG_C3_3 = 0.3731763325901154f, SHG_C3_4 = -0.4570457994644658f, SHG_C3_5 = 1.445305721320277f,
                SHG_C3_6 = -0.5900435899266435f;

// The view direction K1 evaluates the SH at: d = xyz - cam, dl = sqrtf((dx dx + dy dy) + dz dz), dir = d / dl; every operation a
// separately rounded IEEE f32 operation.  This is K1's default (strict) path, NOT its fast rsq path (WS_K1_STRICT=0), which is
// within an ulp or two of it.  dl == 0 and a non-finite xyz give NaN components: every basis is then not finite and adds nothing.
__host__ __device__ inline void sh_spread_dir(float x, float y, float z, const float cam[3], float dir[3]) {
    const float dx = x - cam[0], dy = y - cam[1], dz = z - cam[2];
    const float dl = sqrtf((dx * dx + dy * dy) + dz * dz);
    dir[0] = dx / dl;
    dir[1] = dy / dl;
    dir[2] = dz / dl;
}

// bas[1..15]: the expressions of preprocess.hip's eval_sh3 in its order; bas[3] is NEGATED, since K1 subtracts that term: these
// are the effective factors, colour = max(0, 0.5 + C0 sh[0] + sum_k bas[k] sh[k]).  bas[0] is not written: coefficient 0 takes the
// plain colour sum (the factor C0 stays in the refit step).  |bas[k]| <= 1 on unit directions.
__host__ __device__ inline void sh_spread_basis(float x, float y, float z, float bas[SH_MAX_COEFS]) {
    bas[1] = -SHG_C1 * y;
    bas[2] = SHG_C1 * z;
    bas[3] = -(SHG_C1 * x);
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, yz = y * z, xz = x * z;
    bas[4] = SHG_C2_0 * xy;
    bas[5] = SHG_C2_1 * yz;
    bas[6] = SHG_C2_2 * (2.0f * zz - xx - yy);
    bas[7] = SHG_C2_3 * xz;
    bas[8] = SHG_C2_4 * (xx - yy);
    bas[9] = SHG_C3_0 * y * (3.0f * xx - yy);
    bas[10] = SHG_C3_1 * xy * z;
    bas[11] = SHG_C3_2 * y * (4.0f * zz - xx - yy);
    bas[12] = SHG_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    bas[13] = SHG_C3_4 * x * (4.0f * zz - xx - yy);
    bas[14] = SHG_C3_5 * z * (xx - yy);
    bas[15] = SHG_C3_6 * x * (xx - 3.0f * yy);
}

// What one colour sum adds to the sum of a coefficient: llrint((double)q * (double)basis) -- int64 -> double, the product and
// double -> int64 each round to nearest even.  q == 0 and a basis that is not finite add nothing.  (|q * basis| < 2^63 as long as
// |q| is: |basis| <= 1 on unit directions.)
__host__ __device__ inline long long sh_spread_term(long long q, float basis) {
    if (q == 0 || !(fabsf(basis) <= 3.402823466e+38f)) return 0;
    return llrint((double)q * (double)basis);
}

// Coefficients a frame prepared with max_sh_deg touches on a cloud of degree sh_deg
inline uint32_t sh_active_coefs(uint32_t max_sh_deg, uint32_t sh_deg) {
    const uint32_t d = max_sh_deg < sh_deg ? max_sh_deg : sh_deg;
    return (d + 1u) * (d + 1u);
}

// One launch behind k_gradient on the same stream.  sums: one plane per element, [3 ncoef + 1][n] int64 -- element 3 k + ch is
// sh[k][ch], element 3 ncoef the opacity --, so that a wave's accesses are contiguous in the Gaussian index.
struct ShSpreadParams {
    const uint4* planes;           // the cloud's plane 0: x, y, z as f32 in the first 12 bytes of Gaussian i's chunk
    unsigned long long* scratch;   // [n][GRAD_CHANNELS]: this frame's ws_grad-layout sums; the rows read non-zero are zeroed again
    unsigned long long* sums;      // [3 ncoef + 1][n]
    uint32_t n;
    uint32_t ncoef;                // (sh_deg + 1)^2 of the accumulator
    uint32_t nact;                 // sh_active_coefs of the prepared frame: coefficients nact .. ncoef - 1 are not touched
    float cam[3];                  // view_inv[12..14] of the prepared frame's ws_camera_uniform
};

// TO THE BIT, one thread per Gaussian j, no atomics (a Gaussian belongs to one thread; frames are ordered by the stream):
//   q_r, q_g, q_b, q_o = scratch[j][0..3], two 16-B loads; all four 0: return, nothing else of j is read or written
//   scratch[j] = 0 (the next frame starts clean without a memset)
//   opacity[j] += q_o;   sh[j][0][ch] += q_ch
//   nact > 1:  dir = sh_spread_dir(xyz of plane 0, cam);  bas = sh_spread_basis(dir)
//              sh[j][k][ch] += sh_spread_term(q_ch, bas[k])      1 <= k < nact
// The clamp at 0 is honoured already: k_gradient counts no pair whose staged c_ch is 0.
// (The transposes between these planes and the ABI's per-Gaussian rows are the host's: ws_shgrad_download, ws_shgrad_add.)
int launch_sh_spread(const ShSpreadParams& p, hipStream_t stream);

}  // namespace ws
