// sh_gradient.hip -- k_sh_spread: a frame's four ws_grad-layout sums per Gaussian spread over the SH coefficients of a ws_shgrad
// (include/websplat.h, "SH gradients"; sh_gradient.h has the step to the bit).  Purely streaming: one thread per
// Gaussian, no LDS, no atomics.  Every Gaussian costs the 32 B of its scratch row; one whose row is not all zero also the 32 B
// written back, the 16 B of its plane-0 chunk and a read-modify-write of 8 B in each of the planes the frame's degree touches
// (16 B x (3 nact + 1)), every wave access contiguous in the Gaussian index.
//
// Compiled with -ffp-contract=off (Makefile STRICT): every f32 operation of sh_gradient.h is rounded by itself.
#include <hip/hip_runtime.h>

#include "sh_gradient.h"

namespace ws {

namespace {

__global__ __launch_bounds__(256) void k_sh_spread(const ShSpreadParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    ulonglong2* row = reinterpret_cast<ulonglong2*>(p.scratch) + (size_t)i * 2;
    const ulonglong2 q01 = row[0], q23 = row[1];
    if ((q01.x | q01.y | q23.x | q23.y) == 0ull) return;  // culled or unseen: the common case
    row[0] = make_ulonglong2(0ull, 0ull);
    row[1] = make_ulonglong2(0ull, 0ull);
    const size_t n = p.n;
    unsigned long long* s = p.sums + i;  // element e of this Gaussian: s[e * n]
    s[(size_t)(3u * p.ncoef) * n] += q23.y;
    const long long q[3] = {(long long)q01.x, (long long)q01.y, (long long)q23.x};
    s[0] += q01.x;
    s[n] += q01.y;
    s[2 * n] += q23.x;
    if (p.nact <= 1u) return;
    const uint4 c0 = p.planes[i];
    float dir[3], bas[SH_MAX_COEFS];
    sh_spread_dir(__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z), p.cam, dir);
    sh_spread_basis(dir[0], dir[1], dir[2], bas);
#pragma unroll
    for (uint32_t k = 1; k < SH_MAX_COEFS; ++k) {
        if (k < p.nact) {  // (nact is 4, 9 or 16: uniform over the launch)
#pragma unroll
            for (uint32_t ch = 0; ch < 3; ++ch) s[(size_t)(3u * k + ch) * n] += (unsigned long long)sh_spread_term(q[ch], bas[k]);
        }
    }
}

}  // namespace

int launch_sh_spread(const ShSpreadParams& p, hipStream_t stream) {
    if (p.n == 0) return WS_OK;
    hipLaunchKernelGGL(k_sh_spread, dim3((p.n + 255u) / 256u), dim3(256), 0, stream, p);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
