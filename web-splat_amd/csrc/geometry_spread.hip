// geometry_spread.hip -- k_geom_spread: a frame's five screen-space sums per Gaussian (k_geometry's, in a ws_geomgrad's scratch)
// through K1's projection to dL/d position and dL/d covariance, added to the accumulator's f64 planes (include/websplat.h,
// "Geometry gradients"; geometry_spread.h has the chain to the bit).  Purely streaming: one thread per store slot
// of the prepared frame, no LDS, no atomics.  Every visible splat costs its source index and the 40 B of its Gaussian's scratch
// row; one whose row is not all zero also the 40 B written back, 8 B of its Splat record, the two 16-B chunks of its Gaussian and
// a read-modify-write of 8 B in each of the eleven planes.
//
// Compiled with -ffp-contract=off (Makefile STRICT): every f64 operation of geometry_spread.h is rounded by itself.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "geometry_spread.h"

namespace ws {

namespace {

__global__ __launch_bounds__(256) void k_geom_spread(const GeomSpreadParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n || i >= p.counters->num_visible) return;
    const uint32_t j = p.src_index[i];
    if (j >= p.n) return;  // (K1 writes source indices below its num_points: never taken)
    unsigned long long* row = p.scratch + (size_t)j * GEOM_SCRATCH;
    long long q[GEOM_SCRATCH];
    unsigned long long any = 0ull;
#pragma unroll
    for (int e = 0; e < GEOM_SCRATCH; ++e) {
        const unsigned long long u = row[e];
        q[e] = (long long)u;
        any |= u;
    }
    if (any == 0ull) return;  // nothing counted of this splat: the common case
#pragma unroll
    for (int e = 0; e < GEOM_SCRATCH; ++e) row[e] = 0ull;
    const char* sp = reinterpret_cast<const char*>(p.splats) + (size_t)i * SPLAT_STRIDE;
    uint2 w01;
    __builtin_memcpy(&w01, sp, 8);
    const uint16_t rec[4] = {(uint16_t)w01.x, (uint16_t)(w01.x >> 16), (uint16_t)w01.y, (uint16_t)(w01.y >> 16)};
    const uint4 c0 = p.planes[j], c1 = p.planes[(size_t)p.n + j];
    const float xyz[3] = {__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z)};
    const uint16_t cov[6] = {(uint16_t)c1.x, (uint16_t)(c1.x >> 16), (uint16_t)c1.y, (uint16_t)(c1.y >> 16), (uint16_t)c1.z, (uint16_t)(c1.z >> 16)};
    GeomSpreadRow r;
    geom_spread_row(q, rec, xyz, cov, p.frame, &r);
    const size_t n = p.n;
    double* s = reinterpret_cast<double*>(p.sums) + j;  // element e of this Gaussian: s[e * n]
#pragma unroll
    for (int k = 0; k < 3; ++k) s[(size_t)k * n] += r.position[k];
#pragma unroll
    for (int e = 0; e < 6; ++e) s[(size_t)(3 + e) * n] += r.covariance[e];
    s[(size_t)9 * n] += r.norm;
    p.sums[(size_t)10 * n + j] += 1ull;
}

__global__ __launch_bounds__(256) void k_geom_merge(unsigned long long* sums, const unsigned long long* other, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double* s = reinterpret_cast<double*>(sums);
    const double* o = reinterpret_cast<const double*>(other);
#pragma unroll
    for (int e = 0; e < GEOM_ELEMENTS - 1; ++e) s[(size_t)e * n + i] += o[(size_t)e * n + i];
    sums[(size_t)(GEOM_ELEMENTS - 1) * n + i] += other[(size_t)(GEOM_ELEMENTS - 1) * n + i];
}

}  // namespace

int launch_geom_spread(const GeomSpreadParams& p, hipStream_t stream) {
    if (p.n == 0) return WS_OK;
    hipLaunchKernelGGL(k_geom_spread, dim3((p.n + 255u) / 256u), dim3(256), 0, stream, p);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

int launch_geom_merge(unsigned long long* sums, const unsigned long long* other, uint32_t n, hipStream_t stream) {
    if (n == 0) return WS_OK;
    hipLaunchKernelGGL(k_geom_merge, dim3((n + 255u) / 256u), dim3(256), 0, stream, sums, other, n);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
