// ply_encode.hip -- the resident 8-plane scene layout -> raw INRIA 3DGS PLY vertex rows, on the GPU: k_ply_decode run backwards.
//
// One thread per Gaussian reads its eight 16-B chunks (coalesced: plane p of Gaussian i sits at planes[p * n + i]), works out the
// row (ply_encode.h: positions and SH halves pass through, the opacity becomes a logit, the covariance an eigen-decomposition:
// three log-scales and a quaternion) and writes it into the block's LDS staging; the block then stores its 128 rows as one
// contiguous run (128 x 248 B at SH degree 3), the decode kernel's staging in the other direction.
//
// Arithmetic: f64, + - x / sqrt only, no contraction (this file is compiled with -ffp-contract=off, like the host twin
// ws_ply_rows_encode in host_math.cpp): bit-identical to the host twin in every column but the four that take a logarithm
// (opacity, scale_0..2), where the two log() implementations may differ in the last bit of the f32 they are rounded to.
#include <hip/hip_runtime.h>

#include "ply_encode.h"
#include "ws_internal.h"

namespace ws {

namespace {

constexpr int PLY_ROWS_PER_BLOCK = 128;

__device__ __forceinline__ float term_value(const PlyLogTerm& t, double scale) {
    return t.take_log ? (float)(scale * log(t.arg)) : (float)t.constant;
}

__global__ __launch_bounds__(PLY_ROWS_PER_BLOCK) void k_ply_encode(const uint4* __restrict__ planes, uint32_t n, uint32_t num_coefs,
                                                                  uint32_t row_len, float* __restrict__ rows) {
    extern __shared__ float s_rows[];  // PLY_ROWS_PER_BLOCK x row_len: the block's rows, stored as one contiguous run
    const uint32_t first = blockIdx.x * PLY_ROWS_PER_BLOCK;
    const uint32_t count = (n - first) < (uint32_t)PLY_ROWS_PER_BLOCK ? (n - first) : (uint32_t)PLY_ROWS_PER_BLOCK;
    if (threadIdx.x < count) {
        const uint32_t i = first + threadIdx.x;
        float* r = s_rows + (size_t)threadIdx.x * row_len;  // x y z | nx ny nz | f_dc[3] | f_rest[3][C-1] | opacity | scale[3] | rot[4]
        float* tail = r + (row_len - 8u);
        const uint4 p0 = planes[(size_t)0 * n + i];  // x, y, z, opacity f16 | pad
        const uint4 p1 = planes[(size_t)1 * n + i];  // cov f16 x 6 | pad
        r[0] = __uint_as_float(p0.x);
        r[1] = __uint_as_float(p0.y);
        r[2] = __uint_as_float(p0.z);
        r[3] = r[4] = r[5] = 0.0f;
        // planes 2..7: [[f16; 3]; 16], coefficient-major -> f_dc, f_rest channel-major; coefficients above the degree are not written
        uint32_t hw[24];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const uint4 w = planes[(size_t)(2 + p) * n + i];
            hw[4 * p] = w.x;
            hw[4 * p + 1] = w.y;
            hw[4 * p + 2] = w.z;
            hw[4 * p + 3] = w.w;
        }
#pragma unroll
        for (int e = 0; e < 48; ++e) {
            const uint32_t c = e / 3, j = e % 3;
            if (c < num_coefs) r[ply_sh_column(c, j, num_coefs)] = ply_half_to_f32((hw[e / 2] >> (16 * (e & 1))) & 0xFFFFu);
        }
        tail[0] = term_value(ply_encode_opacity(p0.w & 0xFFFFu), 1.0);
        const PlyEncodedCov ec = ply_encode_cov(p1.x & 0xFFFFu, p1.x >> 16, p1.y & 0xFFFFu, p1.y >> 16, p1.z & 0xFFFFu, p1.z >> 16);
        tail[1] = term_value(ply_encode_extent(ec.l0), 0.5);
        tail[2] = term_value(ply_encode_extent(ec.l1), 0.5);
        tail[3] = term_value(ply_encode_extent(ec.l2), 0.5);
        tail[4] = ec.q0;
        tail[5] = ec.q1;
        tail[6] = ec.q2;
        tail[7] = ec.q3;
    }
    __syncthreads();
    const size_t base = (size_t)first * row_len;
    const uint32_t total = count * row_len;
    for (uint32_t k = threadIdx.x; k < total; k += PLY_ROWS_PER_BLOCK) rows[base + k] = s_rows[k];
}

}  // namespace

int launch_ply_encode(const uint4* d_planes, uint32_t n, uint32_t sh_deg, float* d_rows, hipStream_t stream) {
    if (n == 0) return WS_OK;
    const uint32_t num_coefs = (sh_deg + 1u) * (sh_deg + 1u);
    const uint32_t row_len = 14u + 3u * num_coefs;
    const uint32_t blocks = (n + PLY_ROWS_PER_BLOCK - 1) / PLY_ROWS_PER_BLOCK;
    const size_t lds = (size_t)PLY_ROWS_PER_BLOCK * row_len * sizeof(float);
    hipLaunchKernelGGL(k_ply_encode, dim3(blocks), dim3(PLY_ROWS_PER_BLOCK), lds, stream, d_planes, n, num_coefs, row_len, d_rows);
    WS_HIP(hipGetLastError());
    return WS_OK;
}

}  // namespace ws
