// ply_encode.h -- one resident Gaussian back to the tail of an INRIA 3DGS PLY row: opacity logit, three log-scales, a quaternion.
// The inverse of k_ply_decode's per-vertex work.  Internal: the ABI is include/websplat.h, "Saving a point cloud"; DESIGN.md 3.4l.
//
// One definition for the kernel (ply_encode.hip, k_ply_encode) and for the host twin (host_math.cpp, ws_ply_rows_encode): the
// functions below are compiled for both sides from this text, without contraction, and use only f64 + - x / sqrt, comparisons
// and integer operations -- all correctly rounded IEEE operations on both sides, so everything here agrees bit for bit between
// host and device.  The two logarithms are the one thing that is not an IEEE operation: the callers take them (PlyLogTerm).
#pragma once

#include <stdint.h>

#include "ws_internal.h"

namespace ws {

constexpr int PLY_ENCODE_MAX_SWEEPS = 16;      // cyclic Jacobi sweeps at most; a 3 x 3 matrix is diagonal after 6 to 8
constexpr double PLY_ENCODE_FLOOR = -20.0;     // log-scale of a zero or negative extent, logit of an opacity <= 0: exp(-20)^2 is 0 in f16,
constexpr double PLY_ENCODE_CEIL = 20.0;       // sigmoid(-20) rounds to the half 0 and sigmoid(20) to the half 1
constexpr double PLY_ENCODE_HALF_MAX = 65504.0;

// A binary16 bit pattern as the f32 of the same value, by integer operations alone (a NaN keeps its sign and its payload, shifted).
__host__ __device__ inline uint32_t ply_half_to_f32_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1Fu;
    uint32_t m = h & 0x3FFu;
    if (e == 0x1Fu) return sign | 0x7F800000u | (m << 13);
    if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0u) return sign;
    uint32_t ee = 113u;  // a subnormal half: shift the leading one up to bit 10
    while (!(m & 0x400u)) {
        m <<= 1;
        --ee;
    }
    return sign | (ee << 23) | ((m & 0x3FFu) << 13);
}

__host__ __device__ inline float ply_half_to_f32(uint32_t h) {
    union {
        uint32_t u;
        float f;
    } v;
    v.u = ply_half_to_f32_bits(h);
    return v.f;
}

__host__ __device__ inline bool ply_half_finite(uint32_t h) { return (h & 0x7C00u) != 0x7C00u; }

// What is left to the caller's logarithm: value = (float)(scale * log(arg)) when take_log, else (float)constant.
struct PlyLogTerm {
    double arg;      // > 0 and finite when take_log
    double constant;
    bool take_log;
};

// opacity half -> logit.  0 < o < 1: log(o / (1 - o)); o <= 0 (-0 included): -20; o >= 1: +20 (o > 1 is written as 1: the one
// lossy case); NaN: NaN.
__host__ __device__ inline PlyLogTerm ply_encode_opacity(uint32_t half) {
    const double o = (double)ply_half_to_f32(half);
    PlyLogTerm t;
    t.take_log = false;
    t.arg = 1.0;
    if (o != o) t.constant = o;
    else if (o <= 0.0) t.constant = PLY_ENCODE_FLOOR;
    else if (o >= 1.0) t.constant = PLY_ENCODE_CEIL;
    else {
        t.take_log = true;
        t.arg = o / (1.0 - o);
        t.constant = 0.0;
    }
    return t;
}

// an eigenvalue -> log-scale: 0.5 * log(l) for l > 0, -20 otherwise
__host__ __device__ inline PlyLogTerm ply_encode_extent(double l) {
    PlyLogTerm t;
    t.take_log = l > 0.0;
    t.arg = t.take_log ? l : 1.0;
    t.constant = PLY_ENCODE_FLOOR;
    return t;
}

// One Jacobi rotation in the (p, q) plane: app, aqq the two diagonal entries, apq the entry to annihilate, arp, arq the entries
// that couple p and q to the third index r; vXp, vXq the two columns of the eigenvector matrix.  Numerical Recipes' form
// (tau = s / (1 + c)), which never subtracts nearly equal quantities.
#define WS_PLY_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                      \
    do {                                                                                          \
        const double g_ = 100.0 * fabs(apq);                                                      \
        if (apq != 0.0) {                                                                         \
            if (fabs(app) + g_ == fabs(app) && fabs(aqq) + g_ == fabs(aqq)) {                     \
                apq = 0.0; /* too small to move either diagonal entry by one part in 2^52 */      \
            } else {                                                                              \
                const double h_ = aqq - app;                                                      \
                double t_;                                                                        \
                if (fabs(h_) + g_ == fabs(h_)) {                                                  \
                    t_ = apq / h_;                                                                \
                } else {                                                                          \
                    const double theta_ = 0.5 * h_ / apq;                                         \
                    t_ = 1.0 / (fabs(theta_) + sqrt(1.0 + theta_ * theta_));                      \
                    if (theta_ < 0.0) t_ = -t_;                                                   \
                }                                                                                 \
                const double c_ = 1.0 / sqrt(1.0 + t_ * t_);                                      \
                const double s_ = t_ * c_;                                                        \
                const double tau_ = s_ / (1.0 + c_);                                              \
                const double d_ = t_ * apq;                                                       \
                app = app - d_;                                                                   \
                aqq = aqq + d_;                                                                   \
                apq = 0.0;                                                                        \
                const double rp_ = arp, rq_ = arq;                                                \
                arp = rp_ - s_ * (rq_ + rp_ * tau_);                                              \
                arq = rq_ + s_ * (rp_ - rq_ * tau_);                                              \
                const double a0_ = v0p, b0_ = v0q, a1_ = v1p, b1_ = v1q, a2_ = v2p, b2_ = v2q;    \
                v0p = a0_ - s_ * (b0_ + a0_ * tau_);                                              \
                v0q = b0_ + s_ * (a0_ - b0_ * tau_);                                              \
                v1p = a1_ - s_ * (b1_ + a1_ * tau_);                                              \
                v1q = b1_ + s_ * (a1_ - b1_ * tau_);                                              \
                v2p = a2_ - s_ * (b2_ + a2_ * tau_);                                              \
                v2q = b2_ + s_ * (a2_ - b2_ * tau_);                                              \
            }                                                                                     \
        }                                                                                         \
    } while (0)

// The six covariance halves (c00 c01 c02 c11 c12 c22) -> three eigenvalues and a unit quaternion (scalar first, f32).
//   * any half not finite: identity quaternion, the "eigenvalues" are the diagonal as it stands with +inf taken as 65504 (the
//     largest finite half) and NaN / -inf as 0 (which ply_encode_extent writes as -20): a finite, deterministic row.
//   * else cyclic Jacobi in f64 on the widened halves: pairs in the order (0,1), (0,2), (1,2), at most PLY_ENCODE_MAX_SWEEPS sweeps,
//     ended when the three off-diagonal entries are exactly 0.  THE ORDER: eigenvalue k is entry k of the diagonal the sweeps end
//     with, eigenvector k column k of the accumulated rotations -- nothing is sorted.  A product of plane rotations is a proper
//     rotation (det = +1), C = R diag(l) R^T, and a covariance that is diagonal already keeps R = I: it is written with the identity
//     quaternion and comes back exactly (sorting would turn it by 90 degrees, which f32 quaternion components cannot express exactly).
//   * quaternion by the largest pivot among trace, R00, R11, R22 (the first of equals in that order), normalised in f64, negated
//     as a whole when its scalar part is negative, a scalar part of -0 written as +0, each component rounded once to f32.
struct PlyEncodedCov {
    double l0, l1, l2;      // eigenvalues in the order of the final diagonal (the diagonal as it stands for a covariance that is not finite)
    float q0, q1, q2, q3;   // unit quaternion, scalar first, q0 >= 0
};

// a diagonal entry of a covariance that is not finite, as the extent it is written with
__host__ __device__ inline double ply_diag_extent(double d) {
    return d != d ? 0.0 : (d > PLY_ENCODE_HALF_MAX ? PLY_ENCODE_HALF_MAX : (d < 0.0 ? 0.0 : d));
}

__host__ __device__ inline PlyEncodedCov ply_encode_cov(uint32_t h00, uint32_t h01, uint32_t h02, uint32_t h11, uint32_t h12, uint32_t h22) {
    const bool finite = ply_half_finite(h00) && ply_half_finite(h01) && ply_half_finite(h02) && ply_half_finite(h11) &&
                        ply_half_finite(h12) && ply_half_finite(h22);
    double a00 = (double)ply_half_to_f32(h00), a01 = (double)ply_half_to_f32(h01), a02 = (double)ply_half_to_f32(h02);
    double a11 = (double)ply_half_to_f32(h11), a12 = (double)ply_half_to_f32(h12), a22 = (double)ply_half_to_f32(h22);
    PlyEncodedCov out;
    if (!finite) {
        out.l0 = ply_diag_extent(a00);
        out.l1 = ply_diag_extent(a11);
        out.l2 = ply_diag_extent(a22);
        out.q0 = 1.0f;
        out.q1 = out.q2 = out.q3 = 0.0f;
        return out;
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;  // vRC: row R, column C
    for (int sweep = 0; sweep < PLY_ENCODE_MAX_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        WS_PLY_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (p, q) = (0, 1), r = 2
        WS_PLY_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
        WS_PLY_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
    }
    out.l0 = a00;
    out.l1 = a11;
    out.l2 = a22;
    // R = (vRC): Shepperd's four candidates, each 4 q_k q
    const double tr = v00 + v11 + v22;
    double q0, q1, q2, q3;
    if (tr >= v00 && tr >= v11 && tr >= v22) {
        q0 = 1.0 + tr;
        q1 = v21 - v12;
        q2 = v02 - v20;
        q3 = v10 - v01;
    } else if (v00 >= v11 && v00 >= v22) {
        q0 = v21 - v12;
        q1 = 1.0 + v00 - v11 - v22;
        q2 = v01 + v10;
        q3 = v02 + v20;
    } else if (v11 >= v22) {
        q0 = v02 - v20;
        q1 = v01 + v10;
        q2 = 1.0 - v00 + v11 - v22;
        q3 = v12 + v21;
    } else {
        q0 = v10 - v01;
        q1 = v02 + v20;
        q2 = v12 + v21;
        q3 = 1.0 - v00 - v11 + v22;
    }
    const double inv = 1.0 / sqrt(q0 * q0 + (q1 * q1 + q2 * q2 + q3 * q3));
    q0 = q0 * inv;
    q1 = q1 * inv;
    q2 = q2 * inv;
    q3 = q3 * inv;
    if (q0 < 0.0) {
        q0 = -q0;
        q1 = -q1;
        q2 = -q2;
        q3 = -q3;
    }
    if (q0 == 0.0) q0 = 0.0;
    out.q0 = (float)q0;
    out.q1 = (float)q1;
    out.q2 = (float)q2;
    out.q3 = (float)q3;
    return out;
}

#undef WS_PLY_ROTATE

// The column of coefficient c (0 .. num_coefs - 1), channel j in a row: f_dc at 6 .. 8, f_rest channel-major [3][C-1] behind it.
__host__ __device__ inline uint32_t ply_sh_column(uint32_t c, uint32_t j, uint32_t num_coefs) {
    return c == 0u ? 6u + j : 9u + j * (num_coefs - 1u) + (c - 1u);
}

// d_planes: the resident PC_PLANES x n x 16 B; d_rows: n x (14 + 3 (sh_deg + 1)^2) f32 in device memory
int launch_ply_encode(const uint4* d_planes, uint32_t n, uint32_t sh_deg, float* d_rows, hipStream_t stream);

}  // namespace ws
