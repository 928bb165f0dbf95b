// geometry_spread.h -- one frame's five screen-space sums of a Gaussian (geometry.h) taken through K1's projection to its world
// position and its 3-D covariance (geometry_spread.hip k_geom_spread behind removal.hip's k_removal_base and geometry.hip's
// k_geometry).  Internal: the ABI is include/websplat.h, "Geometry gradients"; DESIGN.md 3.4n.
//
// One definition for the kernel and for the host twin (host_math.cpp, ws_geom_spread_rows): geom_spread_row below is compiled for
// both sides from this text, without contraction, and uses only f64 + - x / sqrt, exact conversions (f16 -> f32 -> f64, int64 ->
// f64 of sums below 2^53 -- larger ones round to nearest even on both sides) and comparisons: all correctly rounded IEEE
// operations on both sides, so everything here agrees bit for bit between host and device.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ws_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#endif
#include "blend_stage.h"

namespace ws {

constexpr int GEOM_SCRATCH = 5;    // m0, m1, S00, S01, S11: the scratch row of a Gaussian (accum_s32.h GEOM_CHANNELS)
constexpr int GEOM_ELEMENTS = 11;  // planes of a ws_geomgrad: position x y z, covariance xx xy xz yy yz zz, screen_norm (f64); seen (uint64)
constexpr double GEOM_LN2 = 0.6931471805599453;
constexpr double GEOM_SQRT_LOG2E = 1.2011224087864498;
constexpr double GEOM_LAMBDA2_MIN = 0.100000001490116119384765625;  // K1's f32 literal 0.1f, as the f64 it is

#if defined(__HIPCC__)
#define WS_GHD __host__ __device__ inline
#else
#define WS_GHD inline
#endif

// What the chain reads of the prepared frame: K1's two uniforms and the scale of the scratch sums.
struct GeomSpreadFrame {
    ws_camera_uniform cam;
    ws_settings_uniform rs;
    float geometry_scale;
    uint32_t _pad[3];
};

struct GeomSpreadRow {
    double position[3];    // dL/d(world x, y, z)
    double covariance[6];  // dL/d(the six STORED elements xx xy xz yy yz zz): an off-diagonal is twice the symmetric matrix's entry
    double norm;           // |dL/d(NDC centre)|
};

// q: the five scratch sums; rec: the Splat record's halves 0..3 (v1.x, v1.y, v2.x, v2.y) as f16 bits; xyz: the cloud's f32
// position; cov: the cloud's six f16 covariance halves (xx xy xz yy yz zz) as bits.
//
//   1. I' by stage::decode's expressions in f64:  M = [v1.x W, v2.x W; -v1.y H, -v2.y H],  I' = sqrt(log2 e) M^-1
//        m, S = q / (2^32 geometry_scale)
//        dmu = -2 ln2 I'^T m                       (pixels, x right, y DOWN)
//        D   = -2 (ln2)^2 I'^T S I'                (the same frame)
//      K1 forms its 2-D covariance with y UP (its Jacobian's second row is negated; decode negates v.y back): D_K = diag(1, -1) D
//      diag(1, -1), the off-diagonal's sign flipped, is dL/d(K1's cov2d).
//   2. cs = view (xyz, 1), clip = proj cs, w = clip[3];  jac = [fx / cz, 0, -fx cx / cz^2; 0, -fy / cz, fy cy / cz^2];  T = jac
//      view3x3;  scaling^2 = (gaussian_scaling scale_mod)^2 with K1's fade-in scale_mod;  V = scaling^2 sym(cov);  cov2d = T V T^T;
//      lambda2_raw = mid - radius of cov2d + kernel_size I.
//   3. position, through the centre: the NDC gradient g = (W/2 dmu_x, -H/2 dmu_y); d clip = (g_x / w, g_y / w, ., -(g_x clip_x +
//      g_y clip_y) / w^2); back through proj and view.  Through the Jacobian (lambda2_raw >= 0.1 only): dL/dT = 2 D_K T V, on
//      through jac's four non-zero entries to cs, and with the centre's part to the world by view^T.
//   4. covariance (lambda2_raw >= 0.1 only): scaling^2 T^T D_K T, off-diagonals doubled.
//   5. norm = sqrt(g_x^2 + g_y^2).
// NOT differentiated: the colour's dependence on the view direction, the mip-splatting opacity factor's on Sigma, the fade-in
// scale_mod's on the position; the record's f16 rounding counts as the identity; a Gaussian whose lambda2_raw < 0.1 (or is NaN)
// has its minor axis on K1's clamp: it gets its centre path only.
WS_GHD void geom_spread_row(const long long q[GEOM_SCRATCH], const uint16_t rec[4], const float xyz[3], const uint16_t cov[6],
                            const GeomSpreadFrame& f, GeomSpreadRow* out) {
#pragma clang fp contract(off)
    const double W = (double)f.cam.viewport[0], H = (double)f.cam.viewport[1];
    // ---- 1
    const double v1x = (double)stage::half_bits(rec[0]), v1y = (double)stage::half_bits(rec[1]);
    const double v2x = (double)stage::half_bits(rec[2]), v2y = (double)stage::half_bits(rec[3]);
    const double m00 = v1x * W, m01 = v2x * W;
    const double m10 = -v1y * H, m11 = -v2y * H;
    const double det = m00 * m11 - m01 * m10;
    const double inv = GEOM_SQRT_LOG2E / det;
    const double i00 = m11 * inv, i01 = -m01 * inv, i10 = -m10 * inv, i11 = m00 * inv;
    const double unit = 4294967296.0 * (double)f.geometry_scale;
    const double m0 = (double)q[0] / unit, m1 = (double)q[1] / unit;
    const double S00 = (double)q[2] / unit, S01 = (double)q[3] / unit, S11 = (double)q[4] / unit;
    const double k1 = -2.0 * GEOM_LN2, k2 = -2.0 * (GEOM_LN2 * GEOM_LN2);
    const double dmux = k1 * (i00 * m0 + i10 * m1), dmuy = k1 * (i01 * m0 + i11 * m1);
    const double A00 = S00 * i00 + S01 * i10, A01 = S00 * i01 + S01 * i11;
    const double A10 = S01 * i00 + S11 * i10, A11 = S01 * i01 + S11 * i11;
    const double D00 = k2 * (i00 * A00 + i10 * A10);
    const double D01 = -(k2 * (i00 * A01 + i10 * A11));  // (D_K: y up)
    const double D11 = k2 * (i01 * A01 + i11 * A11);
    // ---- 2
    const float* vw = f.cam.view;  // column-major: vw[c * 4 + r]
    const float* pj = f.cam.proj;
    const double x = (double)xyz[0], y = (double)xyz[1], z = (double)xyz[2];
    double cs[4], clip[4];
    for (int r = 0; r < 4; ++r) cs[r] = (((double)vw[r] * x + (double)vw[4 + r] * y) + (double)vw[8 + r] * z) + (double)vw[12 + r];
    for (int r = 0; r < 4; ++r)
        clip[r] = (((double)pj[r] * cs[0] + (double)pj[4 + r] * cs[1]) + (double)pj[8 + r] * cs[2]) + (double)pj[12 + r] * cs[3];
    const double w = clip[3];
    const double fx = (double)f.cam.focal[0], fy = (double)f.cam.focal[1];
    const double cz = cs[2], cz2 = cz * cz;
    const double j00 = fx / cz, j02 = -(fx * cs[0]) / cz2, j11 = -fy / cz, j12 = (fy * cs[1]) / cz2;
    double R[3][3], T0[3], T1[3];  // R[r][k] = view3x3 [row r, column k]
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) R[r][k] = (double)vw[k * 4 + r];
    for (int k = 0; k < 3; ++k) {
        T0[k] = j00 * R[0][k] + j02 * R[2][k];
        T1[k] = j11 * R[1][k] + j12 * R[2][k];
    }
    const double ddx = (double)f.rs.scene_center[0] - x, ddy = (double)f.rs.scene_center[1] - y, ddz = (double)f.rs.scene_center[2] - z;
    const double dd = 5.0 * sqrt((ddx * ddx + ddy * ddy) + ddz * ddz) / (double)f.rs.scene_extend;
    const double wall = (double)f.rs.walltime;
    double scale_mod = 0.0;
    if (wall > dd) {
        double t = wall - dd;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        scale_mod = (t * t) * (3.0 - 2.0 * t);
    }
    const double scaling = (double)f.rs.gaussian_scaling * scale_mod;
    const double sc2 = scaling * scaling;
    double c6[6];
    for (int e = 0; e < 6; ++e) c6[e] = (double)stage::half_bits(cov[e]) * sc2;
    const double V[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    double TV0[3], TV1[3];
    for (int k = 0; k < 3; ++k) {
        TV0[k] = (T0[0] * V[0][k] + T0[1] * V[1][k]) + T0[2] * V[2][k];
        TV1[k] = (T1[0] * V[0][k] + T1[1] * V[1][k]) + T1[2] * V[2][k];
    }
    const double c00 = (TV0[0] * T0[0] + TV0[1] * T0[1]) + TV0[2] * T0[2];
    const double c01 = (TV0[0] * T1[0] + TV0[1] * T1[1]) + TV0[2] * T1[2];
    const double c11 = (TV1[0] * T1[0] + TV1[1] * T1[1]) + TV1[2] * T1[2];
    const double ks = (double)f.rs.kernel_size;
    const double d1 = c00 + ks, d2 = c11 + ks;
    const double mid = 0.5 * (d1 + d2), hx = (d1 - d2) / 2.0;
    const double lambda2_raw = mid - sqrt(hx * hx + c01 * c01);
    const bool free_axis = lambda2_raw >= GEOM_LAMBDA2_MIN;  // (a NaN is not)
    // ---- 3: the centre
    const double gx = (0.5 * W) * dmux, gy = -((0.5 * H) * dmuy);
    double dclip[4] = {gx / w, gy / w, 0.0, -((gx * clip[0] + gy * clip[1]) / (w * w))};
    double dcs[4];
    for (int c = 0; c < 4; ++c) dcs[c] = ((double)pj[c * 4] * dclip[0] + (double)pj[c * 4 + 1] * dclip[1]) + (double)pj[c * 4 + 3] * dclip[3];
    for (int e = 0; e < 6; ++e) out->covariance[e] = 0.0;
    if (free_axis) {
        // ---- 3: the Jacobian.  Gt = dL/dT = 2 D_K (T V)
        double Gt0[3], Gt1[3];
        for (int k = 0; k < 3; ++k) {
            Gt0[k] = 2.0 * (D00 * TV0[k] + D01 * TV1[k]);
            Gt1[k] = 2.0 * (D01 * TV0[k] + D11 * TV1[k]);
        }
        const double J00 = (Gt0[0] * R[0][0] + Gt0[1] * R[0][1]) + Gt0[2] * R[0][2];
        const double J02 = (Gt0[0] * R[2][0] + Gt0[1] * R[2][1]) + Gt0[2] * R[2][2];
        const double J11 = (Gt1[0] * R[1][0] + Gt1[1] * R[1][1]) + Gt1[2] * R[1][2];
        const double J12 = (Gt1[0] * R[2][0] + Gt1[1] * R[2][1]) + Gt1[2] * R[2][2];
        const double cz3 = cz2 * cz;
        dcs[0] = dcs[0] + J02 * (-fx / cz2);
        dcs[1] = dcs[1] + J12 * (fy / cz2);
        dcs[2] = dcs[2] + (((J00 * (-fx / cz2) + J02 * ((2.0 * (fx * cs[0])) / cz3)) + J11 * (fy / cz2)) + J12 * (-(2.0 * (fy * cs[1])) / cz3));
        // ---- 4
        double DT0[3], DT1[3];
        for (int k = 0; k < 3; ++k) {
            DT0[k] = D00 * T0[k] + D01 * T1[k];
            DT1[k] = D01 * T0[k] + D11 * T1[k];
        }
        const double g00 = sc2 * (T0[0] * DT0[0] + T1[0] * DT1[0]), g01 = sc2 * (T0[0] * DT0[1] + T1[0] * DT1[1]);
        const double g02 = sc2 * (T0[0] * DT0[2] + T1[0] * DT1[2]), g11 = sc2 * (T0[1] * DT0[1] + T1[1] * DT1[1]);
        const double g12 = sc2 * (T0[1] * DT0[2] + T1[1] * DT1[2]), g22 = sc2 * (T0[2] * DT0[2] + T1[2] * DT1[2]);
        out->covariance[0] = g00;
        out->covariance[1] = 2.0 * g01;
        out->covariance[2] = 2.0 * g02;
        out->covariance[3] = g11;
        out->covariance[4] = 2.0 * g12;
        out->covariance[5] = g22;
    }
    for (int k = 0; k < 3; ++k)
        out->position[k] = (((double)vw[k * 4] * dcs[0] + (double)vw[k * 4 + 1] * dcs[1]) + (double)vw[k * 4 + 2] * dcs[2]) + (double)vw[k * 4 + 3] * dcs[3];
    // ---- 5
    out->norm = sqrt(gx * gx + gy * gy);
}

// One launch behind k_geometry on the same stream.  sums: one plane per element, [GEOM_ELEMENTS][n] 64-bit words (ten f64, then
// the uint64 count), so that accesses are contiguous in the Gaussian index where the store slots are.
struct GeomSpreadParams {
    const uint4* planes;            // the cloud's planes 0 and 1 (ws_internal.h PC_PLANES): xyz f32; six f16 covariance halves
    const uint8_t* splats;          // the prepared frame's Splat records, [V] x SPLAT_STRIDE
    const uint32_t* src_index;      // [V] store slot -> Gaussian
    const FrameCounters* counters;  // num_visible of the prepared frame
    unsigned long long* scratch;    // [n][GEOM_SCRATCH]: this frame's sums; the rows read non-zero are zeroed again
    unsigned long long* sums;       // [GEOM_ELEMENTS][n]
    uint32_t n;                     // Gaussians of the cloud and of the accumulator
    uint32_t _pad;
    GeomSpreadFrame frame;
};

// TO THE BIT, one thread per store slot i of the prepared frame, no atomics, no LDS (a visible Gaussian has one slot, so it
// belongs to one thread; frames are ordered by the stream):
//   i >= num_visible: return;   j = src_index[i];   q[0..4] = scratch[j]: all five 0: return, nothing else of j is read or written
//   scratch[j] = 0 (the next frame starts clean without a memset)
//   row = geom_spread_row(q, halves 0..3 of splats[i], xyz and covariance halves of j, frame)
//   position[j] += row.position;  covariance[j] += row.covariance;  screen_norm[j] += row.norm;  seen[j] += 1     (f64 additions)
int launch_geom_spread(const GeomSpreadParams& p, hipStream_t stream);

// sums += other over the ten f64 planes (in f64) and the count plane (in uint64): ws_geomgrad_add
int launch_geom_merge(unsigned long long* sums, const unsigned long long* other, uint32_t n, hipStream_t stream);

}  // namespace ws
