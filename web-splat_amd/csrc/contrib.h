// contrib.h -- per-Gaussian contribution sums of a prepared frame (contrib.hip k_contrib) and the device gather behind
// ws_pointcloud_create_subset (k_pc_gather).  Internal: the ABI is include/websplat.h, "Per-Gaussian contributions".
#pragma once

#include <cstddef>

#include "weight_walk.h"

namespace ws {

// One attribution launch over a prepared frame's binned, depth-ordered tile lists.  A sibling of the blend, not a form of it:
// it writes no pixel.  One workgroup per blend tile (qw x qh quadrants, one wave each), whatever the blend's own scheduling
// (split halves, longest-first order, tiles per workgroup) would be.
struct ContribParams {
    FrameLists frame;             // (its counters' error bits are folded into *sticky: no blend may follow)
    unsigned long long* sum_q32;  // [num_points]
    uint32_t* max_bits;           // [num_points] bits of the largest weight
    // The weighted form (ws_renderer_accumulate_weighted; nullptr: the plain sums, and nothing below is read).  The members
    // stay behind the plain ones: the unweighted kernels read their arguments at the offsets they always had.
    const float* plane;           // f32 per viewport pixel
    size_t plane_pitch;           // bytes
    float scale, bias;
};
static_assert(offsetof(ContribParams, sum_q32) == 80 && sizeof(ContribParams) == 120, "kernarg segment of k_contrib: 376 B");
// k_contrib<qw, qh, plane != nullptr>.
//
// THE WEIGHTED FORM, to the bit (the ABI text is include/websplat.h, "Attributing a pixel plane").  Pairs, T and
// termination are tile::walk_weights' (weight_walk.h), which reads nothing of the plane.  Before the batch loop every lane inside the viewport loads its pixel's value once,
//   E = fminf(fmaxf(fmaf(scale, plane[p], bias), 0.0f), 1.0f), NaN -> 0;
// a lane outside the viewport loads nothing and has E = 0; nothing past a row's width-th value is read.  Per kept pair
//   v = wgt * E                      one rounded f32 multiply (fp contract off, like wgt itself)
//   q32 = (uint32_t)(v * 2^32)       exact product, truncating conversion
//   mb = q32 ? bits(v) : 0
// and q32 / mb go the way the plain form's go: DPP wave reductions, LDS partials per staged record, one 64-bit add and one 32-bit
// max per (tile, entry) with a non-zero sum.  A wave whose 64 values of E are all 0 adds nothing whatever it walks: it skips its
// walk, keeps staging and meeting the barriers, and votes "done" -- the other waves' walks are private to them, and the batch
// loop ends early only when every wave has nothing left to add.
int launch_contrib(const ContribParams& p, hipStream_t stream);

// dst[i] += src[i] (u64), dst_max[i] = max(dst_max[i], src_max[i]) on the bits: ws_contrib_add
int launch_contrib_merge(unsigned long long* sum, uint32_t* max_bits, const unsigned long long* add_sum, const uint32_t* add_max,
                         uint32_t n, hipStream_t stream);

// Gaussians indices[0..n) of a resident scene: `planes` planes of `n_src` records of `words` 32-bit words each
// (uncompressed: PC_PLANES planes of 4 words; compressed: one plane of 6 words) -> the same layout over n records
int launch_pc_gather(const uint32_t* src, uint32_t* dst, const uint32_t* indices, uint32_t n_src, uint32_t n, uint32_t planes,
                     uint32_t words, hipStream_t stream);

}  // namespace ws
