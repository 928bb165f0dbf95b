// contrib.h -- per-Gaussian contribution sums of a prepared frame (contrib.hip k_contrib) and the device gather behind
// ws_pointcloud_create_subset (k_pc_gather).  Internal: the ABI is include/websplat.h, "Per-Gaussian contributions".
#pragma once

#include <cstddef>

#include "accum_q32.h"
#include "weight_walk.h"

namespace ws {

// One attribution launch over a prepared frame's binned, depth-ordered tile lists.  A sibling of the blend, not a form of it:
// it writes no pixel.  One workgroup per blend tile (qw x qh quadrants, one wave each), whatever the blend's own scheduling
// (split halves, longest-first order, tiles per workgroup) would be.
struct ContribParams {
    FrameLists frame;  // (its counters' error bits are folded into *sticky: no blend may follow)
    Accum acc;         // acc.plane: the weighted form (ws_renderer_accumulate_weighted); nullptr: the plain sums
};
static_assert(offsetof(ContribParams, acc) == 80 && sizeof(ContribParams) == 120, "kernarg segment of k_contrib: 376 B");
// k_contrib<qw, qh, acc.plane != nullptr>.
//
// TO THE BIT (the ABI text is include/websplat.h, "Per-Gaussian contributions" and "Attributing a pixel plane"; DESIGN.md 3.4d,
// 3.4f).  Pairs, T and termination are tile::walk_weights' (weight_walk.h), which reads nothing of the plane.  Per walked pair
//   v = wgt                          the plain form (wgt == 0 for a pair outside the cut-off)
//   v = wgt * E                      the weighted form: one rounded f32 multiply (fp contract off, like wgt itself)
// and E, the wave that skips its walk, and everything from v on are the accumulator's (accum_q32.h).
int launch_contrib(const ContribParams& p, hipStream_t stream);

// dst[i] += src[i] (u64), dst_max[i] = max(dst_max[i], src_max[i]) on the bits: ws_contrib_add
int launch_contrib_merge(unsigned long long* sum, uint32_t* max_bits, const unsigned long long* add_sum, const uint32_t* add_max,
                         uint32_t n, hipStream_t stream);

// Gaussians indices[0..n) of a resident scene: `planes` planes of `n_src` records of `words` 32-bit words each
// (uncompressed: PC_PLANES planes of 4 words; compressed: one plane of 6 words) -> the same layout over n records
int launch_pc_gather(const uint32_t* src, uint32_t* dst, const uint32_t* indices, uint32_t n_src, uint32_t n, uint32_t planes,
                     uint32_t words, hipStream_t stream);

}  // namespace ws
