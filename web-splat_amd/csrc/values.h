// values.h -- per-Gaussian values drawn to pixel planes, and the winner-id plane, of a prepared frame (values.hip k_values).
// Internal: the ABI is include/websplat.h, "Rendering per-Gaussian values".
#pragma once

#include <cstddef>

#include "weight_walk.h"

namespace ws {

// One launch over a prepared frame's binned, depth-ordered tile lists: the forward operator of the attribution pass (contrib.h).
// A sibling of k_contrib, not a form of the blend: one workgroup per blend tile (qw x qh quadrants, one wave each), whatever the
// blend's own scheduling (split halves, longest-first order, tiles per workgroup) would be.
struct ValuesParams {
    FrameLists frame;             // (its counters' error bits are folded into *sticky: no blend need follow)
    const float* values;          // value c of Gaussian j at (char*)values + j * stride + 4 c; nullptr with channels == 0
    size_t stride;                // bytes
    uint32_t channels;            // 0..4
    float* plane[4];              // f32 per viewport pixel, or nullptr: not written
    size_t pitch[4];              // bytes
    uint32_t* winner;             // u32 per viewport pixel, or nullptr
    size_t winner_pitch;
};
static_assert(offsetof(ValuesParams, values) == 80 && sizeof(ValuesParams) == 184, "kernarg segment of k_values: 440 B");
// k_values<qw, qh, winner != nullptr>.
//
// TO THE BIT.  The pairs, the weights wgt = b * T and the stops are tile::walk_weights' (weight_walk.h), the one function k_contrib
// (contrib.hip) runs too: in one context the pairs that contribute are exactly the pairs k_contrib sums.  The staging
// thread of a slot also loads src = src_index[idx] and the `channels` values of Gaussian src, zero-padded to four, into a third
// 16-B record plane (and src itself into a fourth plane when the winner is asked for).  Per kept pair, in list order:
//   acc[c] = fmaf(wgt, val[c], acc[c])                           c < 4 (val[c] == 0 for c >= channels)
//   if (wgt > best_w) { best_w = wgt; best_id = src; }           strict: the nearest of equal weights wins, wgt == 0 never does
// A pair outside the cut-off multiplies nothing.  At the end every lane inside the viewport stores acc[c] to each plane that is
// not null and best_id (0xFFFFFFFF: no pair had a weight above 0) to the winner plane; the lanes of a tile with an empty list
// store 0.0f and 0xFFFFFFFF.  No atomics, no wave reductions; nothing is read from the planes.
int launch_values(const ValuesParams& p, hipStream_t stream);

}  // namespace ws
