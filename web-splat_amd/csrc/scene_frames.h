// scene_frames.h -- the small rules of the scene drivers (drivers.cpp: ws_render_views, ws_scene_evaluate, the ws_scene_accumulate_*
// family, ws_scene_refit), each stated ONCE: the size of a camera's frame, the name and the aspect of its ground-truth PNG, and
// what a frame's error bits mean for a driver that may draw again.  (How far an entry list grows is frame_plan.h's
// grown_entry_capacity: the same rule as the automatic capacity's.)  Plain C++ (no HIP include), included by drivers.cpp only: the
// one walk over a split's cameras there is their consumer, and a CPU test (tests/test_scene_frames.py) enumerates them.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "websplat.h"

namespace ws {

// bin/render.rs:58-62: the frame of a camera.  The width is capped at 1600, the height rescaled in f32 and truncated.
// false: an empty image.
inline bool scene_frame_size(uint32_t cam_w, uint32_t cam_h, uint32_t* w, uint32_t* h) {
    *w = cam_w;
    *h = cam_h;
    if (*w > 1600) {
        const float s = (float)*w / 1600.0f;
        *w = 1600;
        *h = (uint32_t)((float)*h / s);
    }
    return *w != 0 && *h != 0;
}

// The ground-truth image of a camera: <gt_dir>/<img_name>, ".png" appended unless the name ends in it in any letter case.
// (img_name may fill its field without a terminator.)
inline std::string scene_truth_path(const char* gt_dir, const ws_scene_camera& c) {
    const std::string name(c.img_name, strnlen(c.img_name, sizeof c.img_name));
    const size_t L = name.size();
    const bool has_ext = L >= 4 && name[L - 4] == '.' && (name[L - 3] | 0x20) == 'p' && (name[L - 2] | 0x20) == 'n' && (name[L - 1] | 0x20) == 'g';
    return std::string(gt_dir) + "/" + name + (has_ext ? "" : ".png");
}

// A w x h PNG has the aspect of its camera when w * cam_h and h * cam_w differ by at most the camera's longer side: what
// rounding one side of a resized image to whole pixels can leave.  No resampler: the frame is drawn at the PNG's own size.
inline bool scene_truth_aspect_ok(uint32_t w, uint32_t h, uint32_t cam_w, uint32_t cam_h) {
    const uint64_t a = (uint64_t)w * cam_h, b = (uint64_t)h * cam_w;
    return cam_w != 0 && cam_h != 0 && (a > b ? a - b : b - a) <= std::max(cam_w, cam_h);
}

// Entries are emitted far -> near and truncated at the capacity, so an overflowing frame would silently lose its NEAREST splats.
// A driver that may draw again looks at the error bits after attempt 0, 1, 2 of a frame (or of a pass over a split): only a plain
// tile-entry overflow (bit 0 alone) is worth another attempt with a grown entry list, and the third attempt is the last.
enum FrameVerdict { FRAME_DONE = 0, FRAME_GROW_AND_DRAW_AGAIN = 1, FRAME_FAILED = 2 };
constexpr FrameVerdict frame_verdict(uint32_t bits, int attempt) {
    return bits == 0 ? FRAME_DONE : (((bits & ~1u) != 0 || attempt >= 2) ? FRAME_FAILED : FRAME_GROW_AND_DRAW_AGAIN);
}

}  // namespace ws
