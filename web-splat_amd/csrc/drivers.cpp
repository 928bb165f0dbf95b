// drivers.cpp -- the reference's offline front-ends on top of the C ABI (SURVEY 8f, N2 + N4).
//
// Mirrors src/bin/render.rs:33-128 (render_views: resolution cap, fit_near_far, SplattingArgs of the offline
// callers, Rgba16Float target cleared to TRANSPARENT, PNG per view), :187-246 (download_texture: f16 -> clamp ->
// * 255 -> `as u8`), src/bin/measure.rs:27-154 (fixed 2048x2048 Rgba8Unorm target, 1 + 10 x cameras frames, one
// wait, "average FPS") and src/renderer.rs:548-582 (Display::render).  Everything here only CALLS the hot path
// through the public entry points (ws_renderer_prepare / ws_renderer_render); nothing is re-implemented.
#include <sys/stat.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gaussian_sums.h"
#include "scene_frames.h"
#include "ws_internal.h"

using namespace ws;

namespace ws {
int launch_display(const void* src, int src_format, size_t src_pitch, uint32_t w, uint32_t h, const float bg[4],
                   int dst_format, void* dst, size_t dst_pitch, hipStream_t stream);
}

namespace {

size_t texel_bytes(ws_color_format f) { return f == WS_FORMAT_RGBA8_UNORM ? 4 : (f == WS_FORMAT_RGBA16_FLOAT ? 8 : 16); }

// SplattingArgs of the offline callers (bin/render.rs:88-103, bin/measure.rs:63-78)
void offline_args(const ws_scene_camera& sc, const ws_pointcloud* pc, uint32_t vw, uint32_t vh, ws_splatting_args* a) {
    std::memset(a, 0, sizeof *a);
    ws_camera_from_scene(sc.position, sc.rotation, sc.fx, sc.fy, sc.width, sc.height, &a->camera);
    ws_aabb box;
    ws_pointcloud_bbox(pc, &box);
    ws_camera_fit_near_far(&a->camera, &box);
    a->viewport[0] = vw;
    a->viewport[1] = vh;
    a->gaussian_scaling = 1.0f;
    a->max_sh_deg = ws_pointcloud_sh_deg(pc);
    a->walltime_secs = 100.0;
    // background_color: TRANSPARENT (all zero)
}

bool make_dir(const std::string& p) {
    struct stat st;
    if (stat(p.c_str(), &st) == 0) return S_ISDIR(st.st_mode);
    return mkdir(p.c_str(), 0777) == 0;
}
bool make_dirs(const std::string& p) {  // create_dir_all
    for (size_t i = 1; i < p.size(); ++i)
        if (p[i] == '/' && !make_dir(p.substr(0, i))) return false;
    return make_dir(p);
}

}  // namespace

extern "C" {

int ws_download_texture_rgba8(ws_context* ctx, const void* d_image, ws_color_format format, uint32_t width,
                              uint32_t height, size_t row_pitch_bytes, uint8_t* out, void* stream_v) {
    if (!ctx || !d_image || !out || width == 0 || height == 0) return fail(WS_ERR_INVALID, "ws_download_texture_rgba8: bad argument");
    const size_t tb = texel_bytes(format);
    if (row_pitch_bytes < tb * width) return fail(WS_ERR_INVALID, "ws_download_texture_rgba8: row pitch too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    std::vector<uint8_t> raw;
    try {
        raw.resize(row_pitch_bytes * height);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_download_texture_rgba8: host allocation failed");
    }
    WS_HIP(hipMemcpyAsync(raw.data(), d_image, raw.size(), hipMemcpyDeviceToHost, stream));
    WS_HIP(hipStreamSynchronize(stream));
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t* row = raw.data() + (size_t)y * row_pitch_bytes;
        uint8_t* o = out + (size_t)y * width * 4;
        for (uint32_t i = 0; i < width * 4; ++i) {
            if (format == WS_FORMAT_RGBA8_UNORM) {
                o[i] = row[i];
                continue;
            }
            float v;
            if (format == WS_FORMAT_RGBA16_FLOAT) {
                uint16_t h;
                std::memcpy(&h, row + (size_t)i * 2, 2);
                v = host_f16_to_f32(h);
            } else {
                std::memcpy(&v, row + (size_t)i * 4, 4);
            }
            // f32::clamp(0., 1.) * 255. as u8  (bin/render.rs:232; NaN -> 0 like Rust's saturating cast)
            v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
            const float s = v * 255.0f;
            o[i] = (s != s) ? 0 : (uint8_t)s;
        }
    }
    return WS_OK;
}

// ---- the scene drivers ------------------------------------------------------------------------------------------------------
// Seven drivers, ONE walk over the cameras of a split (SceneWalk::pass).  A driver is its argument checks, a description of the
// frames it needs (SceneFrames) and what it does with one frame (its per-frame function); the small rules -- the frame's size
// under the 1600-px cap, the ground-truth PNG's name and aspect, what a frame's error bits mean -- are scene_frames.h's, and how
// far an entry list grows is frame_plan.h's.  Like everything here the walk only calls public entry points.
extern "C++" {
namespace {

ws_image_view view_of(const void* p, ws_color_format f, size_t pitch, const float* bg) {
    ws_image_view v;
    std::memset(&v, 0, sizeof v);
    v.d_pixels = p;
    v.format = f;
    v.row_pitch_bytes = pitch;
    v.over_background = bg ? 1 : 0;
    for (int i = 0; i < 3 && bg; ++i) v.background[i] = bg[i];
    return v;
}

// the cloud's own background colour, or black: what both images of a comparison go over
void eval_background(const ws_pointcloud* pc, float bg[3]) {
    bg[0] = bg[1] = bg[2] = 0.0f;
    float pc_bg[3];
    if (ws_pointcloud_background_color(pc, pc_bg) == 1) std::memcpy(bg, pc_bg, sizeof pc_bg);
}

// One look at a renderer's error bits (syncs, and clears them).  A plain overflow leaves the renderer a grown entry list for
// whatever it draws next.
int look_and_grow(ws_renderer* r, uint32_t* bits) {
    uint32_t needed = 0;
    const int rc = ws_renderer_errors(r, bits, &needed, 1);
    if (rc == WS_OK && (*bits & 1u)) ws_renderer_set_tile_entry_capacity(r, grown_entry_capacity(needed));
    return rc;
}

// What a driver does about frames that overflowed their entry lists.  These are real differences:
enum OverflowPolicy {
    OVERFLOW_DRAWS_THE_FRAME_AGAIN,  // look at the bits behind every frame (a sync per frame), grow, draw that frame again
    OVERFLOW_IS_THE_DRIVERS,         // nothing read back per frame: SceneWalk::bits after the pass, and the driver may run another
    OVERFLOW_FAILS,                  // sums of frames that dropped entries cannot be mended: WS_ERR_OVERFLOW, "... incomplete"
};

// The frames a driver needs of every camera of `split` (sorted by id).
struct SceneFrames {
    const char* who;  // the entry point, for messages
    const ws_pointcloud* pc;
    const ws_scene* scene;
    int split;
    const ws_pointcloud* ref_pc;  // image b: the render of ref_pc, or the PNGs of gt_dir, or (neither) none
    const char* gt_dir;
    bool contrib;        // pc is prepared with contributions enabled
    bool render_a;       // pc is drawn into the Rgba16Float target, cleared to TRANSPARENT
    size_t plane_texel;  // bytes per pixel of a scratch plane, 0: none
    OverflowPolicy overflow;
    const char* incomplete;  // OVERFLOW_FAILS: what the message calls incomplete
};

// One frame, as the per-frame function gets it: everything is enqueued on the null stream, nothing has been waited for.
struct SceneFrame {
    uint32_t index, count;  // the camera's position in the split, and the split's size
    ws_renderer* r;         // pc's renderer, prepared for this frame
    uint32_t w, h;
    ws_image_view va, vb;  // pc's render over the background (render_a only), and image b
    void* plane;
};

// The walk owns the renderers (set up as bin/render.rs:154 needs them), the target, image b and the plane.  A frame is the
// camera's capped size (bin/render.rs:58-62), fit_near_far, the offline callers' SplattingArgs -- except with gt_dir, where it
// is the PNG's own size under the camera's field of view (no resampler: the renderer derives the focal length from both).
struct SceneWalk {
    ws_context* ctx;
    const SceneFrames d;
    std::vector<ws_scene_camera> cams;
    size_t max_px = 0;  // the largest frame at the cameras' own sizes
    float bg[3];
    ws_renderer *r = nullptr, *rb = nullptr;
    void *target = nullptr, *other = nullptr, *plane = nullptr;
    size_t capacity = 0;  // pixels that target, image b and plane hold
    uint32_t frames = 0;  // frames of the last pass whose per-frame function succeeded
    uint32_t bits = 0;    // error bits the last pass left behind

    SceneWalk(ws_context* c, const SceneFrames& f) : ctx(c), d(f) {}
    SceneWalk(const SceneWalk&) = delete;
    ~SceneWalk() {
        release();
        if (rb) ws_renderer_destroy(rb);
        if (r) ws_renderer_destroy(r);
    }

    // The cameras and the renderers.  A camera with an empty image is refused here, before the first frame.
    int open() {
        const uint32_t n = ws_scene_cameras(d.scene, d.split, 0, nullptr);
        cams.resize(n);
        ws_scene_cameras(d.scene, d.split, n, cams.data());
        for (size_t i = 0; i < cams.size() && !d.gt_dir; ++i) {
            uint32_t w, h;
            if (!scene_frame_size(cams[i].width, cams[i].height, &w, &h)) return fail(WS_ERR_INVALID, std::string(d.who) + ": camera with an empty image");
            max_px = std::max(max_px, (size_t)w * h);
        }
        eval_background(d.pc, bg);
        int rc = renderer_for(d.pc, &r);
        if (rc == WS_OK && d.contrib) rc = ws_renderer_enable_contrib(r, 1);
        if (rc == WS_OK && d.ref_pc) rc = renderer_for(d.ref_pc, &rb);
        return rc;
    }

    // bin/render.rs:154 draws into an Rgba16Float target: the fixed-function blender rounds the destination to f16 after every
    // splat.  The target-precision blend mode reproduces that (ws_context_config::render_views_fast_blend: the throughput
    // blend, one rounding at the store).  Only render() reads the mode.
    int renderer_for(const ws_pointcloud* cloud, ws_renderer** out) {
        const int rc = ws_renderer_create(ctx, WS_FORMAT_RGBA16_FLOAT, ws_pointcloud_sh_deg(cloud), ws_pointcloud_compressed(cloud), out);
        if (rc == WS_OK && !ctx->render_views_fast_blend) (void)ws_renderer_set_blend_mode(*out, WS_BLEND_TARGET_PRECISION);
        return rc;
    }

    void release() {
        for (void** p : {&target, &other, &plane}) {
            if (*p) ws_device_free(ctx, *p);
            *p = nullptr;
        }
        capacity = 0;
    }
    // grown when a frame has more pixels than they hold (every earlier frame has been waited for, or the free waits)
    int reserve(size_t px) {
        if (px <= capacity) return WS_OK;
        release();
        int rc = d.render_a ? ws_device_malloc(ctx, px * 8, &target) : (int)WS_OK;
        if (rc == WS_OK && (d.ref_pc || d.gt_dir)) rc = ws_device_malloc(ctx, px * (d.ref_pc ? 8 : 4), &other);
        if (rc == WS_OK && d.plane_texel) rc = ws_device_malloc(ctx, px * d.plane_texel, &plane);
        if (rc == WS_OK) capacity = px;
        return rc;
    }

    // The camera's ground-truth PNG as RGBA8, refused unless it has the camera's aspect.  *rgba is released with ws_host_free
    // (nothing to release on an error).
    int read_truth(const ws_scene_camera& c, uint32_t* w, uint32_t* h, uint8_t** rgba) {
        const std::string path = scene_truth_path(d.gt_dir, c);
        int rc = ws_png_read_rgba8(path.c_str(), w, h, rgba);  // (the message names the file)
        if (rc == WS_OK && !scene_truth_aspect_ok(*w, *h, c.width, c.height)) {
            rc = fail(WS_ERR_INVALID, std::string(d.who) + ": " + path + " (" + std::to_string(*w) + " x " + std::to_string(*h) + ") does not have the aspect of its camera (" +
                                          std::to_string(c.width) + " x " + std::to_string(c.height) + ")");
            ws_host_free(*rgba);
            *rgba = nullptr;
        }
        return rc;
    }

    // Every camera once, in order, all on one stream: image b, pc prepared (and drawn), the per-frame function.  The next frame's
    // renders and plane are ordered behind the per-frame function's work on the stream: targets and plane are reused.  One sync
    // and one look at the error bits at the end.  May be called again: the renderers keep what they learnt of the demand.
    template <class PerFrame>
    int pass(PerFrame&& per_frame) {
        const float clear[4] = {0, 0, 0, 0};
        const std::string who(d.who);
        int rc = WS_OK;
        frames = bits = 0;
        for (uint32_t i = 0; i < cams.size() && rc == WS_OK; ++i) {
            const ws_scene_camera& c = cams[i];
            uint32_t w = 0, h = 0;
            uint8_t* rgba = nullptr;
            if (d.gt_dir) rc = read_truth(c, &w, &h, &rgba);
            else scene_frame_size(c.width, c.height, &w, &h);
            const size_t px = (size_t)w * h;
            if (rc == WS_OK) rc = reserve(d.gt_dir ? px : max_px);
            // the ground truth into image b: the comparison of the frame before still reads it, so that is waited for
            if (rc == WS_OK && rgba) rc = ws_sync(ctx, nullptr);
            if (rc == WS_OK && rgba) rc = ws_memcpy_h2d(ctx, other, rgba, px * 4, nullptr);
            if (rgba) ws_host_free(rgba);
            ws_splatting_args a;
            if (rc == WS_OK) offline_args(c, d.pc, w, h, &a);
            for (int attempt = 0; rc == WS_OK; ++attempt) {
                rc = ws_renderer_prepare(r, d.pc, &a, nullptr);
                if (rc == WS_OK && d.render_a) rc = ws_renderer_render(r, d.pc, clear, target, (size_t)w * 8, nullptr);
                if (rc != WS_OK || d.overflow != OVERFLOW_DRAWS_THE_FRAME_AGAIN) break;
                uint32_t frame_bits = 0;
                rc = look_and_grow(r, &frame_bits);
                const FrameVerdict v = frame_verdict(frame_bits, attempt);
                if (rc != WS_OK || v == FRAME_DONE) break;
                if (v == FRAME_FAILED) rc = fail(WS_ERR_OVERFLOW, who + ": the frame reported device-side errors (tile-entry overflow or a look-back time-out)");
            }
            if (rc == WS_OK && rb) {
                offline_args(c, d.ref_pc, w, h, &a);
                rc = ws_renderer_prepare(rb, d.ref_pc, &a, nullptr);
                if (rc == WS_OK) rc = ws_renderer_render(rb, d.ref_pc, clear, other, (size_t)w * 8, nullptr);
            }
            if (rc != WS_OK) break;
            const SceneFrame f{i, (uint32_t)cams.size(), r, w, h, view_of(target, WS_FORMAT_RGBA16_FLOAT, (size_t)w * 8, bg),
                               rb ? view_of(other, WS_FORMAT_RGBA16_FLOAT, (size_t)w * 8, bg)
                                  : view_of(other, WS_FORMAT_RGBA8_UNORM, (size_t)w * 4, nullptr),  // opaque: alpha ignored
                               plane};
            rc = per_frame(f);
            if (rc == WS_OK) ++frames;
        }
        for (ws_renderer* x : {r, rb}) {  // (the one sync)
            uint32_t b = 0;
            if (rc == WS_OK && x) rc = look_and_grow(x, &b);
            bits |= b;
        }
        if (rc == WS_OK && bits && d.overflow == OVERFLOW_FAILS)
            rc = fail(WS_ERR_OVERFLOW, who + ": a frame reported device-side errors (tile-entry overflow or a look-back time-out): " + d.incomplete);
        if (rc != WS_OK) (void)ws_sync(ctx, nullptr);
        return rc;
    }
};

// a driver that walks its split once: *frames is what it enqueued, also when it fails
template <class PerFrame>
int walk_once(ws_context* ctx, const SceneFrames& d, uint32_t* frames, PerFrame&& per_frame) {
    SceneWalk walk(ctx, d);
    int rc = walk.open();
    if (rc == WS_OK) rc = walk.pass(per_frame);
    if (frames) *frames = walk.frames;
    return rc;
}

// what several entry points refuse in the same words
int refuse_unless_one_split(const std::string& who, int split) {
    return split == WS_SPLIT_TRAIN || split == WS_SPLIT_TEST ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": split must be train or test");
}
int refuse_unless_a_split(const std::string& who, int split) {
    return split == WS_SPLIT_TRAIN || split == WS_SPLIT_TEST || split == WS_SPLIT_ALL ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": split must be train, test or all");
}
int refuse_unless_one_image_b(const std::string& who, const ws_pointcloud* ref_pc, const char* gt_dir) {
    return (ref_pc != nullptr) != (gt_dir != nullptr) ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": exactly one of ref_pc and gt_dir");
}
int refuse_debug_cut(const std::string& who, const ws_context* ctx) {
    return ctx->debug_cut ? fail(WS_ERR_UNSUPPORTED, who + ": the context stops its frames early (debug_cut)") : (int)WS_OK;
}
int refuse_kind(const std::string& who, int kind) {
    return kind == WS_ERROR_SQ || kind == WS_ERROR_ABS ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": kind must be WS_ERROR_SQ or WS_ERROR_ABS");
}
int refuse_scale(const std::string& who, const char* name, float v) {
    return std::isfinite(v) && v > 0.0f ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": " + name + " must be finite and above 0");
}

// One frame of ws_scene_accumulate_gradient and ws_scene_refit: image a is the frame's f32 base plane over the cloud's background,
// the first half of the scratch plane; the loss gradient is the second half.  ws_renderer_accumulate_gradient in its two steps,
// the plane made of pass 1's image.
// Where the frames go is a GradTarget (gaussian_sums.h): the steps are the same for a ws_grad, a ws_shgrad and a ws_geomgrad.
// (the pass speaks under the name of the target's own ws_renderer_accumulate_* entry point, as it always has)
int gradient_frame(ws_context* ctx, const ws_pointcloud* pc, const GradTarget& grad, GradDesc d, int kind, const SceneFrame& f) {
    const size_t pitch = (size_t)f.w * 16;
    float* base = static_cast<float*>(f.plane);
    float* g = base + (size_t)f.w * f.h * 4;
    d.d_base = base;
    d.d_grad = g;
    d.base_pitch_bytes = d.grad_pitch_bytes = pitch;
    int frc = ws_internal_gradient_passes(nullptr, f.r, pc, grad, d, nullptr, GRAD_BASE);
    const ws_image_view va = view_of(base, WS_FORMAT_RGBA32_FLOAT, pitch, nullptr);  // (the alpha slot holds T_end: ignored)
    if (frc == WS_OK) frc = ws_image_error_gradient(ctx, &va, &f.vb, f.w, f.h, kind, 0, g, pitch, nullptr);
    if (frc == WS_OK) frc = ws_internal_gradient_passes(nullptr, f.r, pc, grad, d, nullptr, GRAD_SUMS | GRAD_SPREAD);
    return frc;
}

// ws_scene_accumulate_gradient, ws_scene_accumulate_sh_gradient and ws_scene_accumulate_geometry_gradient
int scene_accumulate_gradient(const std::string& who, ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split,
                              const ws_pointcloud* ref_pc, const char* gt_dir, int kind, float scale, float second_scale, const GradTarget& grad,
                              uint32_t* frames) {
    if (frames) *frames = 0;
    if (const int rc = refuse_kind(who, kind)) return rc;
    if (const int rc = refuse_scale(who, "scale", scale)) return rc;
    if (const int rc = refuse_scale(who, grad.kind == GRAD_GEOMETRY ? "geometry_scale" : "opacity_scale", second_scale)) return rc;
    if (const int rc = refuse_unless_a_split(who, split)) return rc;
    if (!ctx || !pc || !scene || !grad.acc) return fail(WS_ERR_INVALID, who + ": null argument");
    if (const int rc = refuse_unless_one_image_b(who, ref_pc, gt_dir)) return rc;
    if (grad.acc->num_points != ws_pointcloud_num_points(pc)) return fail(WS_ERR_INVALID, who + ": the accumulator was created for another number of points");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    GradDesc d;
    eval_background(pc, d.background);
    d.scale = scale;
    d.second_scale = second_scale;
    return walk_once(ctx, {who.c_str(), pc, scene, split, ref_pc, gt_dir, true, false, 32, OVERFLOW_FAILS, "the accumulators are incomplete"}, frames,
                     [&](const SceneFrame& f) { return gradient_frame(ctx, pc, grad, d, kind, f); });
}

// ws_scene_refit (sh false: params->base is the caller's ws_refit_params, the rest is not looked at) and ws_scene_refit_sh: per
// epoch the frames of the gradient driver into an accumulator of the driver's own, an Adam step and a reset after every batch.
// Everything is enqueued on one stream, so the next frame's K1 reads the planes the step before it wrote; a walk of its own per
// epoch brings the one sync and the one look at the error bits per epoch.
int scene_refit(const std::string& who, ws_context* ctx, ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                const char* gt_dir, int kind, float opacity_scale, ws_refit* refit, const ws_refit_sh_params* params, bool sh,
                uint32_t epochs, uint32_t views_per_step, uint32_t* steps) {
    if (steps) *steps = 0;
    if (const int rc = refuse_kind(who, kind)) return rc;
    if (const int rc = refuse_scale(who, "opacity_scale", opacity_scale)) return rc;
    if (const int rc = refuse_unless_a_split(who, split)) return rc;
    if (const int rc = sh ? ws_internal_refit_check_sh_params(params, who, false) : ws_internal_refit_check_params(params ? &params->base : nullptr, who, false)) return rc;
    if (!ctx || !pc || !scene || !refit) return fail(WS_ERR_INVALID, who + ": null argument");
    if (const int rc = refuse_unless_one_image_b(who, ref_pc, gt_dir)) return rc;
    if (ref_pc == pc) return fail(WS_ERR_INVALID, who + ": ref_pc is the cloud being refitted");
    if (ws_refit_num_points(refit) != ws_pointcloud_num_points(pc)) return fail(WS_ERR_INVALID, who + ": the refit object was created for another number of points");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    ws_grad* colour = nullptr;
    ws_shgrad* rest = nullptr;
    int rc = sh ? ws_refit_enable_sh(refit, pc, nullptr) : (int)WS_OK;
    if (rc == WS_OK)
        rc = sh ? ws_shgrad_create(ctx, ws_pointcloud_num_points(pc), ws_pointcloud_sh_deg(pc), &rest) : ws_grad_create(ctx, ws_pointcloud_num_points(pc), &colour);
    const GradTarget grad = sh ? GradTarget(rest) : GradTarget(colour);
    GradDesc d;  // (scale 1)
    eval_background(pc, d.background);
    d.second_scale = opacity_scale;
    uint32_t taken = 0;
    for (uint32_t epoch = 0; epoch < epochs && rc == WS_OK; ++epoch) {
        uint32_t in_batch = 0;
        rc = walk_once(ctx, {who.c_str(), pc, scene, split, ref_pc, gt_dir, true, false, 32, OVERFLOW_FAILS, "the accumulators are incomplete"}, nullptr,
                       [&](const SceneFrame& f) {
                           int frc = gradient_frame(ctx, pc, grad, d, kind, f);
                           if (frc != WS_OK) return frc;
                           ++in_batch;
                           if (in_batch < (views_per_step ? views_per_step : f.count) && f.index + 1 < f.count) return frc;
                           ws_refit_sh_params sp = *params;
                           sp.base.colour_unit = 1.0 / (WS_GRAD_SUM_SCALE * (double)in_batch);
                           sp.base.opacity_unit = 1.0 / (WS_GRAD_SUM_SCALE * (double)opacity_scale * (double)in_batch);
                           frc = sh ? ws_refit_step_sh(refit, pc, rest, &sp, nullptr) : ws_refit_step(refit, pc, colour, &sp.base, nullptr);
                           if (frc == WS_OK) ++taken, in_batch = 0, frc = GaussianSums::reset(grad.acc, who.c_str(), nullptr);
                           return frc;
                       });
    }
    if (steps) *steps = taken;
    if (colour) ws_grad_destroy(colour);
    if (rest) ws_shgrad_destroy(rest);
    return rc;
}

}  // namespace
}  // extern "C++"

// bin/render.rs:33-128: every camera of `split` drawn and written as <out_dir>/<split>/<index>.png
int ws_render_views(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const char* out_dir,
                    uint32_t* rendered) {
    if (!ctx || !pc || !scene || !out_dir) return fail(WS_ERR_INVALID, "ws_render_views: null argument");
    if (const int rc = refuse_unless_one_split("ws_render_views", split)) return rc;
    if (rendered) *rendered = 0;
    const std::string dir = std::string(out_dir) + "/" + (split == WS_SPLIT_TEST ? "test" : "train");
    if (!make_dirs(dir)) return fail(WS_ERR_IO, "ws_render_views: cannot create " + dir);
    std::vector<uint8_t> rgba;
    return walk_once(ctx, {"ws_render_views", pc, scene, split, nullptr, nullptr, false, true, 0, OVERFLOW_DRAWS_THE_FRAME_AGAIN, nullptr}, nullptr,
                     [&](const SceneFrame& f) {
                         rgba.resize((size_t)f.w * f.h * 4);
                         int rc = ws_download_texture_rgba8(ctx, f.va.d_pixels, WS_FORMAT_RGBA16_FLOAT, f.w, f.h, (size_t)f.w * 8, rgba.data(), nullptr);
                         char name[32];
                         std::snprintf(name, sizeof name, "/%05u.png", f.index);
                         if (rc == WS_OK) rc = ws_png_write_rgba8((dir + name).c_str(), f.w, f.h, rgba.data(), (size_t)f.w * 4);
                         if (rc == WS_OK && rendered) *rendered = f.index + 1;
                         return rc;
                     });
}

// Every camera of `split` into per-Gaussian accumulators (websplat.h "Per-Gaussian contribution"): no target and no blend,
// prepare() and the attribution launches.
int ws_scene_accumulate_contrib(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, ws_contrib* c,
                                uint32_t* frames) {
    const std::string who("ws_scene_accumulate_contrib");
    if (!ctx || !pc || !scene || !c) return fail(WS_ERR_INVALID, who + ": null argument");
    if (const int rc = refuse_unless_one_split(who, split)) return rc;
    if (frames) *frames = 0;
    if (ws_contrib_num_points(c) != ws_pointcloud_num_points(pc))
        return fail(WS_ERR_INVALID, who + ": the accumulator was created for another number of points");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    return walk_once(ctx, {who.c_str(), pc, scene, split, nullptr, nullptr, true, false, 0, OVERFLOW_FAILS, "the accumulator is incomplete"}, frames,
                     [&](const SceneFrame& f) { return ws_renderer_accumulate_contrib(f.r, pc, c, nullptr); });
}

// ... and what deleting each Gaussian alone would do to them (websplat.h "Removal effect"), over the cloud's own background
// colour, or black; `weight`: the plain contribution sums of the same prepared frames.
int ws_scene_accumulate_removal(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, int kind, float scale,
                                ws_contrib* effect, ws_contrib* weight, uint32_t* frames) {
    const std::string who("ws_scene_accumulate_removal");
    if (frames) *frames = 0;
    if (const int rc = refuse_kind(who, kind)) return rc;
    if (const int rc = refuse_scale(who, "scale", scale)) return rc;
    if (const int rc = refuse_unless_one_split(who, split)) return rc;
    if (!ctx || !pc || !scene || !effect) return fail(WS_ERR_INVALID, who + ": null argument");
    if (ws_contrib_num_points(effect) != ws_pointcloud_num_points(pc) || (weight && ws_contrib_num_points(weight) != ws_pointcloud_num_points(pc)))
        return fail(WS_ERR_INVALID, who + ": an accumulator was created for another number of points");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    ws_removal_params rp;
    std::memset(&rp, 0, sizeof rp);
    eval_background(pc, rp.background);
    rp.kind = kind;
    rp.scale = scale;
    return walk_once(ctx, {who.c_str(), pc, scene, split, nullptr, nullptr, true, false, 0, OVERFLOW_FAILS, "the accumulators are incomplete"}, frames,
                     [&](const SceneFrame& f) {
                         int rc = ws_renderer_accumulate_removal(f.r, pc, effect, &rp, nullptr);
                         if (rc == WS_OK && weight) rc = ws_renderer_accumulate_contrib(f.r, pc, weight, nullptr);
                         return rc;
                     });
}

// Every camera of `split` compared on the device (websplat.h "Image metrics"): `pc` against another cloud, or against
// ground-truth PNGs.
int ws_scene_evaluate(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                      const char* gt_dir, uint32_t flags, ws_metrics* m, uint32_t* frames) {
    const std::string who("ws_scene_evaluate");
    if (!ctx || !pc || !scene || !m) return fail(WS_ERR_INVALID, who + ": null argument");
    if (frames) *frames = 0;
    if (const int rc = refuse_unless_a_split(who, split)) return rc;
    if (const int rc = refuse_unless_one_image_b(who, ref_pc, gt_dir)) return rc;
    if (flags & ~WS_METRICS_QUANTIZE_U8) return fail(WS_ERR_INVALID, who + ": unknown flag bits");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    // Against PNGs every frame is waited for anyway (the upload of the next ground truth), so an overflowed frame is drawn again
    // on the spot.  Against a cloud nothing is read back per frame: the bits are looked at once, after the pass, and a pass whose
    // frames overflowed is not a measurement -- the lists have grown, the whole split runs again (as ws_measure does).
    SceneWalk walk(ctx, {who.c_str(), pc, scene, split, ref_pc, gt_dir, false, true, 0, ref_pc ? OVERFLOW_IS_THE_DRIVERS : OVERFLOW_DRAWS_THE_FRAME_AGAIN, nullptr});
    const uint32_t base = ws_metrics_count(m);
    int rc = walk.open();
    for (int attempt = 0; rc == WS_OK; ++attempt) {
        rc = walk.pass([&](const SceneFrame& f) { return ws_metrics_add(m, &f.va, &f.vb, f.w, f.h, flags, nullptr, 0, nullptr); });
        const FrameVerdict v = frame_verdict(walk.bits, attempt);
        if (rc != WS_OK || v == FRAME_DONE) break;
        ws_internal_metrics_truncate(m, base);
        if (v == FRAME_FAILED) rc = fail(WS_ERR_OVERFLOW, who + ": frames reported device-side errors (tile-entry overflow or a look-back time-out)");
    }
    if (rc != WS_OK) ws_internal_metrics_truncate(m, base);  // (the metrics as they stood, and 0 frames)
    else if (frames) *frames = walk.frames;
    return rc;
}

// Every camera of `split` blamed on the Gaussians of `pc` (websplat.h "Attributing a pixel plane to Gaussians"): the frames of
// ws_scene_evaluate with contributions enabled, their per-pixel error against `ref_pc` or the ground-truth PNGs in an f32 plane,
// and the weighted contribution sums.
int ws_scene_accumulate_error(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                              const char* gt_dir, int kind, uint32_t flags, ws_contrib* err, ws_contrib* weight, uint32_t* frames) {
    const std::string who("ws_scene_accumulate_error");
    if (!ctx || !pc || !scene || !err) return fail(WS_ERR_INVALID, who + ": null argument");
    if (frames) *frames = 0;
    if (const int rc = refuse_unless_a_split(who, split)) return rc;
    if (const int rc = refuse_unless_one_image_b(who, ref_pc, gt_dir)) return rc;
    if (flags & ~WS_METRICS_QUANTIZE_U8) return fail(WS_ERR_INVALID, who + ": unknown flag bits");
    if (kind != WS_ERROR_SQ && kind != WS_ERROR_ABS && kind != WS_ERROR_DSSIM)
        return fail(WS_ERR_INVALID, who + ": kind must be WS_ERROR_SQ, WS_ERROR_ABS or WS_ERROR_DSSIM");
    if (ws_contrib_num_points(err) != ws_pointcloud_num_points(pc) || (weight && ws_contrib_num_points(weight) != ws_pointcloud_num_points(pc)))
        return fail(WS_ERR_INVALID, who + ": an accumulator was created for another number of points");
    if (const int rc = refuse_debug_cut(who, ctx)) return rc;
    ws_metrics* ssim = nullptr;  // WS_ERROR_DSSIM: one slot, written again by every frame; only its map is used
    int rc = kind == WS_ERROR_DSSIM ? ws_metrics_create(ctx, 1, &ssim) : (int)WS_OK;
    if (rc == WS_OK)
        rc = walk_once(ctx, {who.c_str(), pc, scene, split, ref_pc, gt_dir, true, true, 4, OVERFLOW_FAILS, "the accumulators are incomplete"}, frames,
                       [&](const SceneFrame& f) {
                           ws_plane_view pv;
                           pv.d_values = static_cast<const float*>(f.plane);
                           pv.row_pitch_bytes = (size_t)f.w * 4;
                           pv.scale = 1.0f;
                           pv.bias = 0.0f;
                           int frc;
                           if (kind == WS_ERROR_DSSIM) {  // (1 - ssim) / 2 of the map
                               frc = ws_metrics_reset(ssim, nullptr);
                               if (frc == WS_OK) frc = ws_metrics_add(ssim, &f.va, &f.vb, f.w, f.h, flags, static_cast<float*>(f.plane), (size_t)f.w * 4, nullptr);
                               pv.scale = -0.5f;
                               pv.bias = 0.5f;
                           } else {
                               frc = ws_image_error_plane(ctx, &f.va, &f.vb, f.w, f.h, kind, flags, static_cast<float*>(f.plane), (size_t)f.w * 4, nullptr);
                           }
                           if (frc == WS_OK) frc = ws_renderer_accumulate_weighted(f.r, pc, err, &pv, nullptr);
                           if (frc == WS_OK && weight) frc = ws_renderer_accumulate_contrib(f.r, pc, weight, nullptr);
                           return frc;
                       });
    if (ssim) ws_metrics_destroy(ssim);
    return rc;
}

// ... and the colour and ln-opacity gradients of that error (websplat.h "Gradients of an image loss"): the same frames without
// the Rgba16Float render of `pc`, a plane of two float4 per pixel (gradient_frame).
int ws_scene_accumulate_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                 const char* gt_dir, int kind, float scale, float opacity_scale, ws_grad* grad, uint32_t* frames) {
    return scene_accumulate_gradient("ws_scene_accumulate_gradient", ctx, pc, scene, split, ref_pc, gt_dir, kind, scale, opacity_scale, grad, frames);
}

// ... the same frames into a ws_shgrad (websplat.h "SH gradients")
int ws_scene_accumulate_sh_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                    const char* gt_dir, int kind, float scale, float opacity_scale, ws_shgrad* grad, uint32_t* frames) {
    return scene_accumulate_gradient("ws_scene_accumulate_sh_gradient", ctx, pc, scene, split, ref_pc, gt_dir, kind, scale, opacity_scale, grad, frames);
}

// ... and into a ws_geomgrad (websplat.h "Geometry gradients"): geometry_scale where the other two have opacity_scale
int ws_scene_accumulate_geometry_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                          const char* gt_dir, int kind, float scale, float geometry_scale, ws_geomgrad* grad, uint32_t* frames) {
    return scene_accumulate_gradient("ws_scene_accumulate_geometry_gradient", ctx, pc, scene, split, ref_pc, gt_dir, kind, scale, geometry_scale, grad, frames);
}

// ... and the loops those gradients are for (websplat.h "Refitting colour and opacity"; scene_refit above)
int ws_scene_refit(ws_context* ctx, ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc, const char* gt_dir,
                   int kind, float opacity_scale, ws_refit* refit, const ws_refit_params* params, uint32_t epochs, uint32_t views_per_step,
                   uint32_t* steps) {
    ws_refit_sh_params block;
    std::memset(&block, 0, sizeof block);
    if (params) block.base = *params;
    return scene_refit("ws_scene_refit", ctx, pc, scene, split, ref_pc, gt_dir, kind, opacity_scale, refit, params ? &block : nullptr, false, epochs, views_per_step, steps);
}

int ws_scene_refit_sh(ws_context* ctx, ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc, const char* gt_dir,
                      int kind, float opacity_scale, ws_refit* refit, const ws_refit_sh_params* params, uint32_t epochs, uint32_t views_per_step,
                      uint32_t* steps) {
    return scene_refit("ws_scene_refit_sh", ctx, pc, scene, split, ref_pc, gt_dir, kind, opacity_scale, refit, params, true, epochs, views_per_step, steps);
}

int ws_measure(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, uint32_t num_samples,
               uint32_t frames_in_flight, float* fps) {
    if (!ctx || !pc || !scene || !fps) return fail(WS_ERR_INVALID, "ws_measure: null argument");
    if (num_samples == 0) num_samples = 10;  // bin/measure.rs:98
    if (frames_in_flight == 0) frames_in_flight = 1;
    const uint32_t n = ws_scene_cameras(scene, WS_SPLIT_TRAIN, 0, nullptr);
    if (n == 0) return fail(WS_ERR_INVALID, "ws_measure: the scene has no training cameras");
    std::vector<ws_scene_camera> cams(n);
    ws_scene_cameras(scene, WS_SPLIT_TRAIN, n, cams.data());
    const uint32_t W = 2048, H = 2048;  // bin/measure.rs:34
    std::vector<ws_renderer*> rs(frames_in_flight, nullptr);
    std::vector<void*> targets(frames_in_flight, nullptr);
    std::vector<Stream> streams(frames_in_flight);  // slot 0 stays empty: the null stream
    int rc = WS_OK;
    for (uint32_t k = 0; k < frames_in_flight && rc == WS_OK; ++k) {
        rc = ws_renderer_create(ctx, WS_FORMAT_RGBA8_UNORM, ws_pointcloud_sh_deg(pc), ws_pointcloud_compressed(pc), &rs[k]);
        if (rc == WS_OK) ws_internal_renderer_set_throughput_mode(rs[k], frames_in_flight > 1);
        if (rc == WS_OK) rc = ws_device_malloc(ctx, (size_t)W * H * 4, &targets[k]);
        if (rc == WS_OK && k > 0 && streams[k].create() != WS_OK) rc = fail(WS_ERR_HIP, "ws_measure: hipStreamCreate failed");
    }
    const float clear[4] = {0, 0, 0, 0};
    // The measurement, at most three times: a run whose frames overflowed the (automatic) tile-entry capacity is not a rate --
    // every slot's renderer is given 1.25 x the largest demand any slot saw and the WHOLE procedure runs again (a
    // scene heavier than the automatic capacity used to fail here for good, each call starting from fresh renderers).
    for (int attempt = 0; rc == WS_OK; ++attempt) {
        const auto start = std::chrono::steady_clock::now();  // before the warm-up frame (bin/measure.rs:50)
        ws_splatting_args a;
        offline_args(cams[0], pc, W, H, &a);
        rc = ws_renderer_prepare(rs[0], pc, &a, streams[0].get());  // "first render to lazy init sorter stuff"
        if (rc == WS_OK) rc = ws_renderer_render(rs[0], pc, clear, targets[0], (size_t)W * 4, streams[0].get());
        uint32_t f = 0;
        for (uint32_t i = 0; i < n && rc == WS_OK; ++i) {
            offline_args(cams[i], pc, W, H, &a);
            for (uint32_t s = 0; s < num_samples && rc == WS_OK; ++s, ++f) {
                const uint32_t k = f % frames_in_flight;
                rc = ws_renderer_prepare(rs[k], pc, &a, streams[k].get());
                if (rc == WS_OK) rc = ws_renderer_render(rs[k], pc, clear, targets[k], (size_t)W * 4, streams[k].get());
            }
        }
        if (rc == WS_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(WS_ERR_HIP, "ws_measure: device sync failed");  // device.poll(Wait)
        const float secs = std::chrono::duration<float>(std::chrono::steady_clock::now() - start).count();
        if (rc == WS_OK) *fps = 1.0f / (secs / ((float)n * (float)num_samples));
        uint32_t all_bits = 0, demand = 0;
        for (uint32_t k = 0; k < frames_in_flight && rc == WS_OK; ++k) {  // a rate over frames that dropped entries is not a rate
            uint32_t bits = 0;
            rc = ws_renderer_errors(rs[k], &bits, nullptr, 1);
            all_bits |= bits;
            demand = std::max(demand, ws_internal_renderer_demand(rs[k]));
        }
        if (rc != WS_OK || all_bits == 0) break;
        if (frame_verdict(all_bits, attempt) == FRAME_FAILED || demand == 0) {
            rc = fail(WS_ERR_OVERFLOW, "ws_measure: frames reported device-side errors (tile-entry overflow or a look-back time-out)");
            break;
        }
        for (uint32_t k = 0; k < frames_in_flight; ++k)
            ws_renderer_set_tile_entry_capacity(rs[k], grown_entry_capacity(demand));
    }
    for (uint32_t k = 0; k < frames_in_flight; ++k) {
        if (rs[k]) ws_renderer_destroy(rs[k]);
        if (targets[k]) ws_device_free(ctx, targets[k]);
    }
    return rc;  // (the streams go here, behind their renderers)
}

// ---- view batches: several frames in flight ---------------------------------------------------------------------
// A frame is a pure function of (scene, camera); the views of a batch are independent.  Every frame in flight gets its
// own renderer (private scratch), and its own HIP stream; the scene is shared, read-only.  Small latency-bound kernels
// of one frame (the 12 launches of the depth sort) then overlap the wide kernels of another: 1.5x the frames/s of
// strictly one frame at a time on MI355X.
// HIP maps user streams onto GPU_MAX_HW_QUEUES hardware queues (default 4, the null stream included): export
// GPU_MAX_HW_QUEUES=8 before the process makes its first HIP call, or two of four slots may share a queue and
// serialise (4800 instead of 5600 frames/s on c2).
// SUBMISSION THREADS (round 4).  A frame is 22 launches + a memset, 65-90 us of one host thread; a small scene (10 k ... 250 k
// Gaussians at 800x600) needs less GPU time per frame than that, so one thread enqueueing for four slots is the limit:
// 13.7 k frames/s on the 10 k scene, 10.9 k at 250 k (profiles/r04/mt_enqueue_probe.txt).  The slots are independent -- own
// renderer, own stream -- and HIP launches into different streams from different threads in parallel, so every slot gets a
// worker thread that enqueues ITS frames of a call, in order (the order on each stream, and therefore every frame, is what
// the single thread produces): 31.4 k and 18.8 k frames/s on the same scenes; nothing changes where the GPU is the limit
// (1 M Gaussians at 1080p: 7.16 k either way), so the workers are used for point clouds of at most BATCH_THREADS_MAX_POINTS
// Gaussians (WS_BATCH_THREADS=0 / 1 forces them off / on).  They cost host cores while they run (about one per slot).
constexpr uint32_t BATCH_THREADS_MAX_POINTS = 512u * 1024u;
// HOST RUN-AHEAD (round 5).  A caller that enqueues a thousand frames in one call gets them all queued: the host needs 77 us per
// frame where the GPU needs 140, so it runs ahead until the runtime's queues are full and then WAITS INSIDE THE HIP RUNTIME
// for queue space -- spinning: the enqueue thread at 100 % of a core and a runtime helper thread beside it at 93 %
// (profiles/r05/host_threads.txt; 1.9 cores per rank, 8 ranks on a 16-CPU quota).  Nothing is gained by being a thousand frames
// ahead.  Every slot therefore keeps its host side at most `queue_depth` frames (default 5, ws_context_config::batch_queue_depth; 0 =
// unbounded; measured 2 / 3 / 5: -2 / -1.6 ... -3 / 0 ... -1 % frames/s against unbounded, profiles/r05/host_run_ahead_ab.txt)
// ahead of the device: the compositing kernel of every frame posts the frame's number to pinned host memory when
// it STARTS (ws_internal_renderer_progress: one store by one thread, no event, no extra packet), and before a slot's next
// frame is enqueued the host polls that word, sleeping 20 us between looks -- no runtime call, no spinning (a HIP event wait,
// blocking flavour included, spins for ~200 us before it sleeps, i.e. always at these frame times: measured, 0.99 of a core).
// With 4 slots x 5 frames the GPU always has > 2 ms of work queued; the image stream is unchanged.
struct SlotWindow {
    uint32_t waits = 0;      // times the host had to wait for this slot (ws_view_batch_host_waits)
    bool stalled = false;    // the slot's progress word did not move for 10 s: windowing is off for it, the batch reports WS_ERR_STATE
};
struct ws_view_batch {
    ws_context* ctx = nullptr;
    std::vector<ws_renderer*> renderers;  // destroyed by ws_view_batch_destroy, in front of ...
    std::vector<Stream> streams;          // ... their streams, which go with the batch itself (the member's destructor)
    std::vector<SlotWindow> windows;
    uint32_t queue_depth = 5;
    bool threads_disabled = false;  // a host that could not start the submission threads: this batch enqueues from the caller's
    uint64_t next = 0;  // frames enqueued so far: frame i runs on slot i % frames_in_flight

    // one call's work, shared by the workers (valid while `pending` != 0)
    struct Job {
        const ws_pointcloud* pc = nullptr;
        const ws_splatting_args* views = nullptr;
        void* const* targets = nullptr;
        uint32_t num_views = 0;
        size_t pitch = 0;
        const float* background = nullptr;
        uint64_t first = 0;  // value of `next` at the start of the call
    } job;
    struct Worker {
        std::thread th;
        int rc = WS_OK;
        std::string err;
    };
    std::vector<Worker> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    uint64_t generation = 0;  // bumped per call: a worker runs when it sees a new generation
    uint32_t pending = 0;     // workers still busy with the current generation
    bool quit = false;
};

namespace {
// before a slot's next frame is enqueued: sleep until the slot's host side is fewer than queue_depth frames ahead of the device
int slot_window_admit(ws_view_batch* b, size_t slot) {
    if (b->queue_depth == 0) return WS_OK;
    const ws_renderer* r = b->renderers[slot];
    const uint32_t enq = ws_internal_renderer_frames_enqueued(r);
    uint32_t started = 0;
    if (!ws_internal_renderer_progress(r, &started)) return WS_OK;  // (no mailbox: unbounded, as before)
    SlotWindow& win = b->windows[slot];
    if (win.stalled) return WS_OK;  // (reported once, below; later frames are enqueued unbounded, as without a mailbox)
    bool waited = false;
    int spins = 0;
    // (sequence numbers wrap: compare differences) -- and never wait forever: a frame that failed to launch posts nothing
    for (; (int32_t)(enq - started) >= (int32_t)b->queue_depth && spins < 500000; ++spins) {
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
        waited = true;
        if (!ws_internal_renderer_progress(r, &started)) break;
    }
    if (waited) ++win.waits;
    if (spins >= 500000) {  // 10 s without progress (a lost launch, a device fault): say so instead of proceeding silently
        win.stalled = true;
        return fail(WS_ERR_STATE, "ws_view_batch_render: a slot's frames made no progress for 10 s (device fault or lost launch); "
                                  "the frames enqueued so far are NOT known to have been drawn");
    }
    return WS_OK;
}

void batch_worker(ws_view_batch* b, size_t slot) {
    (void)hipSetDevice(b->ctx->device);
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(b->m);
            b->cv_work.wait(lk, [&] { return b->quit || b->generation != seen; });
            if (b->quit) return;
            seen = b->generation;
        }
        const ws_view_batch::Job& j = b->job;
        const size_t slots = b->renderers.size();
        int rc = WS_OK;
        for (uint32_t i = 0; i < j.num_views && rc == WS_OK; ++i) {
            if ((j.first + i) % slots != slot) continue;
            rc = slot_window_admit(b, slot);
            if (rc == WS_OK) rc = ws_renderer_prepare(b->renderers[slot], j.pc, &j.views[i], b->streams[slot].get());
            if (rc == WS_OK) rc = ws_renderer_render(b->renderers[slot], j.pc, j.background, j.targets[i], j.pitch, b->streams[slot].get());
        }
        b->workers[slot].rc = rc;
        if (rc) b->workers[slot].err = ws_last_error();  // (the error text is thread-local: hand it to the caller)
        {
            std::lock_guard<std::mutex> lk(b->m);
            if (--b->pending == 0) b->cv_done.notify_one();
        }
    }
}
}  // namespace

int ws_view_batch_create(ws_context* ctx, ws_color_format format, uint32_t sh_deg, int compressed,
                         uint32_t frames_in_flight, ws_view_batch** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_view_batch_create: null argument");
    *out = nullptr;
    if (frames_in_flight == 0 || frames_in_flight > 64) return fail(WS_ERR_INVALID, "ws_view_batch_create: frames_in_flight must be 1..64");
    ws_view_batch* b = new (std::nothrow) ws_view_batch();
    if (!b) return fail(WS_ERR_OOM, "ws_view_batch_create: host allocation failed");
    b->ctx = ctx;
    int rc = WS_OK;
    for (uint32_t k = 0; k < frames_in_flight && rc == WS_OK; ++k) {
        ws_renderer* r = nullptr;
        rc = ws_renderer_create(ctx, format, sh_deg, compressed, &r);
        if (rc) break;
        b->renderers.push_back(r);
        Stream s;
        if (s.create() != WS_OK) {
            rc = fail(WS_ERR_HIP, "ws_view_batch_create: hipStreamCreate failed");
            break;
        }
        b->streams.push_back(std::move(s));
    }
    if (rc == WS_OK) {
        if (ctx->batch_queue_depth >= 0) b->queue_depth = (uint32_t)ctx->batch_queue_depth;
        if (b->queue_depth > 64u) b->queue_depth = 64u;
        b->windows.resize(b->renderers.size());
        // several frames in flight: the slots' blends keep the image order of their workgroups (api_renderer.cpp)
        for (ws_renderer* r : b->renderers) ws_internal_renderer_set_throughput_mode(r, b->renderers.size() > 1);
    }
    if (rc != WS_OK) {
        ws_view_batch_destroy(b);
        return rc;
    }
    *out = b;
    return WS_OK;
}

void ws_view_batch_destroy(ws_view_batch* b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> lk(b->m);
        b->quit = true;
    }
    b->cv_work.notify_all();
    for (auto& w : b->workers)
        if (w.th.joinable()) w.th.join();
    (void)hipDeviceSynchronize();
    for (ws_renderer* r : b->renderers) ws_renderer_destroy(r);
    delete b;  // (the streams, behind their renderers)
}

uint32_t ws_view_batch_frames_in_flight(const ws_view_batch* b) { return b ? (uint32_t)b->renderers.size() : 0u; }

int ws_view_batch_render(ws_view_batch* b, const ws_pointcloud* pc, const ws_splatting_args* views, uint32_t num_views,
                         void* const* d_targets, size_t row_pitch_bytes, const float background[4]) {
    if (!b || !pc || (!views && num_views) || (!d_targets && num_views)) return fail(WS_ERR_INVALID, "ws_view_batch_render: null argument");
    const size_t slots = b->renderers.size();
    // WS_BATCH_K1=g: consecutive frames in groups of g share ONE K1 launch (the scene is read once per group instead of
    // once per frame); groups are aligned to the slot ring, so with slots = 2 g one group's K1 overlaps the other's blends
    size_t group = (size_t)b->ctx->batch_k1;
    if (group > 1 && slots % group != 0) group = 1;
    // every slot's frames enqueued by its own thread (see ws_view_batch): small scenes, enough frames to be worth a wake-up
    const int want_threads = b->ctx->batch_threads;
    if (group == 1 && slots >= 2 && num_views >= 2 * slots && want_threads != 0 && !b->threads_disabled &&
        (want_threads > 0 || pc->num_points <= BATCH_THREADS_MAX_POINTS)) {
        bool have_workers = !b->workers.empty();
        if (!have_workers) {
            try {  // (no C++ exception crosses the ABI: a host that cannot start threads keeps the one-thread path)
                std::vector<ws_view_batch::Worker> ws_(slots);
                b->workers.swap(ws_);
                for (size_t s2 = 0; s2 < slots; ++s2) b->workers[s2].th = std::thread(batch_worker, b, s2);
                have_workers = true;
            } catch (...) {
                {
                    std::lock_guard<std::mutex> lk(b->m);
                    b->quit = true;
                }
                b->cv_work.notify_all();
                for (auto& w : b->workers)
                    if (w.th.joinable()) w.th.join();
                b->workers.clear();
                b->quit = false;
                b->threads_disabled = true;  // (this batch keeps the one-thread path; the context is shared state: untouched)
            }
        }
        if (have_workers) {
            {
                std::lock_guard<std::mutex> lk(b->m);
                b->job.pc = pc;
                b->job.views = views;
                b->job.targets = d_targets;
                b->job.num_views = num_views;
                b->job.pitch = row_pitch_bytes;
                b->job.background = background;
                b->job.first = b->next;
                for (auto& w : b->workers) w.rc = WS_OK;
                b->pending = (uint32_t)slots;
                ++b->generation;
            }
            b->cv_work.notify_all();
            {
                std::unique_lock<std::mutex> lk(b->m);
                b->cv_done.wait(lk, [&] { return b->pending == 0; });
            }
            b->next += num_views;
            for (auto& w : b->workers)
                if (w.rc) return fail(w.rc, w.err);
            return WS_OK;
        }
    }
    uint32_t i = 0;
    while (i < num_views) {
        const size_t k = (size_t)(b->next % slots);
        if (group > 1 && k % group == 0 && num_views - i >= group) {
            ws_renderer* rs[K1_MAX_VIEWS];
            hipStream_t ss[K1_MAX_VIEWS];
            for (size_t j = 0; j < group; ++j) {
                rs[j] = b->renderers[k + j];
                ss[j] = b->streams[k + j].get();
            }
            int rc = WS_OK;
            for (size_t j = 0; j < group && rc == WS_OK; ++j) rc = slot_window_admit(b, k + j);
            if (rc) return rc;
            rc = ws_internal_prepare_group(rs, (uint32_t)group, pc, &views[i], ss);
            if (rc == WS_ERR_UNSUPPORTED) {  // (timers, capture, a frame graph ...: every frame its own K1)
                group = 1;
                continue;
            }
            if (rc) return rc;
            for (size_t j = 0; j < group; ++j) {
                rc = ws_renderer_render(rs[j], pc, background, d_targets[i + j], row_pitch_bytes, ss[j]);
                if (rc) return rc;
            }
            i += (uint32_t)group;
            b->next += group;
            continue;
        }
        // a ragged head (the ring is not at a group boundary) or tail, or no grouping: frame by frame
        // a target that an earlier frame of this call still writes must be on the same slot (same stream: ordered)
        int rc = slot_window_admit(b, k);
        if (rc == WS_OK) rc = ws_renderer_prepare(b->renderers[k], pc, &views[i], b->streams[k].get());
        if (rc == WS_OK) rc = ws_renderer_render(b->renderers[k], pc, background, d_targets[i], row_pitch_bytes, b->streams[k].get());
        if (rc) return rc;
        ++b->next;
        ++i;
    }
    return WS_OK;
}

int ws_view_batch_sync(ws_view_batch* b) {
    if (!b) return fail(WS_ERR_INVALID, "ws_view_batch_sync: null batch");
    for (const Stream& s : b->streams) WS_HIP(hipStreamSynchronize(s.get()));
    return WS_OK;
}

int ws_view_batch_errors(ws_view_batch* b, uint32_t* bits, int reset) {
    if (!b || !bits) return fail(WS_ERR_INVALID, "ws_view_batch_errors: null argument");
    *bits = 0;
    for (ws_renderer* r : b->renderers) {
        uint32_t one = 0;
        int rc = ws_renderer_errors(r, &one, nullptr, reset);
        if (rc) return rc;
        *bits |= one;
    }
    return WS_OK;
}

uint32_t ws_view_batch_host_waits(const ws_view_batch* b) {
    uint32_t n = 0;
    if (b)
        for (const SlotWindow& w : b->windows) n += w.waits;
    return n;
}

ws_renderer* ws_view_batch_renderer(ws_view_batch* b, uint32_t slot) {
    return (b && slot < b->renderers.size()) ? b->renderers[slot] : nullptr;
}

int ws_display_composite(ws_context* ctx, const void* d_src, ws_color_format src_format, size_t src_pitch_bytes,
                         uint32_t width, uint32_t height, const float background[4], ws_surface_format dst_format,
                         void* d_dst, size_t dst_pitch_bytes, void* stream) {
    if (!ctx || !d_src || !d_dst || width == 0 || height == 0) return fail(WS_ERR_INVALID, "ws_display_composite: bad argument");
    if (src_pitch_bytes < texel_bytes(src_format) * width || dst_pitch_bytes < (size_t)width * 4 ||
        (src_pitch_bytes % texel_bytes(src_format)) != 0 || (dst_pitch_bytes % 4) != 0)
        return fail(WS_ERR_INVALID, "ws_display_composite: row pitch does not fit the format");
    if (dst_format != WS_SURFACE_RGBA8_UNORM && dst_format != WS_SURFACE_BGRA8_UNORM)
        return fail(WS_ERR_INVALID, "ws_display_composite: unknown surface format");
    const float zero[4] = {0, 0, 0, 0};
    return launch_display(d_src, (int)src_format, src_pitch_bytes, width, height, background ? background : zero,
                          (int)dst_format, d_dst, dst_pitch_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
