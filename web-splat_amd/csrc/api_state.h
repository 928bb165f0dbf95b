// api_state.h -- what the translation units of the C ABI share: the renderer with its prepared frame, and how a handle's data is
// read back and a handle destroyed.  Host only: included by the units of the object model (api_pointcloud.cpp, api_renderer.cpp,
// api_readback.cpp, api_sorter.cpp) and by api_attrib.cpp, api_metrics.cpp and api_refit.cpp (the passes that read a prepared frame,
// and the objects they fill), never by a .hip.
#pragma once

#include "frame_graph.h"
#include "frame_scratch.h"
#include "ws_internal.h"

namespace ws {

// Device -> host read-back ORDERED ON THE RENDERER'S OWN STREAM (then waited for): the library never touches the legacy
// NULL stream for a frame's data.  (Besides the device-wide implicit synchronisation a NULL-stream copy brings, a
// hipMemcpy on the NULL stream between two launches of a captured frame graph made the next launch of an already
// used executable graph fault on ROCm 7.2 -- found by scripts/sweep.py, which reads frame_stats() between frames.)
static inline int copy_d2h(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return WS_OK;
    WS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    WS_HIP(hipStreamSynchronize(stream));
    return WS_OK;
}

// How the ABI destroys a handle whose buffers a launch may still read, and how a creator drops one it could not finish:
// behind a device sync (DeviceBuf frees without one)
struct SyncedDelete {
    template <typename H>
    void operator()(H* h) const {
        if (!h) return;
        (void)hipDeviceSynchronize();
        delete h;
    }
};

}  // namespace ws

// The last prepared frame.  Reset as a whole wherever it stops being one: every reader asks `prepared` first.
struct PreparedFrame {
    bool prepared = false;
    const ws_pointcloud* pc = nullptr;
    bool contrib = false;            // K1 kept the source indices (ws_renderer_enable_contrib was on)
    bool depth = false;              // K1 wrote the z plane (ws_renderer_enable_depth was on)
    float znear = 0.0f, zfar = 0.0f; // K1Params::znear / zfar (the composite's NDC occluder)
    float cam_pos[3] = {0.0f, 0.0f, 0.0f};  // view_inv[12..14] of K1's camera uniform: where K1 takes the SH direction from
    uint32_t max_sh_deg = 0;         // of K1's settings uniform (both read by ws_renderer_accumulate_sh_gradient)
    ws_camera_uniform cam{};         // K1's two uniforms as the frame was prepared with them (read by
    ws_settings_uniform settings{};  //   ws_renderer_accumulate_geometry_gradient, which takes the sums back through K1's projection)
    FrameArrays arrays;
    float* k1_depths = nullptr;      // the z plane the prepare() in progress writes (nullptr: depth off)
    unsigned long long* trace_slot = nullptr;  // the frame's slot of ws_renderer::frame_trace (nullptr: not traced)
};

// FOUR pinned host words the blend posts to, read here without a sync and without a runtime call.  A renderer whose pinned
// allocation failed has an empty one: every reader below then gives its "no mailbox" answer.
class __attribute__((visibility("hidden"))) Mailbox {
public:
    int create() { return words_.create(4); }
    bool present() const { return words_.get() != nullptr; }
    // [0] the largest entries_needed of an overflowed frame (ws_renderer::sticky [1]) -- prepare() reads it, so the automatic
    // capacity grows without anyone polling (0: none, or no mailbox)
    uint32_t demand() const { return present() ? word(0) : 0u; }
    void clear_demand() { word(0) = 0u; }  // present() only
    // [1] the number of the last frame whose blend has started (present() only: ws_internal_renderer_progress)
    uint32_t started_seq() const { return word(1); }
    // [2] FrameCounters::depth_span_class of that frame -> the next frame's digit width (0: none yet, or no mailbox)
    uint32_t span_class() const { return present() ? word(2) : 0u; }
    // what the blend is given: the device's address of [0], the progress word behind it (nullptr: no mailbox)
    uint32_t* dev() const { return words_.dev(); }

private:
    volatile uint32_t& word(int k) const { return *reinterpret_cast<volatile uint32_t*>(words_.get() + k); }
    ws::PinnedWords words_;
};

struct __attribute__((visibility("hidden"))) ws_renderer {  // (its destructor is the renderer's free list: not a dynamic symbol)
    // ---- fixed configuration and switches ----
    ws_context* ctx = nullptr;
    ws_color_format format = WS_FORMAT_RGBA32_FLOAT;
    uint32_t sh_deg = 3;
    bool compressed = false;
    uint64_t entry_cap_request = 0;
    int blend_mode = WS_BLEND_FAST;  // ws_renderer_set_blend_mode
    bool capture = false;
    bool contrib = false;            // ws_renderer_enable_contrib: K1 keeps the source indices from the next prepare() on
    bool depth = false;              // ws_renderer_enable_depth: K1 writes the z plane from the next prepare() on
    bool blend_timing = false;       // ws_renderer_enable_blend_timing: render() launches the time-stamped blend
    bool throughput_mode = false;    // this renderer runs beside others (a slot of a view batch with frames in flight):
                                     //   its blend keeps the image order of its workgroups (see ws_renderer_render)

    // ---- the scratch, (re)created when num_points, the viewport or the entry capacity changes (renderer.rs:200-211) ----
    ws::FrameScratch scratch;
    uint32_t cap_points = 0, vw = 0, vh = 0;  // what it was made for
    ws::FramePlan plan{};                // of the last prepare(): the scratch is sized by it, the frame's launches are filled from it (frame_plan.h)
    uint32_t epoch = 0;              // look-back epoch of the last frame (lookback.h); 0 with fresh (zeroed) status arrays
    uint64_t scratch_generation = 0;
    ws::FrameGraph fg;               // the frame's launch sequence of prepare(), captured and replayed (frame_graph.h); dropped by
                                     //   renderer_free_graph alone (api_renderer.cpp)

    // ---- the last prepared frame ----
    PreparedFrame frame;
    int order_mode = 0;              // decide_blend_order() of the last prepare(): a captured graph replays only under its own

    // ---- error words and progress: they outlive a failed prepare() and a new scratch (ws_renderer_errors) ----
    hipStream_t last_stream = nullptr;
    ws::DeviceBuf<uint32_t> sticky;      // two device words that survive the per-frame memset (ws_renderer_errors): [0] error bits
                                     // of all frames since the last reset, [1] the largest entries_needed of an overflowed frame
    uint32_t needed_seen = 0;        // host copy of [1]: the automatic entry capacity grows to it at the next prepare()
    Mailbox mailbox;                 // what the blend posts to the host (optional: empty without pinned memory)
    uint32_t frames_enqueued = 0;    // render() calls so far (the sequence number the blend posts)

    // ---- instrumentation ----
    ws::DeviceBuf<unsigned long long> frame_trace;  // [frames][4]: {K1 start, K1 end, blend start, blend end} per frame (ws_renderer_enable_frame_trace)
    uint32_t trace_count = 0;        // slots handed out so far
    bool timers = false;
    ws::KernelMarks marks;               // per-kernel events, timers level 2
    ws::Event ev[6];                     // the stage timers (ws_renderer_stage_times), created with the renderer
    ws::Event ev_group[2];               // grouped prepare of a view batch: "arena cleared" / "shared K1 done"; created there, on first use
    bool ev_prepare_valid = false, ev_render_valid = false;
};
