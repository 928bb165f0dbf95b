// api_state.h -- what the translation units of the C ABI share: the renderer with its prepared frame, and how a handle's data is
// read back and a handle destroyed.  Host only: included by ws_api.cpp (the object model) and by api_attrib.cpp, api_metrics.cpp
// and api_refit.cpp (the passes that read a prepared frame, and the objects they fill), never by a .hip.
#pragma once

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

// Where the prepared frame's arrays are: one value, so that the frame graph's capture and replay cannot forget a member.
struct FrameArrays {
    // the depth sort's result: vals = the draw-ordered store indices, aux = their footprint words; the *_skipped members are
    // where they are when the sort's last pass had nothing to do (FrameCounters::depth_skip_top, decided on the device per
    // frame), nullptr: this frame's sort cannot skip
    ws::SortResult depth;
    uint32_t* entries = nullptr;     // the tile-sorted entry values (store indices)
    bool blend_order_valid = false;  // the frame wrote FrameScratch::blend_order (it ran k_blend_order)
};

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

struct ws_renderer {
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
    // The frame's launch sequence of prepare() (memset + 21 kernels), captured once per (point cloud, scratch) and replayed:
    // only K1's arguments change from frame to frame (camera / settings uniforms, epoch).  A ring of executable graphs,
    // because updating an executable graph's kernel arguments while an earlier launch of it has not run yet would change
    // that earlier frame: slot i is reused only after the event recorded behind its last launch has completed.
    static constexpr int GRAPH_RING = 4;
    struct FrameGraph {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec[GRAPH_RING] = {};
        hipEvent_t done[GRAPH_RING] = {};
        bool used[GRAPH_RING] = {};
        hipGraphNode_t k1_node = nullptr;
        hipKernelNodeParams k1_params{};
        const ws_pointcloud* pc = nullptr;
        uint64_t generation = 0;   // scratch generation the graph was captured for
        uint32_t next = 0;
        bool valid = false;
        FrameArrays arrays;              // of the captured frame
        int order_mode = 0;              // decide_blend_order() of the captured frame: a change re-captures
        int depth_bits = 0;              // != 0 while the graph is valid: the digit width its depth sort was captured with
    } fg;

    // ---- the last prepared frame ----
    PreparedFrame frame;
    int order_mode = 0;              // decide_blend_order() of the last prepare(): a captured graph replays only under its own

    // ---- error words and progress: they outlive a failed prepare() and a new scratch (ws_renderer_errors) ----
    hipStream_t last_stream = nullptr;
    ws::DeviceBuf<uint32_t> sticky;      // two device words that survive the per-frame memset (ws_renderer_errors): [0] error bits
                                     // of all frames since the last reset, [1] the largest entries_needed of an overflowed frame
    uint32_t needed_seen = 0;        // host copy of [1]: the automatic entry capacity grows to it at the next prepare()
    uint32_t* demand_mailbox = nullptr;      // FOUR pinned host words the blend posts to (device-visible address: demand_mailbox_dev):
    uint32_t* demand_mailbox_dev = nullptr;  //   [0] the demand [1] above -- prepare() reads it without a sync, so the capacity grows
                                             //   without anyone polling; [1] the number of the last frame whose blend has started;
                                             //   [2] depth_span_class of that frame -> the next frame's digit width
    uint32_t frames_enqueued = 0;            // render() calls so far (the sequence number the blend posts)

    // ---- instrumentation ----
    ws::DeviceBuf<unsigned long long> frame_trace;  // [frames][4]: {K1 start, K1 end, blend start, blend end} per frame (ws_renderer_enable_frame_trace)
    uint32_t trace_count = 0;        // slots handed out so far
    bool timers = false;
    ws::KernelMarks marks;               // per-kernel events, timers level 2
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_group[2] = {nullptr, nullptr};  // grouped prepare of a view batch: "arena cleared" / "shared K1 done"
    bool ev_prepare_valid = false, ev_render_valid = false;
};
