// frame_graph.h -- the captured launch sequence of a frame.  prepare()'s memset + 21 kernels are captured once per (point cloud,
// scratch, blend order) and replayed: only K1's arguments change from frame to frame (camera / settings uniforms, epoch), so a frame
// costs the host one kernel-argument update and one hipGraphLaunch.  A RING of executable graphs, because updating an executable
// graph's kernel arguments while an earlier launch of it has not run yet would change that earlier frame: slot i is reused only
// after the event recorded behind its last launch has completed.  The object owns its handles (hip_handles.h) and knows nothing of
// the renderer: what a frame enqueues comes in as a callable, the policy of when to drop the graph stays with the renderer
// (api_renderer.cpp renderer_free_graph).  Host only.
#pragma once

#include <functional>

#include "ws_internal.h"

// Where the prepared frame's arrays are: one value, so that the frame graph's capture and replay cannot forget a member.
struct FrameArrays {
    // the depth sort's result: vals = the draw-ordered store indices, aux = their footprint words; the *_skipped members are
    // where they are when the sort's last pass had nothing to do (FrameCounters::depth_skip_top, decided on the device per
    // frame), nullptr: this frame's sort cannot skip
    ws::SortResult depth;
    uint32_t* entries = nullptr;     // the tile-sorted entry values (store indices)
    bool blend_order_valid = false;  // the frame wrote FrameScratch::blend_order (it ran k_blend_order)
};

namespace ws {

// What a captured graph was captured for: one value, compared as a whole.  The frame about to be prepared replays the graph only
// under an equal key; anything else re-captures.
struct FrameGraphKey {
    const ws_pointcloud* pc = nullptr;
    uint64_t generation = 0;  // of the renderer's scratch (it also counts K1's change of form: ws_renderer_enable_depth)
    int order_mode = 0;       // decide_blend_order() of the frame
};
inline bool operator==(const FrameGraphKey& a, const FrameGraphKey& b) {
    return a.pc == b.pc && a.generation == b.generation && a.order_mode == b.order_mode;
}

constexpr int GRAPH_RING = 4;
// the ring slot of a graph's n-th launch (n = 0, 1, ...)
inline uint32_t graph_ring_slot(uint32_t n) { return n % (uint32_t)GRAPH_RING; }

class __attribute__((visibility("hidden"))) FrameGraph {  // (between the ABI's units: not among the library's dynamic symbols)
public:
    bool matches(const FrameGraphKey& key) const { return valid_ && key_ == key; }
    // != 0 while a graph stands: the digit width its depth sort was captured with
    int depth_bits() const { return depth_bits_; }

    // Captures what `enqueue` enqueues on `stream` (it fills in where its frame's arrays are) and makes the ring ready for launch:
    // K1's node is the one kernel node whose function is k1_func.  The capture is ended whatever enqueue answers, and its answer is
    // the one returned.  On any failure the object is empty.
    int capture(const FrameGraphKey& key, hipStream_t stream, const void* k1_func, int depth_bits,
                const std::function<int(FrameArrays*)>& enqueue);
    // One frame: the next ring slot, K1's arguments patched to k1_args.  *arrays: what the captured frame's launches write.
    int launch(hipStream_t stream, void** k1_args, FrameArrays* arrays);
    void reset();  // (no sync, like every owner)

private:
    int make_ring(const void* k1_func);

    struct Slot {
        GraphExec exec;
        Event done;         // recorded behind the slot's last launch
        bool used = false;
    };
    Graph graph_;             // declared in front of the ring: the executable graphs go first, then the graph they were made from
    Slot ring_[GRAPH_RING];
    hipGraphNode_t k1_node_ = nullptr;
    hipKernelNodeParams k1_params_{};
    FrameGraphKey key_;
    uint32_t launches_ = 0;
    bool valid_ = false;
    FrameArrays arrays_;  // of the captured frame
    int depth_bits_ = 0;
};

}  // namespace ws
