// frame_graph.cpp -- capture, ring and launch of a frame's graph (frame_graph.h)
#include "frame_graph.h"

#include <string>
#include <vector>

namespace ws {

void FrameGraph::reset() {
    for (Slot& s : ring_) s = Slot();
    graph_.reset();
    k1_node_ = nullptr;
    k1_params_ = hipKernelNodeParams{};
    key_ = FrameGraphKey();
    launches_ = 0;
    valid_ = false;
    arrays_ = FrameArrays();
    depth_bits_ = 0;
}

int FrameGraph::capture(const FrameGraphKey& key, hipStream_t stream, const void* k1_func, int depth_bits,
                        const std::function<int(FrameArrays*)>& enqueue) {
    reset();
    WS_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    FrameArrays arrays;
    const int rc = enqueue(&arrays);
    const std::string why = rc ? ws_last_error() : "";
    const int captured = graph_.create(stream);
    if (rc) {  // the enqueue's own failure is the one reported
        reset();
        set_error(why);
        return rc;
    }
    if (captured) return captured;
    if (const int ring = make_ring(k1_func)) {
        reset();
        return ring;
    }
    key_ = key;
    arrays_ = arrays;  // (with: did the captured frame run k_blend_order?)
    depth_bits_ = depth_bits;
    valid_ = true;
    return WS_OK;
}

int FrameGraph::make_ring(const void* k1_func) {
    const hipGraph_t graph = graph_.get();
    size_t nn = 0;
    WS_HIP(hipGraphGetNodes(graph, nullptr, &nn));
    std::vector<hipGraphNode_t> nodes(nn);
    WS_HIP(hipGraphGetNodes(graph, nodes.data(), &nn));
    for (size_t i = 0; i < nn && !k1_node_; ++i) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams kn;
        if (hipGraphKernelNodeGetParams(nodes[i], &kn) != hipSuccess) continue;
        if (kn.func == k1_func) {
            k1_node_ = nodes[i];
            k1_params_ = kn;
        }
    }
    if (!k1_node_) return fail(WS_ERR_HIP, "ws_renderer_prepare: the preprocess kernel was not found in the captured frame graph");
    for (Slot& s : ring_) {
        WS_TRY(s.exec.create(graph));
        WS_TRY(s.done.create(false));
    }
    return WS_OK;
}

int FrameGraph::launch(hipStream_t stream, void** k1_args, FrameArrays* arrays) {
    Slot& s = ring_[graph_ring_slot(launches_++)];
    if (s.used) WS_HIP(hipEventSynchronize(s.done.get()));  // an earlier launch of this executable graph must have run
    hipKernelNodeParams np = k1_params_;
    np.kernelParams = k1_args;
    np.extra = nullptr;
    WS_HIP(hipGraphExecKernelNodeSetParams(s.exec.get(), k1_node_, &np));
    WS_HIP(hipGraphLaunch(s.exec.get(), stream));
    WS_HIP(hipEventRecord(s.done.get(), stream));
    s.used = true;
    *arrays = arrays_;  // what THIS graph's frames write, whatever a launch-by-launch frame left behind
    return WS_OK;
}

}  // namespace ws
