// hip_handles.h -- the owners of the runtime's other resources: an event, a stream, a captured graph, an executable graph and a
// block of pinned mapped words.  What device_buf.h is for device memory: every object behind the C ABI holds these as members, so a
// handle's destructor IS its free list and an early return releases what the function created so far.  The destructors release
// WITHOUT synchronising: whoever lets a resource go while a launch may still use it synchronises first, in the caller (DESIGN.md
// section 3, "Device memory").  Plain C++ but for the runtime's opaque handle types: the runtime is reached only through the
// functions below, which ws_api.cpp defines over HIP and a CPU test (tests/test_hip_handles.py) over counters.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "websplat.h"

// (the runtime's own declarations of its opaque handles, hip_runtime_api.h)
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipGraph* hipGraph_t;
typedef struct hipGraphExec* hipGraphExec_t;

#pragma GCC visibility push(hidden)  // (between the library's units: not among its dynamic symbols)
namespace ws {

// Each create: WS_OK, or the code of the failure with ws_last_error set; the handle is null then.  Each destroy: a handle != nullptr.
int event_create(hipEvent_t* e, bool timing);
void event_destroy(hipEvent_t e);
int stream_create(hipStream_t* s);  // non-blocking
void stream_destroy(hipStream_t s);
int graph_end_capture(hipGraph_t* g, hipStream_t capturing);  // a graph is made by ending the capture of a stream
void graph_destroy(hipGraph_t g);
int graph_exec_create(hipGraphExec_t* x, hipGraph_t g);
void graph_exec_destroy(hipGraphExec_t x);
int pinned_words_create(uint32_t** host, uint32_t** dev, size_t count);  // zeroed; *dev: the device's address of *host
void pinned_words_destroy(uint32_t* host);

template <typename H, void (*Destroy)(H)>
class Handle {  // move-only; default-constructed = empty
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Handle() { reset(); }
    void reset() {
        if (h_) Destroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }

protected:
    // after releasing what the owner holds; a failed create leaves it empty
    template <typename... A>
    int create_by(int (*make)(H*, A...), A... a) {
        reset();
        H h = nullptr;
        if (const int rc = make(&h, a...)) return rc;
        h_ = h;
        return WS_OK;
    }

private:
    H h_ = nullptr;
};

struct Event : Handle<hipEvent_t, event_destroy> {
    int create(bool timing) { return create_by(event_create, timing); }
};
struct Stream : Handle<hipStream_t, stream_destroy> {
    int create() { return create_by(stream_create); }
};
struct Graph : Handle<hipGraph_t, graph_destroy> {
    int create(hipStream_t capturing) { return create_by(graph_end_capture, capturing); }  // ends the stream's capture either way
};
struct GraphExec : Handle<hipGraphExec_t, graph_exec_destroy> {
    int create(hipGraph_t g) { return create_by(graph_exec_create, g); }
};

class PinnedWords {  // host memory the device writes and the host reads without a runtime call
public:
    PinnedWords() = default;
    PinnedWords(PinnedWords&& o) noexcept : host_(o.host_), dev_(o.dev_), n_(o.n_) { o.host_ = o.dev_ = nullptr, o.n_ = 0; }
    PinnedWords& operator=(PinnedWords&& o) noexcept {
        if (this != &o) {
            reset();
            host_ = o.host_, dev_ = o.dev_, n_ = o.n_;
            o.host_ = o.dev_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~PinnedWords() { reset(); }
    int create(size_t count) {
        reset();
        uint32_t *h = nullptr, *d = nullptr;
        if (const int rc = pinned_words_create(&h, &d, count)) return rc;
        host_ = h, dev_ = d, n_ = count;
        return WS_OK;
    }
    void reset() {
        if (host_) pinned_words_destroy(host_);
        host_ = dev_ = nullptr, n_ = 0;
    }
    uint32_t* get() const { return host_; }  // the host's address
    uint32_t* dev() const { return dev_; }   // the device's address of the same words
    size_t count() const { return n_; }

private:
    uint32_t *host_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;
};

}  // namespace ws
#pragma GCC visibility pop
