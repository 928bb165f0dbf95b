"""CPU test of who owns the runtime's handles (web-splat_amd/csrc/hip_handles.h: events, streams, graphs, executable graphs, pinned
words), of the renderer's mailbox over the pinned words (api_state.h) and of the frame graph's key and ring arithmetic
(frame_graph.h).  No GPU test may make a create fail, so the ownership code runs here, as tests/test_frame_scratch.py runs the
device buffers': a stand-alone program defines the functions the header reaches the runtime through over counters -- live handles
per kind, "the k-th create from now fails" -- and is built with the address and undefined-behaviour sanitizers (their runtimes
linked into it).  Every handle is a heap block of its own, so a leak, a double destroy or a use after destroy ends the child
process with a non-zero status and a line on stderr, as a wrong count does."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include "api_state.h"
using namespace ws;

enum Kind { EVENT, STREAM, GRAPH, EXEC, PINNED, KINDS };
static long g_live[KINDS] = {}, g_destroyed = 0, g_fail_at = 0;  // g_fail_at = k: the k-th create from now fails (0: none)
static int g_fail_code = WS_ERR_HIP;
static long live_total() { long t = 0; for (long l : g_live) t += l; return t; }

// a handle is a heap block of its own: one byte for an event (its timing flag), a stream, a graph and an executable graph
template <typename H>
static int make(Kind k, H* h, unsigned char tag) {
    *h = nullptr;
    if (g_fail_at && --g_fail_at == 0) return g_fail_code;
    unsigned char* p = (unsigned char*)malloc(1);
    *p = tag;
    *h = reinterpret_cast<H>(p);
    ++g_live[k];
    return WS_OK;
}
template <typename H>
static void drop(Kind k, H h) {
    if (!h) { fprintf(stderr, "destroy(nullptr) of kind %d\n", (int)k); exit(2); }
    free(reinterpret_cast<void*>(h));
    --g_live[k], ++g_destroyed;
}
int ws::event_create(hipEvent_t* e, bool timing) { return make(EVENT, e, timing ? 1 : 0); }
void ws::event_destroy(hipEvent_t e) { drop(EVENT, e); }
int ws::stream_create(hipStream_t* s) { return make(STREAM, s, 2); }
void ws::stream_destroy(hipStream_t s) { drop(STREAM, s); }
int ws::graph_end_capture(hipGraph_t* g, hipStream_t capturing) {
    if (*reinterpret_cast<unsigned char*>(capturing) != 2) { fprintf(stderr, "end of capture: not a live stream\n"); exit(2); }
    return make(GRAPH, g, 3);
}
void ws::graph_destroy(hipGraph_t g) { drop(GRAPH, g); }
int ws::graph_exec_create(hipGraphExec_t* x, hipGraph_t g) {
    if (*reinterpret_cast<unsigned char*>(g) != 3) { fprintf(stderr, "instantiate: not a live graph\n"); exit(2); }
    return make(EXEC, x, 4);
}
void ws::graph_exec_destroy(hipGraphExec_t x) { drop(EXEC, x); }
int ws::pinned_words_create(uint32_t** host, uint32_t** dev, size_t count) {
    *host = *dev = nullptr;
    if (g_fail_at && --g_fail_at == 0) return g_fail_code;
    *host = *dev = (uint32_t*)calloc(count, sizeof(uint32_t));  // (one address space here)
    ++g_live[PINNED];
    return WS_OK;
}
void ws::pinned_words_destroy(uint32_t* host) { drop(PINNED, host); }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// what every owner kind does alike; a... = the arguments of its create
template <typename O, typename... A>
static void check_owner(Kind k, A... a) {
    const long others = live_total();
    long& live = g_live[k];
    CHECK(live == 0);
    {
        O x;
        CHECK(!x.get());
        x.reset();                                   // of an empty owner
        CHECK(x.create(a...) == WS_OK && x.get() && live == 1);
        CHECK(x.create(a...) == WS_OK && x.get() && live == 1);   // over a held handle: released first
        O y(std::move(x));                           // move construction
        CHECK(!x.get() && y.get() && live == 1);
        O z;
        CHECK(z.create(a...) == WS_OK && live == 2 && z.get() != y.get());
        const auto kept = y.get();
        z = std::move(y);                            // move assignment onto a full owner
        CHECK(!y.get() && z.get() == kept && live == 1);
        O& self = z;
        z = std::move(self);                         // onto itself
        CHECK(z.get() == kept && live == 1);
        z.reset();
        z.reset();                                   // twice
        CHECK(!z.get() && live == 0);
        for (int code : {WS_ERR_HIP, WS_ERR_OOM}) {
            g_fail_at = 1, g_fail_code = code;
            CHECK(z.create(a...) == code && !z.get() && live == 0 && g_fail_at == 0);  // a failed create leaves it empty, and says why
            CHECK(z.create(a...) == WS_OK && live == 1);
            g_fail_at = 1;
            CHECK(z.create(a...) == code && !z.get() && live == 0);                    // ... the held handle is gone too (released first)
        }
        CHECK(z.create(a...) == WS_OK && x.create(a...) == WS_OK && live == 2);        // a moved-from owner is an empty owner
    }
    CHECK(live == 0 && live_total() == others);
}

int main() {
    check_owner<Event>(EVENT, true);
    check_owner<Event>(EVENT, false);
    check_owner<Stream>(STREAM);
    {
        Stream s;
        CHECK(s.create() == WS_OK);
        check_owner<Graph>(GRAPH, s.get());
        Graph g;
        CHECK(g.create(s.get()) == WS_OK);
        check_owner<GraphExec>(EXEC, g.get());
    }
    check_owner<PinnedWords>(PINNED, (size_t)4);
    CHECK(live_total() == 0);

    {   // the flag of an event arrives; pinned words are zeroed, as many as asked for, and known by both addresses
        Event timed, untimed;
        CHECK(timed.create(true) == WS_OK && untimed.create(false) == WS_OK);
        CHECK(*reinterpret_cast<unsigned char*>(timed.get()) == 1 && *reinterpret_cast<unsigned char*>(untimed.get()) == 0);
        PinnedWords w;
        CHECK(!w.get() && !w.dev() && w.count() == 0);
        CHECK(w.create(4) == WS_OK && w.get() && w.dev() == w.get() && w.count() == 4);
        for (int i = 0; i < 4; ++i) CHECK(w.get()[i] == 0u);
        w.get()[3] = 7u;
        PinnedWords v(std::move(w));
        CHECK(!w.get() && !w.dev() && w.count() == 0 && v.count() == 4 && v.dev()[3] == 7u && g_live[PINNED] == 1);
    }
    CHECK(live_total() == 0);

    {   // six events, the fourth create fails (ws_renderer_create): leaving the scope releases exactly three
        g_destroyed = 0;
        {
            Event ev[6];
            g_fail_at = 4, g_fail_code = WS_ERR_HIP;
            int rc = WS_OK, made = 0;
            for (Event& e : ev) {
                if ((rc = e.create(true))) break;
                ++made;
            }
            CHECK(rc == WS_ERR_HIP && made == 3 && g_live[EVENT] == 3 && g_destroyed == 0);
            CHECK(ev[2].get() && !ev[3].get() && !ev[4].get() && !ev[5].get());
        }
        CHECK(g_destroyed == 3 && live_total() == 0);
    }

    {   // a ring of four (executable graph, event) pairs, the third instantiate fails (FrameGraph): everything goes at scope exit
        g_destroyed = 0;
        {
            struct Slot { GraphExec exec; Event done; };
            Stream s;
            Graph graph;           // in front of the ring, as FrameGraph declares them: the executable graphs go first
            Slot ring[4];
            CHECK(s.create() == WS_OK && graph.create(s.get()) == WS_OK);
            g_fail_at = 5, g_fail_code = WS_ERR_OOM;  // exec, event, exec, event, EXEC
            int rc = WS_OK, made = 0;
            for (Slot& sl : ring) {
                if ((rc = sl.exec.create(graph.get())) || (rc = sl.done.create(false))) break;
                ++made;
            }
            CHECK(rc == WS_ERR_OOM && made == 2 && g_live[EXEC] == 2 && g_live[EVENT] == 2 && g_live[GRAPH] == 1 && !ring[2].exec.get() && !ring[2].done.get());
        }
        CHECK(g_destroyed == 6 && live_total() == 0);
    }

    {   // KernelMarks' events: a round of creates that failed half way is made whole by the next round, nothing left over
        g_destroyed = 0;
        {
            KernelMarks km;
            g_fail_at = 10, g_fail_code = WS_ERR_HIP;
            int n = 0, rc = WS_OK;
            for (Event& e : km.ev) { if ((rc = e.create(true))) break; ++n; }
            CHECK(rc == WS_ERR_HIP && n == 9 && g_live[EVENT] == 9);
            for (Event& e : km.ev) CHECK(e.create(true) == WS_OK);
            CHECK(g_live[EVENT] == KernelMarks::MAX + 1 && g_destroyed == 9);
        }
        CHECK(live_total() == 0);
    }

    {   // the mailbox: an empty one gives every reader its "no mailbox" answer; a present one reads what the device posted
        Mailbox none;
        CHECK(!none.present() && none.demand() == 0u && none.span_class() == 0u && none.dev() == nullptr);
        g_fail_at = 1, g_fail_code = WS_ERR_OOM;
        CHECK(none.create() == WS_ERR_OOM && !none.present() && none.demand() == 0u && none.span_class() == 0u && !none.dev());
        Mailbox mb;
        CHECK(mb.create() == WS_OK && mb.present() && mb.dev() && mb.demand() == 0u && mb.started_seq() == 0u && mb.span_class() == 0u);
        mb.dev()[0] = 123456u, mb.dev()[1] = 42u, mb.dev()[2] = 2u;   // (the blend's three stores)
        CHECK(mb.demand() == 123456u && mb.started_seq() == 42u && mb.span_class() == 2u);
        mb.clear_demand();
        CHECK(mb.demand() == 0u && mb.dev()[0] == 0u && mb.started_seq() == 42u && mb.span_class() == 2u);
        Mailbox moved(std::move(mb));
        CHECK(!mb.present() && mb.demand() == 0u && moved.present() && moved.started_seq() == 42u && g_live[PINNED] == 1);
    }
    CHECK(live_total() == 0);

    {   // the frame graph's key differs when any ONE of its three members does; ring slots come back in ring order
        const ws_pointcloud* const pa = reinterpret_cast<const ws_pointcloud*>(0x1000);
        const ws_pointcloud* const pb = reinterpret_cast<const ws_pointcloud*>(0x2000);
        const FrameGraphKey k{pa, 7, 1};
        CHECK(k == (FrameGraphKey{pa, 7, 1}));
        CHECK(!(k == FrameGraphKey{pb, 7, 1}) && !(k == FrameGraphKey{pa, 8, 1}) && !(k == FrameGraphKey{pa, 7, 0}));
        CHECK(!(k == FrameGraphKey{pa, 7ull + (1ull << 32), 1}));   // (the generation is compared at its full width)
        CHECK(!(k == FrameGraphKey()) && FrameGraphKey() == FrameGraphKey());
        FrameGraph empty;
        CHECK(!empty.matches(k) && !empty.matches(FrameGraphKey()) && empty.depth_bits() == 0);  // no graph matches nothing, its own default key included
        for (uint32_t n = 0; n < 3 * (uint32_t)GRAPH_RING; ++n) CHECK(graph_ring_slot(n) == n % 4u && graph_ring_slot(n) < (uint32_t)GRAPH_RING);
        CHECK(graph_ring_slot(0xFFFFFFFFu) == 3u && graph_ring_slot(0xFFFFFFFFu + 1u) == 0u);    // the launch count wraps at a ring boundary
        static_assert(GRAPH_RING == 4 && (0x100000000ull % GRAPH_RING) == 0, "ring");
    }
    CHECK(live_total() == 0);
    printf("ok\n");
    return 0;
}
"""


def test_ownership_under_the_sanitizers(tmp_path):
    src, exe = tmp_path / "hip_handles.cpp", tmp_path / "hip_handles"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-self-move",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-isystem", os.path.join(ROCM, "include"), str(src), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout == "ok\n" and run.stderr == "", (run.returncode, run.stdout, run.stderr)
