"""CPU test of who owns the device memory (web-splat_amd/csrc/device_buf.h, frame_scratch.h).  No GPU test may make an allocation
fail, so the ownership code runs here: a stand-alone program with its own device_alloc / device_free over malloc / free -- the two
functions the headers reach the runtime through -- counts live blocks, fails the k-th allocation on request, and is built with the
address and undefined-behaviour sanitizers (their runtimes linked into it).  It runs as a child process; a leak, a double free, a use after free or a wrong count
ends it with a non-zero status and a line on stderr."""
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
#include "frame_scratch.h"
using namespace ws;

static long g_live = 0, g_calls = 0, g_fail_at = 0;  // g_fail_at = k: the k-th call from now fails (0: none)
int ws::device_alloc(void** p, size_t bytes) {
    *p = nullptr;
    ++g_calls;
    if (g_fail_at && --g_fail_at == 0) return WS_ERR_OOM;
    *p = malloc(bytes);
    if (!*p) return WS_ERR_OOM;
    memset(*p, 0xA5, bytes);  // (every byte of the block is the owner's: the sanitizer sees an overstated size)
    ++g_live;
    return WS_OK;
}
void ws::device_free(void* p) {
    if (!p) { fprintf(stderr, "device_free(nullptr)\n"); exit(2); }
    free(p);
    --g_live;
}
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static ScratchLayout layout_of(uint32_t n, uint32_t vw, uint32_t vh, bool wide, bool fat) {
    FramePlanRequest p{};
    p.tile_qw = p.tile_qh = 4, p.bin_request = BIN_AUTO, p.blend_tpw_log2 = p.blend_split = -1, p.num_cus = 256, p.depth_skip_top = 1;
    p.num_points = n, p.viewport[0] = vw, p.viewport[1] = vh, p.order_mode = 1, p.tile_sort_wide = wide;
    p.entry_cap_request = wide ? (SORT_SMALL_MAX + 1u) : 1000u;  // (the single-pass sort's rows need the large sort tile)
    ScratchRequest q{};
    q.plan = frame_plan(p), q.num_points = n, q.vw = vw, q.vh = vh, q.fat_depth_sort = fat;
    q.k1_blocks = (n + 2047) / 2048, q.bin_blocks = (n + 1023) / 1024, q.order_blocks = q.plan.ntiles, q.fat_status_words = 4096;
    return scratch_layout(q);
}
static bool empty(const FrameScratch& s) {
    return !s.splats.get() && !s.keys_a.get() && !s.keys_b.get() && !s.vals_a.get() && !s.vals_b.get() && !s.fpw_a.get() && !s.fpw_b.get() &&
           !s.src_index.get() && !s.bin_offsets.get() && !s.k1_status.get() && !s.bin_status.get() && !s.ekeys_a.get() && !s.ekeys_b.get() &&
           !s.evals_a.get() && !s.evals_b.get() && !s.emit_start.get() && !s.blend_order.get() && !s.debug_consumed.get() &&
           !s.debug_walked.get() && !s.zero.get() && !s.depth_sums.get() && !s.tile_sums.get() && !s.tile_wide_hist.get() &&
           !s.fat_status.get() && !s.depths.get() && !s.debug_timing.get() && !s.removal_base.get() && !s.counters() && !s.tile_ranges() &&
           s.layout.points == 0 && s.zero.count() == 0;
}
// the arrays hold what the layout says, and every byte of them can be written
static void check_filled(FrameScratch& s, const ScratchLayout& l) {
    CHECK(s.splats.count() == l.splats && s.keys_a.count() == l.points && s.bin_offsets.count() == l.points);
    CHECK(s.k1_status.count() == l.k1_status && s.bin_status.count() == l.bin_status && s.evals_b.count() == l.entries);
    CHECK(s.emit_start.count() == l.emit_start && s.blend_order.count() == l.blend_order && s.debug_walked.count() == l.debug_walked);
    CHECK(s.zero.count() == l.zero && s.depth_sums.count() == l.sort_depth.sum_words && s.tile_sums.count() == l.sort_tiles.sum_words);
    CHECK((s.tile_wide_hist.get() != nullptr) == (l.sort_tiles.wide_bins != 0) && (s.fat_status.get() != nullptr) == (l.fat_status != 0));
    CHECK(!s.depths.get() && !s.debug_timing.get() && !s.removal_base.get());  // on first use, by the caller
    memset(s.splats.get(), 1, s.splats.bytes());
    memset(s.fpw_b.get(), 1, s.fpw_b.bytes());
    memset(s.zero.get(), 0, s.zero.bytes());
    memset(s.tile_sums.get(), 1, s.tile_sums.bytes());
    CHECK((void*)s.counters() == (void*)s.zero.get() && (char*)s.tile_ranges() + s.debug_consumed.count() * sizeof(uint2) == (char*)s.zero.get() + l.zero);
    const SortScratch d = s.sort_depth(), t = s.sort_tiles();
    CHECK(d.keys_alt == s.keys_b.get() && d.vals_alt == s.vals_b.get() && d.tile_sums == s.depth_sums.get() && d.hist_pitch == 512 && d.rows == 512);
    CHECK(t.keys_alt == s.ekeys_b.get() && t.tile_sums == s.tile_sums.get() && t.wide_hist == s.tile_wide_hist.get() && t.hist_pitch == 256);
    CHECK(d.hist == s.arena()->depth_hist && t.hist == s.arena()->tile_hist && t.cap == l.sort_tiles.cap && t.tiles_cap == l.sort_tiles.tiles_cap);
    const FatSortScratch f = s.fat_sort(3);
    CHECK(f.status == s.fat_status.get() && f.aux_alt == s.fpw_b.get() && f.tickets == s.counters()->sort_ticket && f.grid_request == 3);
}

int main() {
    {   // DeviceBuf
        DeviceBuf<uint32_t> a;
        CHECK(!a.get() && a.count() == 0 && g_live == 0);
        a.reset();                                 // of an empty buffer
        CHECK(a.alloc(0) == WS_OK && a.count() == 1 && a.bytes() == 4 && g_live == 1);  // a count of 0 is 1
        CHECK(a.alloc(100) == WS_OK && a.count() == 100 && g_live == 1);                // over a held block: freed first
        a.get()[99] = 7u;
        DeviceBuf<uint32_t> b(std::move(a));        // move construction
        CHECK(!a.get() && a.count() == 0 && b.count() == 100 && b.get()[99] == 7u && g_live == 1);
        DeviceBuf<uint32_t> c;
        CHECK(c.alloc(5) == WS_OK && g_live == 2);
        c = std::move(b);                          // move assignment onto a full buffer
        CHECK(!b.get() && c.count() == 100 && c.get()[99] == 7u && g_live == 1);
        DeviceBuf<uint32_t>& self = c;
        c = std::move(self);                       // onto itself
        CHECK(c.count() == 100 && c.get()[99] == 7u && g_live == 1);
        c.reset();
        c.reset();                                 // twice
        CHECK(!c.get() && c.count() == 0 && g_live == 0);
        g_fail_at = 1;
        CHECK(c.alloc(3) == WS_ERR_OOM && !c.get() && c.count() == 0 && g_live == 0);  // a failed alloc leaves it empty
        CHECK(c.alloc(3) == WS_OK && g_live == 1);
        g_fail_at = 1;
        CHECK(c.alloc(9) == WS_ERR_OOM && !c.get() && g_live == 0);                    // ... the held block is gone too (freed first)
    }
    CHECK(g_live == 0);

    const ScratchLayout small = layout_of(7, 33, 17, false, false), large = layout_of(300000, 1920, 1080, true, true);
    CHECK(large.sort_tiles.wide_bins != 0 && large.fat_status != 0 && small.sort_tiles.wide_bins == 0 && small.fat_status == 0);
    {   // FrameScratch: three layouts in a row, the lazily allocated arrays, letting go by assignment
        FrameScratch s;
        CHECK(empty(s));
        const ScratchLayout* order[3] = {&small, &large, &small};
        for (const ScratchLayout* l : order) {
            g_calls = 0;
            CHECK(s.alloc(*l) == WS_OK && g_live == g_calls);
            CHECK(g_calls == 22 + (l->sort_tiles.wide_bins ? 1 : 0) + (l->fat_status ? 1 : 0));
            check_filled(s, *l);
            CHECK(s.depths.alloc(s.layout.depths) == WS_OK && s.debug_timing.alloc(s.layout.debug_timing) == WS_OK &&
                  s.removal_base.alloc(s.layout.removal_base) == WS_OK && g_live == g_calls);
            memset(s.removal_base.get(), 0, s.removal_base.bytes());
        }
        s = FrameScratch();  // what renderer_free_scratch does
        CHECK(empty(s) && g_live == 0);
    }
    for (const ScratchLayout* l : {&small, &large}) {   // every allocation of a layout fails in turn
        FrameScratch s;
        g_calls = 0;
        CHECK(s.alloc(*l) == WS_OK);
        const long total = g_calls;
        for (long k = 1; k <= total; ++k) {
            g_fail_at = k;
            CHECK(s.alloc(*l) == WS_ERR_OOM);      // (over a full object for k = 1, over an empty one after)
            CHECK(g_fail_at == 0 && empty(s) && g_live == 0);
            g_calls = 0;
            CHECK(s.alloc(*l) == WS_OK && g_calls == total && g_live == total);
            check_filled(s, *l);
            if (k % 2) s = FrameScratch();         // the next failure meets an empty object, or a full one
        }
        g_fail_at = total + 1;                     // one past the last: nothing fails
        CHECK(s.alloc(*l) == WS_OK && g_fail_at == 1 && g_live == total);
        g_fail_at = 0;
    }
    CHECK(g_live == 0);
    printf("ok\n");
    return 0;
}
"""


def test_ownership_under_the_sanitizers(tmp_path):
    src, exe = tmp_path / "frame_scratch.cpp", tmp_path / "frame_scratch"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-self-move",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-isystem", os.path.join(ROCM, "include"), str(src), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout == "ok\n" and run.stderr == "", (run.returncode, run.stdout, run.stderr)
