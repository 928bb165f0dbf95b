"""CPU test of the staged-batch layout of the compositing kernels (web-splat_amd/csrc/blend_tile.h, layout layer): where a slot's
quadrant mask is stored, how a wave's compaction reads the masks back into its near -> far list, how a tile's range is cut into
batches with clamped prefetch addresses, the range decode and the bin-shift list index.  A few lines of C++ against the header
(plain C++, no HIP), built with -Wall -Werror and a second time with the address and undefined-behaviour sanitizers, walk
(STAGE, LCAP) = (256, 256), (512, 512), (1024, 512).  The expressions the header replaced are written out in the probe as they
stood in k_blend / k_contrib before blend_tile.h, and compared value for value."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")

PROBE = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "blend_tile.h"
using namespace ws::tile;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (++fails >= 20) exit(1); } } while (0)

static uint32_t rng_state;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// One sub-round's compaction for the quadrant bit `qbit`, as the device reads: per lane LCAP / 64 adjacent masks in 64-bit pieces
// (two 32-bit words x, y), quarters in order, lanes in order within a quarter (ballot + mbcnt), the skip rule on or off.
template <int LCAP>
static void compact_ref(const uint16_t* s_m, uint32_t sub, uint32_t nb, uint32_t qbit, bool skip, std::vector<uint32_t>& list) {
    for (int h = 0; h < LCAP / 256; ++h) {
        if (skip && piece_empty(nb, sub, h)) break;
        for (int q = 0; q < 4; ++q)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                uint32_t w[2];
                memcpy(w, s_m + mask_read_base<LCAP>(sub, lane) + 4 * h, 8);
                const uint32_t word = (q & 2) ? w[1] : w[0];
                if (word & (qbit << ((q & 1) * 16))) list.push_back(list_value(compact_slot(sub, lane, h, q)));
            }
    }
}

template <int QW, int QH, int STAGE_MAX, int STAGE_WANT, int LCAP_WANT>
static void geometry_case() {
    using G = Geometry<QW, QH, STAGE_MAX>;
    constexpr int STAGE = G::STAGE, LCAP = G::LCAP;
    static_assert(STAGE == STAGE_WANT && LCAP == LCAP_WANT, "the case this instantiation is meant to be");
    static_assert(G::NW == QW * QH && G::NT == 64 * QW * QH && G::SLOTS == STAGE + 1 && G::TW == 8 * QW && G::TH == 8 * QH, "geometry");
    unsigned long slots = 0, lists = 0, entries = 0, batches = 0;

    // 1. mask_slot: the parent's literal expression, and a bijection on [0, STAGE)
    std::vector<int> hit(STAGE, 0);
    for (uint32_t tid = 0; tid < (uint32_t)STAGE; ++tid) {
        const uint32_t parent = ((uint32_t)tid / LCAP) * LCAP + ((uint32_t)tid & 63u) * (LCAP / 64) + (((uint32_t)tid % LCAP) >> 6);
        const uint32_t got = mask_slot<LCAP>(tid);
        CHECK(got == parent, "mask_slot<%d>(%u) = %u, parent %u", LCAP, tid, got, parent);
        CHECK(got < (uint32_t)STAGE, "mask_slot<%d>(%u) = %u out of the plane", LCAP, tid, got);
        if (got < (uint32_t)STAGE) ++hit[got];
        ++slots;
    }
    for (int i = 0; i < STAGE; ++i) CHECK(hit[i] == 1, "mask index %d written %d times", i, hit[i]);

    // 2. round trip: store through mask_slot, read back as compact reads
    const int nbs[] = {1, 63, 64, 65, 255, 256, 257, LCAP - 1, LCAP, LCAP + 1, STAGE - 1, STAGE};
    for (int nbi : nbs) {
        if (nbi < 1 || nbi > STAGE) continue;
        const uint32_t nb = (uint32_t)nbi;
        for (int kind = 0; kind < 4; ++kind) {  // dense random, sparse random (x2 seeds), every bit set
            rng_state = 0x9E3779B9u * (uint32_t)(kind + 1) + nb;
            std::vector<uint16_t> masks(STAGE, 0);
            for (uint32_t s = 0; s < nb; ++s) masks[s] = kind == 3 ? 0xFFFFu : (uint16_t)(kind == 0 ? rng() : (rng() & rng() & rng()));
            std::vector<uint16_t> s_m(STAGE, 0xDEADu);  // (every index is written: the bijection above)
            for (uint32_t s = 0; s < (uint32_t)STAGE; ++s) s_m[mask_slot<LCAP>(s)] = masks[s];
            for (int skip = 0; skip < 2; ++skip)
                for (int bit = 0; bit < 16; ++bit) {
                    std::vector<uint32_t> list, want;
                    for (uint32_t sub = 0; sub < nb; sub += (uint32_t)LCAP) compact_ref<LCAP>(s_m.data(), sub, nb, 1u << bit, skip != 0, list);
                    for (uint32_t s = 0; s < (uint32_t)STAGE; ++s)
                        if (masks[s] & (1u << bit)) want.push_back(s);
                    CHECK(list.size() == want.size(), "STAGE %d nb %u kind %d skip %d bit %d: %zu listed, %zu set", STAGE, nb, kind, skip, bit,
                          list.size(), want.size());
                    for (size_t i = 0; i < list.size() && i < want.size(); ++i) {
                        CHECK(list[i] == want[i] * 16u, "STAGE %d nb %u kind %d skip %d bit %d: list[%zu] = %u, slot %u expected", STAGE, nb,
                              kind, skip, bit, i, list[i], want[i]);
                        CHECK(list[i] / 16u < nb, "slot %u listed beyond nb %u", list[i] / 16u, nb);
                    }
                    ++lists;
                    entries += list.size();
                }
        }
    }

    // 3. batch arithmetic: walk hi down by nb as the kernels do, with their prefetch calls
    const uint32_t begin = 1000003u;
    const uint32_t lens[] = {1u, (uint32_t)STAGE - 1u, (uint32_t)STAGE, (uint32_t)STAGE + 1u, 2u * STAGE, 2u * STAGE + 1u};
    for (uint32_t len : lens) {
        const uint32_t end = begin + len;
        std::vector<int> covered(len, 0);
        auto inside = [&](uint32_t hi, const char* what) {
            for (uint32_t tid = 0; tid < (uint32_t)STAGE; ++tid) {
                const uint32_t pos = entry_pos<STAGE>(begin, hi, tid);
                CHECK(pos >= begin && pos < end, "len %u %s hi %u tid %u: position %u outside [%u, %u)", len, what, hi, tid, pos, begin, end);
            }
        };
        uint32_t hi = end;
        while (hi > begin) {
            const uint32_t nb = batch_len<STAGE>(begin, hi);
            const uint32_t parent_nb = (hi - begin) < (uint32_t)STAGE ? (hi - begin) : (uint32_t)STAGE;
            CHECK(nb == parent_nb && nb >= 1u, "batch_len<%d>(%u, %u) = %u, parent %u", STAGE, begin, hi, nb, parent_nb);
            inside(hi, "batch");
            for (uint32_t tid = 0; tid < nb; ++tid) {
                const uint32_t pos = entry_pos<STAGE>(begin, hi, tid);
                CHECK(pos == hi - 1u - tid, "len %u hi %u tid %u: position %u, expected %u", len, hi, tid, pos, hi - 1u - tid);
                if (pos >= begin && pos < end) ++covered[pos - begin];
            }
            const uint32_t hi_next = hi - nb;
            // the prefetches: the next batch (hi_next, == begin behind the last batch) and the entry indices of the one after it
            inside(hi_next, "next batch");
            inside(hi_next - begin > (uint32_t)STAGE ? hi_next - (uint32_t)STAGE : begin, "batch after next");
            hi = hi_next;
            ++batches;
        }
        inside(begin, "hi == begin");
        for (uint32_t i = 0; i < len; ++i) CHECK(covered[i] == 1, "len %u: entry %u staged %d times", len, i, covered[i]);
    }
    printf("case STAGE %d LCAP %d slots %lu lists %lu entries %lu batches %lu\n", STAGE, LCAP, slots, lists, entries, batches);
}

int main() {
    geometry_case<2, 2, 512, 256, 256>();
    geometry_case<4, 4, 512, 512, 512>();
    geometry_case<4, 4, 1024, 1024, 512>();
    static_assert(Geometry<4, 2, 512>::STAGE == 512 && Geometry<4, 4>::STAGE == (WS_BLEND_STAGE_MAX < 1024 ? WS_BLEND_STAGE_MAX : 1024), "default");

    // 4. range decode: (0, 0) stays empty; (0xFFFFFFFF - begin, end) -> begin
    unsigned long decoded = 0, indexed = 0;
    CHECK(range_begin(0u, 0u) == 0u, "(0, 0) must decode to the empty range [0, 0)");
    const uint32_t begins[] = {0u, 1u, 12345u, 0x7FFFFFFFu, 0xFFFFFFF0u};
    for (uint32_t b : begins) {
        const uint32_t x = 0xFFFFFFFFu - b, y = b + 5u;
        const uint32_t parent = y ? 0xFFFFFFFFu - x : 0u;
        CHECK(range_begin(x, y) == b && parent == b, "range_begin(%u, %u) = %u, expected %u", x, y, range_begin(x, y), b);
        ++decoded;
    }
    // list index on an odd bin_tiles_x, bin_shift 0 / 1 x range_row_shift 0 / 1, against the parent's expression
    const uint32_t bin_tiles_x = 7u, bin_tiles_y = 5u;
    for (uint32_t s = 0; s < 2; ++s)
        for (uint32_t rrs = 0; rrs < 2; ++rrs) {
            const uint32_t lists_x = s ? (bin_tiles_x + 1u) >> 1 : bin_tiles_x, lists_y = s ? (bin_tiles_y + 1u) >> 1 : bin_tiles_y;
            for (uint32_t ty = 0; ty < (bin_tiles_y << rrs); ++ty)
                for (uint32_t tx = 0; tx < bin_tiles_x; ++tx) {
                    const uint32_t btx = s ? (bin_tiles_x + 1u) >> 1 : bin_tiles_x;
                    const uint32_t parent = ((ty >> rrs) >> s) * btx + (tx >> s);
                    const uint32_t got = list_index(tx, ty, s, bin_tiles_x, rrs);
                    CHECK(got == parent, "list_index(%u, %u, %u, %u, %u) = %u, parent %u", tx, ty, s, bin_tiles_x, rrs, got, parent);
                    CHECK(got < lists_x * lists_y, "list %u of %u", got, lists_x * lists_y);
                    CHECK(got == ((ty >> rrs) >> s) * lists_x + (tx >> s), "list %u is not the one of binning tile (%u, %u)", got, tx >> s, (ty >> rrs) >> s);
                    ++indexed;
                }
        }
    printf("ranges %lu indices %lu\n", decoded, indexed);
    printf(fails ? "FAILED %d\n" : "ok %d\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_layout_probe(flags, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout[-4000:], res.stderr[-4000:])
    assert res.returncode == 0, "the layout probe failed (its output is above)"
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok 0"
    cases = [dict(zip(ln.split()[1::2], map(int, ln.split()[2::2]))) for ln in lines if ln.startswith("case ")]
    assert [(c["STAGE"], c["LCAP"]) for c in cases] == [(256, 256), (512, 512), (1024, 512)]
    for c in cases:  # nothing vacuous: every slot, lists with entries, more than one batch
        assert c["slots"] == c["STAGE"] and c["lists"] >= 10 * 4 * 2 * 16 and c["entries"] > 10 * c["STAGE"] and c["batches"] >= 10
    assert lines[-2] == "ranges 5 indices %d" % (2 * (7 * 5 + 7 * 10))
