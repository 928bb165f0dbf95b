"""CPU test of the scene drivers' rule sheet (web-splat_amd/csrc/scene_frames.h, and grown_entry_capacity of frame_plan.h): the
size of a camera's frame, the name and the aspect of its ground-truth PNG, the verdict on a frame's error bits and the entry
capacity an overflowed frame asks for.  Built like tests/test_frame_plan.py: a few lines of C++ against the two headers (plain
C++, no HIP) answer an enumerated input space; the expected answers are transcriptions of the rules as they stood in
drivers.cpp at 8b93808, before the header merged their copies, each cited where it is transcribed.  One constant of a transcription
changed at a time must make the comparison fail."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")

IMG_NAME_FIELD = 128  # websplat.h ws_scene_camera::img_name
DONE, GROW_AND_DRAW_AGAIN, FAILED = 0, 1, 2

WIDTHS = (0, 1, 1599, 1600, 1601, 1920, 2000, 3200, 4096, 65535)
HEIGHTS = (0, 1, 2, 799, 1000, 1080, 1201, 65535)
NAMES = [b"a", b"a.png", b"a.PNG", b"a.PnG", b".png", b"png", b"a.pngx", b"a.jpg",
         b"n" * IMG_NAME_FIELD, b"n" * (IMG_NAME_FIELD - 4) + b".pNg", b"n" * (IMG_NAME_FIELD - 1)]   # (a full field has no terminator)
# (png w, png h, camera w, camera h): the exact aspect, skew == max(w, h) and one above it (5 w - 7 h = 7 and 8), a camera without
# width or height, and products beyond 32 bits on both sides of the rule
ASPECTS = [(96, 72, 160, 120), (4, 2, 160, 120), (7, 4, 7, 5), (3, 1, 7, 5), (4, 7, 5, 7), (1, 3, 5, 7), (7, 5, 7, 5), (7, 5, 0, 5), (7, 5, 7, 0),
           (0, 0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 1, 65535, 65535), (2 ** 32 - 1, 2 ** 32 - 2, 65535, 65535), (2 ** 32 - 1, 2 ** 32 - 3, 65535, 65535),
           (2 ** 32 - 3, 2 ** 32 - 1, 65535, 65535), (65536, 65536, 65536, 65537), (65536, 65537, 65536, 65536)]
DEMANDS = (0, 1, 4095, 8 << 20, 2 ** 32 - 1)


def parent_size(cam_w, cam_h, cap=1600):
    """capped_size, drivers.cpp:263-272 (the same lines inline at :127-136 and :191-200; bin/render.rs:58-62)."""
    w, h = cam_w, cam_h
    if w > cap:
        s = np.float32(w) / np.float32(cap)      # const float s = (float)*w / 1600.0f;
        w = cap
        h = int(np.float32(h) / s)               # *h = (uint32_t)((float)*h / s);
    return int(w != 0 and h != 0), w, h


def parent_path(gt_dir, field):
    """truth_read, drivers.cpp:325-328: strnlen over the field, the extension compared with | 0x20."""
    name = field[:IMG_NAME_FIELD].split(b"\0")[0]
    n = len(name)
    has_ext = n >= 4 and name[n - 4] == ord(".") and (name[n - 3] | 0x20) == ord("p") and (name[n - 2] | 0x20) == ord("n") and (name[n - 1] | 0x20) == ord("g")
    return gt_dir + b"/" + name + (b"" if has_ext else b".png")


def parent_aspect_ok(w, h, cam_w, cam_h):
    """truth_read, drivers.cpp:332-334: the skew of the cross products in 64 bits against the camera's longer side."""
    skew = abs(w * cam_h - h * cam_w)
    assert w * cam_h < 2 ** 64 and h * cam_w < 2 ** 64
    return int(not (cam_w == 0 or cam_h == 0 or skew > max(cam_w, cam_h)))


def parent_verdict(bits, attempt, last=2):
    """ws_render_views, drivers.cpp:151-159 (and eval_render_checked :292-297, evaluate_against_cloud :416-420): no bits, done; any
    bit but 0, or the last attempt, failed; else grow and draw again."""
    if bits == 0:
        return DONE
    if (bits & ~1) != 0 or attempt == last:
        return FAILED
    return GROW_AND_DRAW_AGAIN


def parent_capacity(needed, quarter=4):
    """drivers.cpp:159, :297, :414, :784 and frame_plan.h:179: (uint64_t)needed + needed / 4 + 4096."""
    return needed + needed // quarter + 4096


PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "frame_plan.h"
#include "scene_frames.h"
using namespace ws;
int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 's') {  // scene_frame_size
            unsigned cw, ch;
            uint32_t w = 7, h = 7;
            if (scanf("%u %u", &cw, &ch) != 2) return 1;
            const bool ok = scene_frame_size(cw, ch, &w, &h);
            printf("%d %u %u\n", ok ? 1 : 0, w, h);
        } else if (kind == 'n') {  // scene_truth_path: the name in hex, copied into a camera's field without a terminator of its own
            char hex[2 * sizeof(ws_scene_camera().img_name) + 2];
            struct { ws_scene_camera c; char guard[4]; } s;
            memset(&s, 0, sizeof s);
            memcpy(s.guard, "XYZ", 4);
            if (scanf("%257s", hex) != 1) return 1;
            const size_t n = strlen(hex) / 2;
            if (n > sizeof s.c.img_name) return 1;
            for (size_t i = 0; i < n; ++i) {
                unsigned b;
                sscanf(hex + 2 * i, "%2x", &b);
                s.c.img_name[i] = (char)b;
            }
            s.c.width = 0x58585858u;  // (what follows the field in the struct is not part of the name either)
            printf("%s\n", scene_truth_path("gt/dir", s.c).c_str());
        } else if (kind == 'a') {  // scene_truth_aspect_ok
            unsigned w, h, cw, ch;
            if (scanf("%u %u %u %u", &w, &h, &cw, &ch) != 4) return 1;
            printf("%d\n", scene_truth_aspect_ok(w, h, cw, ch) ? 1 : 0);
        } else if (kind == 'v') {  // frame_verdict
            unsigned bits;
            int attempt;
            if (scanf("%u %d", &bits, &attempt) != 2) return 1;
            printf("%d\n", (int)frame_verdict(bits, attempt));
        } else if (kind == 'c') {  // grown_entry_capacity: 64-bit
            unsigned demand;
            if (scanf("%u", &demand) != 1) return 1;
            static_assert(sizeof(grown_entry_capacity(0u)) == 8, "the capacity is 64-bit");
            printf("%llu\n", (unsigned long long)grown_entry_capacity(demand));
        } else {
            return 1;
        }
    }
    static_assert(frame_verdict(1u, 1) == FRAME_GROW_AND_DRAW_AGAIN && frame_verdict(1u, 2) == FRAME_FAILED && frame_verdict(0u, 2) == FRAME_DONE, "verdict");
    static_assert(grown_entry_capacity(4294967295u) == 4294967295ull + 1073741823ull + 4096ull, "no 32-bit wrap");
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_frames")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return ask


@pytest.fixture(scope="module")
def answers(ask):
    """The header's answers over the whole enumerated space, asked once."""
    sizes = list(itertools.product(WIDTHS, HEIGHTS))
    verdicts = list(itertools.product((0, 1, 2, 3), (0, 1, 2)))
    return dict(
        sizes=(sizes, [tuple(int(x) for x in ln.split()) for ln in ask([f"s {w} {h}" for w, h in sizes])]),
        names=(NAMES, [ln.encode() for ln in ask(["n " + name.hex() for name in NAMES])]),
        aspects=(ASPECTS, [int(ln) for ln in ask(["a %d %d %d %d" % a for a in ASPECTS])]),
        verdicts=(verdicts, [int(ln) for ln in ask([f"v {b} {k}" for b, k in verdicts])]),
        capacities=(DEMANDS, [int(ln) for ln in ask([f"c {d}" for d in DEMANDS])]))


def _differences(answers, what, rule):
    inputs, got = answers[what]
    return [(i, g, rule(i)) for i, g in zip(inputs, got) if g != rule(i)]


def test_frame_sizes(answers):
    assert _differences(answers, "sizes", lambda s: parent_size(*s)) == []
    assert parent_size(2000, 1000) == (1, 1600, 800)   # (tests/test_gpu_drivers.py relies on this one)
    assert parent_size(1600, 0) == (0, 1600, 0) and parent_size(65535, 1) == (0, 1600, 0) and parent_size(1601, 1) == (0, 1600, 0)
    assert parent_size(1601, 1201) == (1, 1600, 1200)


def test_truth_names(answers):
    assert _differences(answers, "names", lambda n: parent_path(b"gt/dir", n)) == []
    got = dict(zip(*answers["names"]))
    assert got[b"a"] == b"gt/dir/a.png" and got[b"a.PnG"] == b"gt/dir/a.PnG" and got[b".png"] == b"gt/dir/.png" and got[b"png"] == b"gt/dir/png.png"
    assert got[b"a.pngx"] == b"gt/dir/a.pngx.png" and got[b"a.jpg"] == b"gt/dir/a.jpg.png"
    assert got[b"n" * IMG_NAME_FIELD] == b"gt/dir/" + b"n" * IMG_NAME_FIELD + b".png"          # (nothing read past the field)
    assert got[b"n" * (IMG_NAME_FIELD - 4) + b".pNg"] == b"gt/dir/" + b"n" * (IMG_NAME_FIELD - 4) + b".pNg"


def test_truth_aspect(answers):
    assert _differences(answers, "aspects", lambda a: parent_aspect_ok(*a)) == []
    got = dict(zip(*answers["aspects"]))
    assert got[(7, 4, 7, 5)] == 1 and got[(3, 1, 7, 5)] == 0            # skew 7 == max(7, 5), and 8
    assert got[(7, 5, 0, 5)] == 0 and got[(7, 5, 7, 0)] == 0 and got[(96, 72, 160, 120)] == 1
    assert got[(2 ** 32 - 1, 2 ** 32 - 2, 65535, 65535)] == 1 and got[(2 ** 32 - 1, 2 ** 32 - 3, 65535, 65535)] == 0


def test_verdicts(answers):
    assert _differences(answers, "verdicts", lambda v: parent_verdict(*v)) == []
    got = dict(zip(*answers["verdicts"]))
    assert [got[(1, k)] for k in (0, 1, 2)] == [GROW_AND_DRAW_AGAIN, GROW_AND_DRAW_AGAIN, FAILED]
    assert all(got[(0, k)] == DONE and got[(2, k)] == FAILED and got[(3, k)] == FAILED for k in (0, 1, 2))


def test_capacities(answers):
    assert _differences(answers, "capacities", parent_capacity) == []
    got = dict(zip(*answers["capacities"]))
    assert got[0] == 4096 and got[8 << 20] == (10 << 20) + 4096 and got[2 ** 32 - 1] == 2 ** 32 - 1 + (2 ** 30 - 1) + 4096 > 2 ** 32


def test_a_changed_constant_is_told_apart(answers):
    """One constant of a transcription per mutation: the comparison against the header has to fail."""
    assert _differences(answers, "sizes", lambda s: parent_size(*s, cap=1599)) != []
    assert _differences(answers, "capacities", lambda d: parent_capacity(d, quarter=3)) != []
    assert _differences(answers, "verdicts", lambda v: parent_verdict(*v, last=1)) != []
    assert _differences(answers, "verdicts", lambda v: parent_verdict(*v, last=3)) != []
