"""The footprint patterns of tests/bin_patterns.py, checked on the CPU: what tests/test_gpu_binning.py asserts on the device means
something only if (1) reference_lists computes the lists it says it does, (2) every cloud the GPU file prepares is decided (no
rectangle within rounding of a tile boundary), drawn in the intended order and listed in the intended tiles -- on the oracle's K1
and sort, Cloud.oracle_frame's route with the uniforms built on the host -- and (3) every pattern reaches the edge of
k_bin_prefix / k_bin_emit / the tile-id sort it is named for, by the per-slice and per-workgroup numbers of the reference."""
import numpy as np
import pytest

import bin_patterns as bp
from bin_patterns import A_, B_, D_, E, N_, P


# ---- 1. reference_lists on a frame written by hand -------------------------------------------------------------------------
def _record(cx, cy, ax, ay, viewport):
    """A Splat record (10 halves) of an axis-aligned ellipse: half axes (ax, ay) px of the quad around the pixel (cx, cy)."""
    w, h = viewport
    rec = np.zeros(10, dtype=np.float16)
    rec[0], rec[1] = ax / w, 0.0                  # v1 / viewport
    rec[2], rec[3] = 0.0, -ay / h                 # v2 / viewport (y up in NDC)
    rec[4], rec[5] = 2.0 * cx / w - 1.0, 1.0 - 2.0 * cy / h
    rec[6:10] = 0.5
    return rec


def _hand_frame():
    """96 x 64 px = 3 x 2 tiles of 32 px, five splats by store slot; the kept extent is 2.1698 x the half axis:
         slot 0  a dot in tile (0, 0)                         (centre 16, 16; extent 2.2 px)
         slot 1  tiles (0, 0) .. (1, 0)                       (centre 32, 16; x extent 16 px: pixels 16 .. 47)
         slot 2  every tile                                    (centre 48, 32; extent 217 px)
         slot 3  no tile                                       (centre 105.6, 32: x_ndc = 1.2, off screen)
         slot 4  tiles (2, 0) .. (2, 1)                       (centre 80, 32; y extent 16 px)
    drawn far to near in the order 2, 0, 4, 1, 3."""
    vp = (96, 64)
    a16 = 16.0 / 2.1697873
    recs = np.stack([_record(16, 16, 1, 1, vp), _record(32, 16, a16, 1, vp), _record(48, 32, 100, 100, vp),
                     _record(105.6, 32, 1, 1, vp), _record(80, 32, 1, a16, vp)])
    return {"splats": recs.view(np.uint8).reshape(5, 20), "sorted": np.array([2, 0, 4, 1, 3], dtype=np.uint32)}, vp


def test_reference_lists_on_a_hand_written_frame():
    fr, vp = _hand_frame()
    L = bp.reference_lists(fr, vp, (5, 5), False)
    assert (L.tiles_x, L.tiles_y, L.ntiles) == (3, 2, 6)
    assert L.rects.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 2, 1], [-1, -1, -1, -1], [2, 0, 2, 1]]   # by store slot
    assert not L.undecided.any()
    assert L.counts.tolist() == [6, 1, 2, 2, 0] and L.offsets.tolist() == [0, 6, 7, 9, 11] and L.d == 11      # by draw position
    assert L.keys.tolist() == [0, 1, 2, 3, 4, 5, 0, 2, 5, 0, 1]
    assert L.vals.tolist() == [2, 2, 2, 2, 2, 2, 0, 4, 4, 1, 1]
    lists = [[2, 0, 1], [2, 1], [2, 4], [2], [2], [2, 4]]
    assert L.list_len.tolist() == [3, 2, 2, 1, 1, 2]
    assert L.begin.tolist() == [0, 3, 5, 7, 8, 9] and L.end.tolist() == [3, 5, 7, 8, 9, 11]
    assert [L.entries[b:e].tolist() for b, e in zip(L.begin, L.end)] == lists
    assert L.slices.tolist() == [[0, 4, 5]] and L.wg_totals.tolist() == [11]
    assert L.slice_starts.tolist() == [1, 0, 0, 0, 0]

    # lists per 2 x 2 tiles: 2 x 1 of them
    C = bp.reference_lists(fr, vp, (5, 5), True)
    assert (C.tiles_x, C.tiles_y, C.ntiles) == (2, 1, 2)
    assert C.counts.tolist() == [2, 1, 1, 1, 0] and C.d == 5
    assert C.keys.tolist() == [0, 1, 0, 1, 0] and C.vals.tolist() == [2, 2, 0, 4, 1]
    assert C.begin.tolist() == [0, 3] and C.end.tolist() == [3, 5] and C.entries.tolist() == [2, 0, 1, 2, 4]
    assert np.array_equal(C.rects, L.rects)                                                               # in tiles, not coarse

    # an overflowed frame keeps the first entries in draw order
    T = bp.reference_lists(fr, vp, (5, 5), False, count_cap=8)
    assert T.d == 11 and T.d_kept == 8
    assert [T.entries[b:e].tolist() for b, e in zip(T.begin, T.end)] == [[2, 0], [2], [2, 4], [2], [2], [2]]
    T = bp.reference_lists(fr, vp, (5, 5), False, count_cap=3)
    assert T.list_len.tolist() == [1, 1, 1, 0, 0, 0]
    assert T.begin.tolist() == [0, 1, 2, 0, 0, 0] and T.end.tolist() == [1, 2, 3, 0, 0, 0]             # empty: (0, 0)
    assert bp.reference_lists(fr, vp, (5, 5), False, count_cap=11).entries.tolist() == L.entries.tolist()
    assert bp.reference_lists(fr, vp, (5, 5), False, count_cap=0).d_kept == 0

    # 16-px tiles in y: 3 x 4 tiles, the column of slot 4 spans rows 1 .. 2 (pixels 16 .. 47)
    H = bp.reference_lists(fr, vp, (5, 4), False)
    assert (H.tiles_x, H.tiles_y) == (3, 4) and H.rects[4].tolist() == [2, 1, 2, 2] and H.rects[0].tolist() == [0, 0, 0, 1]


def test_reference_lists_reports_an_undecided_splat():
    """Slot 1 sits on the boundary between tile 0 and tile 1 (centre x = 32): it reaches the pixels 31 and 32 -- one tile each --
    as soon as its x extent, 2.1698 x the half axis a, is 0.5 px.  a = 0.23: the extent is 0.5 to within the 0.01 px band."""
    fr, vp = _hand_frame()
    recs = fr["splats"].view(np.float16).reshape(5, 10).copy()
    for a, undecided in ((0.23, True), (0.1, False), (0.5, False)):
        recs[1] = _record(32, 16, a, 1, vp)
        f = {"splats": recs.view(np.uint8).reshape(5, 20), "sorted": fr["sorted"]}
        L = bp.reference_lists(f, vp, (5, 5), False)
        assert bool(L.undecided[1]) == undecided, a
        assert L.undecided.sum() == int(undecided)


def test_slices_and_workgroup_totals():
    """Per-slice (s_lo, s_hi, ns) and the slice starts per position, on counts chosen by hand (E = 2048 entries per slice)."""
    vp = (96, 64)
    v = 3 * E
    recs = np.tile(_record(16, 16, 1, 1, vp), (v, 1))                    # one tile each ...
    recs[5] = _record(48, 32, 2000, 2000, vp)                            # ... but position 5: six tiles
    recs[10:E + 500] = _record(105.6, 32, 1, 1, vp)                      # and a run of none
    fr = {"splats": recs.view(np.uint8).reshape(v, 20), "sorted": np.arange(v, dtype=np.uint32)}
    L = bp.reference_lists(fr, vp, (5, 5), False)
    zeros = E + 490
    assert L.d == v - zeros + 5 == 2 * E + 5 - 490
    # entry E is owned by the position with offset E: 15 entries come before position 10, the run owns none
    own = E + 500 + (E - 15)
    assert L.offsets[own] == E
    assert L.slices.tolist() == [[0, own, own + 1], [own, v - 1, v - own]]
    assert L.wg_totals.tolist() == [15 + (P - E - 500), v - P]
    assert L.slice_starts[0] == 1 and L.slice_starts[own] == 1 and L.slice_starts.sum() == 2


# ---- 2. the recipes at 1024 x 512 ------------------------------------------------------------------------------------------
def _frame(ws, oracle, p):
    cl = bp.cloud(ws, p)
    fr = cl.oracle_frame(oracle)
    tl = (p.tile[0].bit_length() - 1, p.tile[1].bit_length() - 1)
    return fr, tl


def _margins(fr, viewport, tile):
    """px from each kept pixel bound (before the clamp to the viewport) to the nearest tile boundary, per store slot: how far
    the extents may move before a tile bound changes.  [V, 4]; bounds outside the viewport count as far."""
    vw, vh = viewport
    h = np.ascontiguousarray(fr["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    cx, cy = (h[:, 4] * 0.5 + 0.5) * vw, (0.5 - h[:, 5] * 0.5) * vh
    exx = bp.RAD * np.hypot(h[:, 0] * vw, h[:, 2] * vw) + 1e-3
    eyy = bp.RAD * np.hypot(h[:, 1] * vh, h[:, 3] * vh) + 1e-3
    out = []
    for edge, size, t in ((cx - exx - 0.5, vw, tile[0]), (cx + exx - 0.5, vw, tile[0]), (cy - eyy - 0.5, vh, tile[1]),
                          (cy + eyy - 0.5, vh, tile[1])):
        # the bound is ceil / floor of `edge`: a tile bound changes when `edge` crosses a multiple of the tile (minus one pixel
        # for the upper bound: pixel 31 -> 32)
        m = np.minimum(edge % t, t - edge % t)
        m2 = np.minimum((edge + 1.0) % t, t - (edge + 1.0) % t)
        inside = (edge > -1.0) & (edge < size)
        out.append(np.where(inside, np.minimum(m, m2), np.inf))
    return np.stack(out, axis=1)


def test_recipes_at_1024x512(ws, oracle):
    """Twenty Gaussians of all four classes: all visible (the N ones included), sorted as laid out, every rectangle the intended
    one, and no kept bound closer than 6 px to a tile boundary (dots 12 px, blocks of two or more tiles 15 px)."""
    vp, tile = (1024, 512), (32, 32)
    b = bp._Builder("recipes", vp, tile)
    b.none(2)
    b.dots([0, 31, 511, 300])
    b.block(3, 2, 3, 9)          # one column, tall
    b.block(0, 0, 1, 15)         # the left edge, full height
    b.block(10, 4, 12, 8)
    b.all()
    b.none()
    b.block(30, 0, 31, 15)       # the right edge
    b.block(5, 5, 5, 6)
    b.block(16, 1, 20, 14)
    b.dots([45, 200])
    b.all()
    b.block(7, 7, 7, 7)          # one tile: reads back as a dot
    b.block(0, 14, 0, 15)
    b.none()
    p = b.done()
    assert p.v == 20
    fr, tl = _frame(ws, oracle, p)
    assert fr["num_visible"] == 20 and np.array_equal(fr["src_index"], np.arange(20))
    assert np.array_equal(fr["sorted"], np.arange(20))
    L = bp.reference_lists(fr, vp, tl, False)
    assert not L.undecided.any()
    kind, rect = bp.classes(L, p, tl)
    wk, wr = bp.wanted_classes(p)
    assert np.array_equal(kind, wk) and np.array_equal(rect, wr)
    m = _margins(fr, vp, tile).min(axis=1)
    m[p.kind == N_] = np.inf                   # (no tile whatever its y bounds do: 52 px off screen in x)
    print("nearest bound to a tile boundary, px:", {"all": float(m[np.isfinite(m)].min()), "dots": float(m[p.kind == D_].min()),
                                                    "blocks": float(m[p.kind == B_].min())})
    # a dot: half a tile, less half a pixel, less the extent 3.0686 * sqrt(1 + 0.3) = 3.5 px (0.3: the low-pass of K1): 12 px, but
    # for the centre's f16 rounding (up to 0.25 px at 1024 px) and what the third scale adds through the Jacobian
    assert m.min() >= 6.0
    assert m[p.kind == D_].min() >= 11.5
    wide = (p.kind == B_) & ((p.rect[:, 2] > p.rect[:, 0]) & (p.rect[:, 3] > p.rect[:, 1]))
    assert m[wide].min() >= 15.0


# ---- 3. every pattern: decided, ordered, intended, and at its edge -----------------------------------------------------------
def _checked(ws, oracle, p):
    fr, tl = _frame(ws, oracle, p)
    assert fr["num_visible"] == p.v, p.name
    assert np.array_equal(fr["src_index"], np.arange(p.v)), p.name
    assert np.array_equal(fr["sorted"], np.arange(p.v, dtype=fr["sorted"].dtype)), p.name
    L = bp.reference_lists(fr, p.viewport, tl, False)
    assert not L.undecided.any(), (p.name, np.nonzero(L.undecided)[0][:5])
    kind, rect = bp.classes(L, p, tl)
    wk, wr = bp.wanted_classes(p)
    bad = np.nonzero((kind != wk) | (rect != wr).any(axis=1))[0]
    assert len(bad) == 0, (p.name, [(int(i), wr[i].tolist(), rect[i].tolist()) for i in bad[:5]])
    assert L.d == int(L.counts.sum()) == int(L.list_len.sum()) and len(L.entries) == L.d
    return L


@pytest.mark.parametrize("v", bp.DOT_SIZES)
def test_dots(ws, oracle, v):
    L = _checked(ws, oracle, bp.dots(v))
    assert L.d == v and np.all(L.counts == 1)
    assert len(L.slices) == -(-v // E) and len(L.wg_totals) == -(-v // P)
    assert L.wg_totals.sum() == v and (v <= P or L.wg_totals[0] == P)
    assert L.slices[-1, 1] == v - 1                                     # s_hi = V - 1 on the last slice
    if v > 1:
        assert len(np.unique(L.keys[:300])) == min(v, 300)              # the dots go round the tiles (300 of them at 640 x 480)


@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_one_tile(ws, oracle, which):
    p = bp.one_tile(which)
    L = _checked(ws, oracle, p)
    t = {"first": 0, "middle": 7 * 20 + 10, "last": 299}[which]
    assert L.ntiles == 300 and L.list_len[t] == 5000 and (L.list_len == 0).sum() == L.ntiles - 1
    assert L.begin[t] == 0 and L.end[t] == 5000 and not L.begin[np.arange(300) != t].any() and not L.end[np.arange(300) != t].any()
    assert np.array_equal(L.entries, np.arange(5000))
    assert -(-5000 // 2048) == 3 and -(-5000 // 1024) == 5              # the one list spans 3 (5) sort tiles


@pytest.mark.parametrize("where", bp.ZERO_WHERE)
@pytest.mark.parametrize("r", bp.ZERO_RUNS)
def test_zero_run(ws, oracle, r, where):
    p = bp.zero_run(r, where)
    L = _checked(ws, oracle, p)
    assert (p.kind == N_).sum() == r
    ns = L.slices[:, 2]
    if where == "lead":          # the run owns no entry and precedes the first owner: no slice holds it
        assert L.d == 2 and L.slices.tolist() == [[r, r + 1, 2]]
    elif where == "inner":
        assert L.d == 2 and L.slices.tolist() == [[0, r + 1, r + 2]]
    elif where == "trail":       # s_hi = V - 1 takes the whole run into the last slice
        assert L.d == 2 and L.slices.tolist() == [[0, r + 1, r + 2]]
    else:
        assert L.d == E + 2 and L.slices.tolist() == [[0, E, E + 1], [E, E + r + 1, r + 2]]
    if where != "lead":
        assert ns.max() == r + 2
        assert (ns.max() > E + 2) == (r > E)                            # E - 1, E: the LDS window; E + 1, 3 E + 5: global memory


def test_zero_run_edges_named_in_the_table(ws, oracle):
    assert bp.reference_lists(*_frame_args(ws, oracle, bp.zero_run(E + 1, "inner"))).slices[:, 2].tolist() == [E + 3]
    assert bp.reference_lists(*_frame_args(ws, oracle, bp.zero_run(E, "inner"))).slices[:, 2].tolist() == [E + 2]


def _frame_args(ws, oracle, p):
    fr, tl = _frame(ws, oracle, p)
    return fr, p.viewport, tl, False


def test_empty_blocks(ws, oracle):
    p = bp.empty_blocks()
    L = _checked(ws, oracle, p)
    assert p.v == bp.V_BLOCKS == 274449 and len(L.wg_totals) == 68 > bp.LOOKBACK
    assert L.wg_totals.tolist() == [2] + [0] * 65 + [1, 17]            # 65 consecutive workgroups of total 0
    assert p.kind[0] == D_ and p.kind[P - 1] == D_ and p.kind[66 * P] == D_ and np.all(p.kind[-17:] == D_)
    assert (p.kind == D_).sum() == 20
    # workgroup 66 polls 64 predecessors (2 .. 65: all zero, none inclusive) and then a second time; so does workgroup 67
    assert 66 - bp.LOOKBACK >= 1 and not L.wg_totals[66 - bp.LOOKBACK:66].any()
    assert L.slices.tolist() == [[0, p.v - 1, p.v]]                     # one slice, the offsets of 274 449 positions: global memory


def test_one_per_block(ws, oracle):
    p = bp.one_per_block()
    L = _checked(ws, oracle, p)
    assert p.v == bp.V_BLOCKS and L.wg_totals.tolist() == [1] * 68
    own = np.nonzero(p.kind == D_)[0]
    assert len(own) == 68 and np.array_equal(own[:67] % P, (61 * np.arange(67)) % P) and len(set((own[:67] % P).tolist())) == 67
    assert np.diff(own[:67]).min() > E + 2                              # owners further apart than the LDS window
    assert L.slices.tolist() == [[int(own[0]), p.v - 1, p.v - int(own[0])]]


@pytest.mark.parametrize("viewport", bp.BIG_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_big(ws, oracle, viewport):
    p = bp.big(viewport)
    L = _checked(ws, oracle, p)
    per_a = (viewport[0] // 32) * (viewport[1] // 32)
    assert "".join(bp.CLASS_NAMES[k] for k in p.kind) == "DDDDDADDDAAD"
    assert per_a == {(2048, 1152): 2304, (4096, 1056): 4224}[viewport] and L.d == 3 * per_a + 9
    assert L.counts.tolist() == [1] * 5 + [per_a] + [1] * 3 + [per_a] * 2 + [1]
    assert np.all(L.offsets[p.kind == A_] % E != 0)                      # unaligned
    starts = L.slice_starts[p.kind == A_]
    if viewport == (2048, 1152):
        assert per_a > E and starts.tolist() == [1, 1, 1]                 # each A across one slice start
    else:
        assert per_a > 2 * E and starts.tolist() == [2, 2, 2]             # a splat whose entry range holds two of them
        assert (L.slices[:, 2] == 1).sum() >= 3                           # slices that begin and end inside one A


@pytest.mark.parametrize("viewport", bp.WIDTH_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_widths(ws, oracle, viewport):
    p = bp.widths(viewport)
    L = _checked(ws, oracle, p)
    tx, ty = p.grid
    assert (tx, ty) == (256, viewport[1] // 16) and L.ntiles == {4080: 65280, 4096: 65536}[viewport[1]]
    assert (L.ntiles < 65535) == (viewport[1] == 4080)                    # 16-bit tile ids | 32-bit ones (frame_plan.h key16)
    blocks = p.rect[p.kind != D_]
    w = blocks[:, 2] - blocks[:, 0] + 1
    assert tuple(w.tolist()) == bp.WIDTHS and len(w) == 28
    assert np.all(blocks[:, 1] == 0) and np.all(blocks[:, 3] == ty - 1)  # full height: k runs up to w * rows - 1
    assert L.counts[p.kind != D_].tolist() == (w * ty).tolist() and L.counts.max() == 256 * ty <= 65536
    assert np.all(blocks[1::2, 2] == 255)                                 # every second block: x0 + w = 256
    assert len(set(blocks[0::2, 0].tolist())) > 8
    assert L.d == int((w * ty).sum()) + 29 < 700_000
    assert p.kind[-1] == D_ and p.kind[0] == D_ and np.all(p.kind[0::2] == D_)


@pytest.mark.parametrize("seed", [0, 1])
def test_mixed(ws, oracle, seed):
    p = bp.mixed(seed)
    L = _checked(ws, oracle, p)
    assert p.v == 20000
    share = np.bincount(p.kind, minlength=4) / p.v
    assert abs(share[N_] - 0.40) < 0.02 and abs(share[D_] - 0.40) < 0.02 and abs(share[B_] - 0.19) < 0.02 and 0.005 < share[A_] < 0.02
    b = p.rect[p.kind == B_]
    bw, bh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    assert np.all(bh * p.tile[1] >= bw * p.tile[0]) and bw.max() >= 8 and bh.max() >= 12 and (bw > 1).mean() > 0.5
    assert len(L.wg_totals) == 5 and L.d > 100_000 and (L.list_len > 0).all()
    assert L.slice_starts.max() == 1 and (L.slice_starts[p.kind == A_] == 1).any()   # 300-tile A's across slice starts


def test_look_away_sees_nothing(ws, oracle):
    """The V = 0 frame of the many-frames test: the camera turned round; its reference is empty lists."""
    for p in (bp.dots(1), bp.empty_blocks()):
        cl = bp.cloud(ws, p)
        fr = cl.oracle_frame(oracle, bp.look_away(ws, cl))
        assert fr["num_visible"] == 0 and len(fr["sorted"]) == 0
        L = bp.reference_lists(fr, p.viewport, (5, 5), False)
        assert L.d == 0 and L.ntiles == 300 and not L.list_len.any() and not L.begin.any() and not L.end.any()
        assert len(L.entries) == 0 and len(L.slices) == 0 and len(L.wg_totals) == 0


# ---- 4. the forms of tests/test_gpu_binning.py -------------------------------------------------------------------------------
FORM_GRIDS = [((640, 480), (32, 16)), ((640, 480), (16, 16)), ((8256, 96), (32, 32)), ((8192, 64), (32, 32)),
              ((256, 256), (32, 32)), ((288, 256), (32, 32)), ((2048, 1152), (32, 16)), ((2048, 1152), (16, 16))]


@pytest.mark.parametrize("viewport,tile", FORM_GRIDS, ids=[f"{v[0]}x{v[1]}-{t[0]}x{t[1]}" for v, t in FORM_GRIDS])
def test_form_patterns(ws, oracle, viewport, tile):
    """The five patterns of the forms, at every viewport and tile the GPU file builds them for."""
    for p in bp.form_patterns(viewport, tile, big_viewport=viewport):
        if viewport == (2048, 1152) and not p.name.startswith("big"):
            continue                                                      # (that viewport is big()'s alone)
        L = _checked(ws, oracle, p)
        if p.name.startswith("zero_run(2049"):
            assert L.slices[:, 2].tolist() == [E + 3]
        if p.name.startswith("zero_run(6149"):
            assert L.slices[:, 2].tolist() == [E + 1, 3 * E + 7]
        if p.name.startswith("big"):
            assert L.d == 3 * L.ntiles + 9
        if p.name.startswith("one_tile"):
            assert L.list_len[-1] == 5000 == L.d
    tx, ty = bp.grid(viewport, tile)
    if viewport == (8192, 64):
        assert tx == 256                                                  # still packed; an A of w = 256
    if viewport == (8256, 96):
        assert tx == 258 > 256                                            # FP_RECT_COUNT
    if viewport == (256, 256):
        assert tx * ty == 64
    if viewport == (288, 256):
        assert tx * ty == 72
