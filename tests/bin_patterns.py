"""Footprint patterns for the binning stage (web-splat_amd/csrc/raster.hip k_bin_prefix / k_bin_emit, emit_gen.h, the tile-id
sort of sort.hip with its range recording), the clouds that realise them, and the exact lists a frame must end up with.  Pure
numpy plus websplat.synth and the Cloud of tests/k1_patterns.py; the library (`ws`) and the oracle are handed in by the caller,
nothing here needs a GPU.

Random clouds put the edges of this stage where chance puts them.  Here the CALLER decides which tiles every draw position is
listed in:

  classes         every Gaussian is axis-aligned (identity quaternion, third scale 1e-3) and of one of four classes:
                    N  none   sigma = 1 px, centre at x_ndc = 1.1: visible (inside the 1.2 w cull bound), zero tiles
                    D  dot    sigma = 1 px at the centre of a chosen tile: one tile
                    B  block  tiles a..b x c..d: the kept extent ends in the middle of the first and the last tile of an axis
                              (half extent = half a tile x (b - a), at least 6 px; sigma = half extent / 3.0686)
                    A  all    sigma = 20 x the viewport's width: every tile
  draw order      a pattern is a sequence of classes over draw positions, far to near: position i sits at view depth
                  3 + (V - i) * step, so the depth sort returns 0 .. V-1 and `store slot == draw position == Gaussian`
  reference_lists the tile lists of a frame, from the frame's OWN records (download_frame / the oracle's frame): the rectangle of
                  footprint.h restated in float64, entries in draw order, a stable sort by tile id.  Integer-exact: a splat whose
                  rectangle a relative 1e-4 and 0.01 px on the extents could change is reported as undecided, and the callers
                  assert that there is none.

tests/test_bin_patterns.py shows on the CPU that every pattern is decided, ordered as intended and reaches the edge it is
named for; tests/test_gpu_binning.py compares the device's lists with reference_lists of the device's own frame."""
import functools
from dataclasses import dataclass

import numpy as np

import k1_patterns as kp
from websplat import synth

E = 2048                 # entries per emit slice and per (large) sort tile: frame_plan.h EMIT_TILE (= SORT_TILE = 256 x 8)
P = 4096                 # draw positions per workgroup of the binning prefix: raster.hip BIN_THREADS * BIN_IPT (256 x 16)
LOOKBACK = 64            # predecessors per poll of the look-back (lookback.h: one wave)
V_BLOCKS = 67 * P + 17   # 68 prefix workgroups (a look-back of two polls), the last one with 17 positions
SH_DEG = 0               # 17 floats per row: the 274 k clouds stay small
CAM_Z = -3.0             # synth.camera_c1: at (0, 0, -3), looking along +z
D_FAR = 6.0              # no pattern reaches further than this view depth
SIGMA_PER_EXTENT = 3.0686    # half extent of the kept ellipse = 2.1698 * sqrt(2) * sigma (footprint.h: rad * |row of M|)
N_, D_, B_, A_ = 0, 1, 2, 3
CLASS_NAMES = "NDBA"

DOT_SIZES = (1, 2, 255, 256, 257, E - 1, E, E + 1, P - 1, P, P + 1, 2 * P, 2 * P + 1)
ZERO_RUNS = (E - 1, E, E + 1, 3 * E + 5)
ZERO_WHERE = ("lead", "inner", "trail", "second_slice")
WIDTHS = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 47, 63, 65, 95, 127, 129, 191, 253, 254, 255, 256)
BIG_VIEWPORTS = ((2048, 1152), (4096, 1056))      # 2304 tiles per A | 4224 tiles per A: more than 2 E
WIDTH_VIEWPORTS = ((4096, 4080), (4096, 4096))    # 16-px tiles: 65280 tiles, 16-bit ids | 65536 tiles, 32-bit ids
MIXED_V = 20000


# ---- patterns --------------------------------------------------------------------------------------------------------------
@dataclass
class Pattern:
    name: str
    viewport: tuple           # (w, h) in pixels
    tile: tuple               # (tw, th) in pixels: the tile the classes are laid out on
    kind: np.ndarray          # int8 [V]: N_ / D_ / B_ / A_ by draw position
    rect: np.ndarray          # int32 [V, 4]: (tx0, ty0, tx1, ty1) inclusive, in `tile` units; -1 for N

    @property
    def v(self):
        return len(self.kind)

    @property
    def grid(self):
        return grid(self.viewport, self.tile)


def grid(viewport, tile):
    return -(-viewport[0] // tile[0]), -(-viewport[1] // tile[1])


class _Builder:
    def __init__(self, name, viewport, tile):
        self.name, self.viewport, self.tile = name, tuple(viewport), tuple(tile)
        # a dot sits at the centre of a whole tile, a block ends in the middle of one: no partial tile at the viewport's edge
        assert viewport[0] % tile[0] == 0 and viewport[1] % tile[1] == 0, (viewport, tile)
        self.tx, self.ty = grid(viewport, tile)
        self.kinds, self.rects = [], []

    def _add(self, kind, rects):
        rects = np.asarray(rects, dtype=np.int32).reshape(-1, 4)
        self.kinds.append(np.full(len(rects), kind, dtype=np.int8))
        self.rects.append(rects)

    def none(self, count=1):
        self._add(N_, np.full((count, 4), -1))

    def dots(self, tiles):
        t = np.asarray(tiles, dtype=np.int64).reshape(-1)
        assert len(t) == 0 or (t.min() >= 0 and t.max() < self.tx * self.ty)
        x, y = t % self.tx, t // self.tx
        self._add(D_, np.stack([x, y, x, y], axis=1))

    def block(self, tx0, ty0, tx1, ty1):
        assert 0 <= tx0 <= tx1 < self.tx and 0 <= ty0 <= ty1 < self.ty
        self._add(B_, [[tx0, ty0, tx1, ty1]])

    def all(self, count=1):
        self._add(A_, np.tile([[0, 0, self.tx - 1, self.ty - 1]], (count, 1)))

    def done(self):
        return Pattern(self.name, self.viewport, self.tile, np.concatenate(self.kinds), np.concatenate(self.rects))


def _spread(i, ntiles):
    """The tile of dot i: 7919 is prime and shares no factor with any grid used here, so the dots visit every tile."""
    return (np.asarray(i, dtype=np.int64) * 7919) % ntiles


def dots(v, viewport=(640, 480), tile=(32, 32)):
    b = _Builder(f"dots({v})", viewport, tile)
    b.dots(_spread(np.arange(v), b.tx * b.ty))
    return b.done()


def one_tile(which, viewport=(640, 480), tile=(32, 32)):
    b = _Builder(f"one_tile({which})", viewport, tile)
    n = b.tx * b.ty
    t = {"first": 0, "middle": (b.ty // 2) * b.tx + b.tx // 2, "last": n - 1}[which]
    b.dots(np.full(5000, t))
    return b.done()


def zero_run(r, where, viewport=(640, 480), tile=(32, 32)):
    b = _Builder(f"zero_run({r},{where})", viewport, tile)
    n = b.tx * b.ty
    if where == "lead":
        b.none(r)
        b.dots(_spread([0, 1], n))
    elif where == "inner":
        b.dots(_spread([0], n))
        b.none(r)
        b.dots(_spread([1], n))
    elif where == "trail":
        b.dots(_spread([0, 1], n))
        b.none(r)
    elif where == "second_slice":
        b.dots(_spread(np.arange(E), n))
        b.dots(_spread([E], n))
        b.none(r)
        b.dots(_spread([E + 1], n))
    else:
        raise KeyError(where)
    return b.done()


def empty_blocks(viewport=(640, 480), tile=(32, 32)):
    """Workgroup 0: dots at its first and last position.  Workgroups 1 .. 65: nothing.  Workgroup 66: a dot at its position 0.
    Workgroup 67: its 17 positions, all dots."""
    b = _Builder("empty_blocks", viewport, tile)
    n = b.tx * b.ty
    b.dots(_spread([0], n))
    b.none(P - 2)
    b.dots(_spread([1], n))
    b.none(65 * P)
    b.dots(_spread([2], n))
    b.none(P - 1)
    b.dots(_spread(3 + np.arange(17), n))
    p = b.done()
    assert p.v == V_BLOCKS
    return p


def one_per_block(viewport=(640, 480), tile=(32, 32)):
    b = _Builder("one_per_block", viewport, tile)
    n = b.tx * b.ty
    for blk in range(68):
        size = P if blk < 67 else 17
        at = (61 * blk) % P
        if at >= size:
            at = at % size
        b.none(at)
        b.dots(_spread([blk], n))
        b.none(size - at - 1)
    p = b.done()
    assert p.v == V_BLOCKS
    return p


def big(viewport, tile=(32, 32)):
    """D x 5, A, D x 3, A, A, D."""
    b = _Builder(f"big({viewport[0]}x{viewport[1]})", viewport, tile)
    n = b.tx * b.ty
    b.dots(_spread(np.arange(5), n))
    b.all()
    b.dots(_spread(5 + np.arange(3), n))
    b.all(2)
    b.dots(_spread([8], n))
    return b.done()


def widths(viewport, tile=(16, 16)):
    """One full-height block per width of WIDTHS, dots between: every second block ends at the right edge of the grid (with 256
    columns: x0 + w = 256), the others start at a column that changes from block to block."""
    b = _Builder(f"widths({viewport[0]}x{viewport[1]})", viewport, tile)
    n = b.tx * b.ty
    for k, w in enumerate(WIDTHS):
        assert w <= b.tx
        x0 = b.tx - w if k & 1 else (37 * k) % (b.tx - w + 1)
        b.dots(_spread([k], n))
        b.block(x0, 0, x0 + w - 1, b.ty - 1)
    b.dots(_spread([len(WIDTHS)], n))
    return b.done()


def mixed(seed, viewport=(640, 480), tile=(32, 32)):
    """MIXED_V positions, the class drawn per position: 40 % N, 40 % D, 19 % blocks of random place and size, 1 % A.

    A block is never wider than tall in pixels.  K1 (preprocess.wgsl, and the oracle and the kernel with it) takes the first
    axis of the 2-D covariance as normalize((offDiagonal, lambda1 - diagonal1)).  For an axis-aligned Gaussian with the larger
    variance in x both components are next to nothing -- offDiagonal is the 1e-6 the third scale leaves, lambda1 - diagonal1
    is 0 or an ulp of rounding -- and their quotient turns the ellipse by whatever angle the noise gives (tried: 12 of 3800
    wider-than-tall blocks came back with another rectangle).  With the larger variance in y the second component is the
    difference of the variances and the axis is exact; the full-height blocks of widths() cover the wide rectangles."""
    b = _Builder(f"mixed({seed})", viewport, tile)
    rng = np.random.default_rng(4000 + seed)
    v = MIXED_V
    u = rng.random(v)
    kind = np.where(u < 0.40, N_, np.where(u < 0.80, D_, np.where(u < 0.99, B_, A_))).astype(np.int8)
    t = rng.integers(0, b.tx * b.ty, size=v)
    tw, th = b.tile
    bw = rng.integers(1, min(b.tx, 9, b.ty * th // tw) + 1, size=v)
    bh_min = -(-bw * tw // th)                         # at least as tall as wide
    bh = bh_min + (rng.random(v) * (np.minimum(b.ty, bh_min + 8) - bh_min + 1)).astype(np.int64)
    bh[(bw == 1) & (bh == 1)] = 2                      # a 1 x 1 block reads back as a dot
    x0 = (rng.random(v) * (b.tx - bw + 1)).astype(np.int64)
    y0 = (rng.random(v) * (b.ty - bh + 1)).astype(np.int64)
    rect = np.full((v, 4), -1, dtype=np.int32)
    d = kind == D_
    rect[d] = np.stack([t % b.tx, t // b.tx, t % b.tx, t // b.tx], axis=1)[d]
    k = kind == B_
    rect[k] = np.stack([x0, y0, x0 + bw - 1, y0 + bh - 1], axis=1)[k]
    rect[kind == A_] = [0, 0, b.tx - 1, b.ty - 1]
    return Pattern(b.name, b.viewport, b.tile, kind, rect)


def form_patterns(viewport=(640, 480), tile=(32, 32), big_viewport=BIG_VIEWPORTS[0]):
    """The five patterns every launch form is checked on."""
    return [zero_run(E + 1, "inner", viewport, tile), zero_run(3 * E + 5, "second_slice", viewport, tile), big(big_viewport, tile),
            one_tile("last", viewport, tile), mixed(0, viewport, tile)]


def table(tile=(32, 32), viewport=(640, 480)):
    """Every pattern of the table, as (id, builder): built when the test runs, not when it is collected."""
    out = [(f"dots-{v}", functools.partial(dots, v, viewport, tile)) for v in DOT_SIZES]
    out += [(f"one_tile-{t}", functools.partial(one_tile, t, viewport, tile)) for t in ("first", "middle", "last")]
    out += [(f"zero_run-{r}-{w}", functools.partial(zero_run, r, w, viewport, tile)) for r in ZERO_RUNS for w in ZERO_WHERE]
    out += [("empty_blocks", functools.partial(empty_blocks, viewport, tile)),
            ("one_per_block", functools.partial(one_per_block, viewport, tile))]
    out += [(f"big-{vp[0]}x{vp[1]}", functools.partial(big, vp, tile)) for vp in BIG_VIEWPORTS]
    out += [(f"widths-{vp[0]}x{vp[1]}", functools.partial(widths, vp, (16, 16))) for vp in WIDTH_VIEWPORTS]
    out += [(f"mixed-{s}", functools.partial(mixed, s, viewport, tile)) for s in (0, 1)]
    return out


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def depth_step(v):
    """1e-3 for small clouds, at least 1e-5 for the largest: consecutive depth keys (bits of zfar - z, z around 3 .. 6: an ulp
    of 5e-7) stay strictly decreasing in f32."""
    return max(1e-5, min(1e-3, 2.5 / max(v, 1)))


def bbox(ws, viewport):
    """One bounding box per viewport, holding every centre a pattern can produce (x_ndc = 1.1 at the far end): near / far, the
    scene extend and the default clip box do not depend on the pattern."""
    w, h = viewport
    bx = 0.55 * D_FAR + 0.2
    by = 0.55 * D_FAR * h / w + 0.2
    return ws.Aabb([-bx, -by, -0.25], [bx, by, D_FAR + CAM_Z + 0.25])


def geometry(p):
    """(px, py, sigma_x, sigma_y) in pixels per draw position."""
    w, h = p.viewport
    tw, th = p.tile
    v = p.v
    r = p.rect.astype(np.float64)
    px, py = np.full(v, w / 2.0), np.full(v, h / 2.0)
    sx, sy = np.ones(v), np.ones(v)
    n = p.kind == N_
    px[n] = w / 2.0 + 1.1 * w / 2.0
    d = p.kind == D_
    px[d], py[d] = (r[d, 0] + 0.5) * tw, (r[d, 1] + 0.5) * th
    b = p.kind == B_
    px[b], py[b] = (r[b, 0] + r[b, 2] + 1.0) / 2.0 * tw, (r[b, 1] + r[b, 3] + 1.0) / 2.0 * th
    sx[b] = np.maximum(6.0, (r[b, 2] - r[b, 0]) * tw / 2.0) / SIGMA_PER_EXTENT
    sy[b] = np.maximum(6.0, (r[b, 3] - r[b, 1]) * th / 2.0) / SIGMA_PER_EXTENT
    a = p.kind == A_
    sx[a] = sy[a] = 20.0 * w
    return px, py, sx, sy


def rows(p):
    """PLY rows (17 floats: sh_deg 0) of the pattern's cloud, Gaussian i = draw position i."""
    w, h = p.viewport
    fx = float(w)
    v = p.v
    px, py, sx, sy = geometry(p)
    d = 3.0 + (v - np.arange(v)) * depth_step(v)
    assert v == 0 or d.max() <= D_FAR
    rng = np.random.default_rng(v)
    out = np.zeros((v, synth.PLY_ROW_LEN[SH_DEG]), dtype=np.float32)
    out[:, 0] = (px - w / 2.0) * d / fx
    out[:, 1] = (py - h / 2.0) * d / fx
    out[:, 2] = d + CAM_Z
    out[:, 6:9] = rng.uniform(-1.5, 1.5, size=(v, 3))
    # opacities (logits) by class, so that a frame of thousands still shows through and every entry moves its pixels by more
    # than the blend's gate: an A 0.0025 .. 0.007, a block 0.007 .. 0.03, a dot 0.27 .. 0.73
    out[:, 9] = np.where(p.kind == A_, rng.uniform(-6.0, -5.0, size=v),
                         np.where(p.kind == B_, rng.uniform(-5.0, -3.5, size=v), rng.uniform(-1.0, 1.0, size=v)))
    out[:, 10] = np.log(sx * d / fx)
    out[:, 11] = np.log(sy * d / fx)
    out[:, 12] = np.log(1e-3)
    out[:, 13] = 1.0                                       # identity quaternion (w, x, y, z)
    return out


def cloud(ws, p):
    """The pattern's cloud as a k1_patterns.Cloud (uniforms() and oracle_frame() are its), under k1_patterns' camera:
    synth.camera_c1 with fx = fy = the viewport's width."""
    viewport = p.viewport
    rw = rows(p)
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rw, SH_DEG)
    box = bbox(ws, viewport)
    gpc.aabb, gpc.center = box, box.center()
    cj = synth.camera_c1(*viewport)
    cj.fx = cj.fy = float(viewport[0])
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, *viewport)
    cam.fit_near_far(box)
    args = ws.SplattingArgs(camera=cam, viewport=viewport, max_sh_deg=SH_DEG)
    return kp.Cloud(p.name, p.v, "uncompressed", "bin", viewport, np.ones(p.v, dtype=bool), rw[:, 0:3].copy(), gpc, None, cam,
                    args)


def look_away(ws, cl):
    """SplattingArgs that see nothing of cl: the same camera turned round (V = 0)."""
    w, h = cl.viewport
    cj = synth.camera_c1(w, h)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, [[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], float(w),
                                                 float(w), w, h)
    cam.fit_near_far(cl.gpc.aabb)
    return ws.SplattingArgs(camera=cam, viewport=cl.viewport, max_sh_deg=SH_DEG)


# ---- the reference ---------------------------------------------------------------------------------------------------------
RAD = 2.1697873 * 1.00001        # footprint.h:65 sqrt(2 * CUTOFF), padded


def _tile_rects(cx, cy, exx, eyy, ok, vw, vh, tw_log2, th_log2):
    """footprint.h:72-83 per splat: int64 [n, 4] (tx0, ty0, tx1, ty1), -1 where the rectangle is empty."""
    x_lo, x_hi = np.ceil(cx - exx - 0.5), np.floor(cx + exx - 0.5)
    y_lo, y_hi = np.ceil(cy - eyy - 0.5), np.floor(cy + eyy - 0.5)
    x_lo, y_lo = np.maximum(x_lo, 0.0), np.maximum(y_lo, 0.0)
    x_hi, y_hi = np.minimum(x_hi, vw - 1.0), np.minimum(y_hi, vh - 1.0)
    some = ok & (x_lo <= x_hi) & (y_lo <= y_hi)
    out = np.full((len(cx), 4), -1, dtype=np.int64)
    s = np.nonzero(some)[0]
    out[s, 0] = x_lo[s].astype(np.int64) >> tw_log2
    out[s, 1] = y_lo[s].astype(np.int64) >> th_log2
    out[s, 2] = x_hi[s].astype(np.int64) >> tw_log2
    out[s, 3] = y_hi[s].astype(np.int64) >> th_log2
    return out


def splat_rects(splats, viewport, tile_log2):
    """(rects int64 [n, 4] by store slot, undecided bool [n]): lines 57-83 of footprint.h in float64 on the f16 record, and
    whether a relative 1e-4 plus 0.01 px on the extents -- far more than f32 rounding, the 1.000001 by which K1's packed rectangle
    and fp::setup differ, and v_sqrt_f32 against sqrt can move them -- changes a tile bound or the empty / non-empty verdict.
    The bounds are monotone in the extents: the two extremes decide."""
    vw, vh = float(viewport[0]), float(viewport[1])
    h = np.ascontiguousarray(splats).view(np.float16).reshape(-1, 10).astype(np.float64)
    m00, m01 = h[:, 0] * vw, h[:, 2] * vw
    m10, m11 = -h[:, 1] * vh, -h[:, 3] * vh
    det = m00 * m11 - m01 * m10
    cx = (h[:, 4] * 0.5 + 0.5) * vw
    cy = (0.5 - h[:, 5] * 0.5) * vh
    with np.errstate(invalid="ignore", over="ignore"):
        exx = RAD * np.sqrt(m00 * m00 + m01 * m01) * 1.000001 + 1e-3
        eyy = RAD * np.sqrt(m10 * m10 + m11 * m11) * 1.000001 + 1e-3
        ok = (np.abs(det) > 0.0) & (np.abs(det) < 3.0e38) & (np.abs(cx) < 1.0e9) & (np.abs(cy) < 1.0e9) & (exx < 1.0e9) & (eyy < 1.0e9)
    exx, eyy = np.where(ok, exx, 0.0), np.where(ok, eyy, 0.0)
    cx, cy = np.where(ok, cx, 0.0), np.where(ok, cy, 0.0)
    args = (ok, vw, vh, tile_log2[0], tile_log2[1])
    rects = _tile_rects(cx, cy, exx, eyy, *args)
    lo = _tile_rects(cx, cy, exx * (1.0 - 1e-4) - 0.01, eyy * (1.0 - 1e-4) - 0.01, *args)
    hi = _tile_rects(cx, cy, exx * (1.0 + 1e-4) + 0.01, eyy * (1.0 + 1e-4) + 0.01, *args)
    undecided = (lo != rects).any(axis=1) | (hi != rects).any(axis=1)
    return rects, undecided


@dataclass
class Lists:
    tiles_x: int
    tiles_y: int
    ntiles: int               # lists of the frame (binning tiles: with `coarse`, 2 x 2 tiles each)
    rects: np.ndarray         # int64 [V, 4] by store slot, in TILES (not coarse), -1 = none
    undecided: np.ndarray     # bool [V] by store slot
    counts: np.ndarray        # int64 [V] by draw position: entries of the position
    offsets: np.ndarray       # int64 [V] exclusive prefix of counts
    d: int                    # total entries (before any cap)
    keys: np.ndarray          # int64 [d_kept] tile id per entry, draw order
    vals: np.ndarray          # uint32 [d_kept] store slot per entry, draw order
    list_len: np.ndarray      # int64 [ntiles]
    begin: np.ndarray         # uint32 [ntiles]; 0 for an empty list
    end: np.ndarray           # uint32 [ntiles]; 0 for an empty list
    entries: np.ndarray       # uint32 [d_kept]: the lists, one behind the other in tile order
    slices: np.ndarray        # int64 [ceil(d_kept / E), 3]: (s_lo, s_hi, ns) of every emit slice (emit_gen.h slice_setup)
    wg_totals: np.ndarray     # int64 [ceil(V / P)]: entries per workgroup of the binning prefix
    slice_starts: np.ndarray  # int64 [V] by draw position: multiples of E inside the position's entry range

    @property
    def d_kept(self):
        return len(self.keys)


def reference_lists(frame, viewport, tile_log2, coarse, count_cap=None):
    """The tile lists of `frame` (dict of splats [V, 20] u8 and sorted [V]) at tiles of 2^tile_log2 px; coarse: lists per 2 x 2
    tiles.  count_cap: only the first count_cap entries in draw order take part (an overflowed frame)."""
    rects, undecided = splat_rects(frame["splats"], viewport, tile_log2)
    tiles_x = -(-int(viewport[0]) // (1 << tile_log2[0]))
    tiles_y = -(-int(viewport[1]) // (1 << tile_log2[1]))
    r = rects.copy()
    if coarse:
        r = np.where(r >= 0, r >> 1, r)
        tiles_x, tiles_y = (tiles_x + 1) >> 1, (tiles_y + 1) >> 1
    ntiles = tiles_x * tiles_y
    order = np.asarray(frame["sorted"]).astype(np.int64)
    v = len(order)
    r = r[order]                                                       # by draw position
    some = r[:, 0] >= 0
    wd = np.where(some, r[:, 2] - r[:, 0] + 1, 0)
    counts = wd * np.where(some, r[:, 3] - r[:, 1] + 1, 0)
    offsets = np.cumsum(counts) - counts
    d = int(counts.sum())
    # entries in draw order: per position rows top to bottom, columns left to right
    pos = np.repeat(np.arange(v, dtype=np.int64), counts)
    k = np.arange(d, dtype=np.int64) - offsets[pos]
    keys = (r[pos, 1] + k // np.maximum(wd[pos], 1)) * tiles_x + r[pos, 0] + k % np.maximum(wd[pos], 1)
    kept = d if count_cap is None else min(d, int(count_cap))
    pos, keys = pos[:kept], keys[:kept]
    vals = order[pos].astype(np.uint32)
    by_tile = np.argsort(keys, kind="stable")
    list_len = np.bincount(keys, minlength=ntiles).astype(np.int64)
    run = np.cumsum(list_len) - list_len
    begin = np.where(list_len > 0, run, 0).astype(np.uint32)           # an empty list: (0, 0), tile::range_begin's encoding
    end = np.where(list_len > 0, run + list_len, 0).astype(np.uint32)
    # the emit slices: positions [s_lo, s_hi] own the entries [m E, min((m + 1) E, d_kept))
    m = np.arange(-(-kept // E), dtype=np.int64)
    s_lo = pos[m * E] if kept else np.zeros(0, dtype=np.int64)
    nxt = (m + 1) * E
    s_hi = np.where(nxt < kept, pos[np.minimum(nxt, max(kept - 1, 0))], v - 1) if kept else np.zeros(0, dtype=np.int64)
    slices = np.stack([s_lo, s_hi, s_hi - s_lo + 1], axis=1) if kept else np.zeros((0, 3), dtype=np.int64)
    pad = np.zeros(-(-v // P) * P, dtype=np.int64)
    pad[:v] = counts
    last = offsets + counts - 1
    starts = np.where(counts > 0, last // E - (offsets + E - 1) // E + 1, 0)
    return Lists(tiles_x, tiles_y, ntiles, rects, undecided, counts, offsets, d, keys, vals, list_len, begin, end,
                 vals[by_tile], slices, pad.reshape(len(pad) // P, P).sum(axis=1), starts)


def classes(lists, p, tile_log2):
    """(kind int8 [V], rect [V, 4]) read back from reference rectangles at the PATTERN's tile, by draw position (the frame's
    store slots are its draw positions): none -> N, one tile -> D, the whole grid -> A, anything else -> B."""
    assert (1 << tile_log2[0], 1 << tile_log2[1]) == p.tile
    r = lists.rects
    tx, ty = p.grid
    one = (r[:, 0] == r[:, 2]) & (r[:, 1] == r[:, 3])
    whole = (r[:, 0] == 0) & (r[:, 1] == 0) & (r[:, 2] == tx - 1) & (r[:, 3] == ty - 1)
    kind = np.where(r[:, 0] < 0, N_, np.where(whole & ~one, A_, np.where(one, D_, B_))).astype(np.int8)
    return kind, r


def wanted_classes(p):
    """The pattern's classes as `classes` reads them back: a block over the whole grid is an A, a 1 x 1 grid's A a dot."""
    tx, ty = p.grid
    r = p.rect.astype(np.int64)
    one = (r[:, 0] == r[:, 2]) & (r[:, 1] == r[:, 3])
    whole = (r[:, 0] == 0) & (r[:, 1] == 0) & (r[:, 2] == tx - 1) & (r[:, 3] == ty - 1)
    kind = np.where(r[:, 0] < 0, N_, np.where(whole & ~one, A_, np.where(one, D_, B_))).astype(np.int8)
    return kind, r
