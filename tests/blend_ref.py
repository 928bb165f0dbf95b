"""Marker stacks and the float64 reference of everything the FAST blend writes: what tests/test_blend_boundary_ref.py (CPU) and
tests/test_gpu_blend_boundary.py (device) share.

A marker stack is the stack scene of test_gpu_contrib._stack -- k isotropic Gaussians behind one another, index 0 nearest, so
that with bin_request=0 a tile's list is the stack and list position = index -- with a faint base opacity (T stays far above
T_MIN, nothing ends early) and a few MARKER records of a larger opacity and a colour of their own at the list positions where
k_blend's batch arithmetic changes (marker_positions).  A kernel that loses one marker, or lets two neighbouring ones change
places, then draws an image that is far outside the 2e-4 gate; test_blend_boundary_ref.py shows that from the reference alone.

The reference is composite_ref.composite_f64 over the frame's own records, draw order and z plane (reference()); its `drop=` and
`swap=` mutate the walk.  One walk per frame is shared by every launch form of that frame (_REF_CACHE)."""
import hashlib

import numpy as np

import composite_ref
from websplat import synth

T_MIN = 2.0 ** -14
FOCAL = 320.0       # pixels; the camera sits at z = -3 and looks down +z (x right, y down)
CAM_DIST = 3.0
SH_C0 = 0.28209479177387814
GATE = 2e-4         # |device - float64| per colour channel and for alpha (test_gpu_composite._check_f64)
GATE_DEPTH = 1e-4   # x max |z| (test_gpu_aux._check_against_f64)
NEAR_HALF = 1e-4    # the median is exact unless the reference's crossing lies this close to T = 0.5
STAGE = {(4, 4): 512, (4, 2): 512, (2, 2): 256}  # records per staged batch of a tile shape (blend_tile.h Geometry)
FORMATS = ("rgba32float", "rgba16float", "rgba8unorm")


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def marker_positions(k, stage):
    """List positions, counted from the near end, at which the staging changes batch (STAGE), sub-round or piece (256), the
    walk changes group (4) or wave-size chunk (64), and the two ends."""
    s = stage
    want = {0, 1, 3, 4, 63, 64, 65, 255, 256, 257, s - 1, s, s + 1, s + 255, s + 256, s + 257, 2 * s - 1, 2 * s, k - 1}
    return sorted(p for p in want if 0 <= p < k)


def marker_opacities(n, c):
    """Opacities b_0 .. b_{n-1} of n markers behind one another with b_j sqrt(T_j) = c at the centre of the stack (T_j = the
    transmittance in front of marker j, the base records left out).  What exchanging markers j and j + 1 moves the colour by is
    b_j b_{j+1} T_j |colour_j - colour_{j+1}|, about c^2 |..| wherever the pair stands: with one opacity for all, or one weight
    b_j T_j for all, either the last pairs of a long stack or the first would be invisible."""
    b, T = [], 1.0
    for _ in range(n):
        b.append(min(c / np.sqrt(T), 0.9))
        T *= 1.0 - b[-1]
    return np.array(b)


def _marker_colours(n, rng):
    """One colour per marker, random, but every colour channel alternates between a low (0 .. 0.1) and a high (0.9 .. 1) value
    from one marker to the next: exchanging two neighbouring markers moves every channel by at least 0.8 of their weight."""
    phase = rng.integers(0, 2, size=3)
    hi = ((np.arange(n)[:, None] + phase[None, :]) & 1).astype(bool)
    return np.where(hi, rng.uniform(0.9, 1.0, (n, 3)), rng.uniform(0.0, 0.1, (n, 3)))


def marker_stack(k, base, marker, positions, sigma_px, centre_px, viewport=(32, 32), seed=None, z_range=(-0.25, 0.25)):
    """PLY rows (synth._rows) of k isotropic Gaussians at distinct depths, index 0 nearest, every one projected to the pixel
    position `centre_px` with a standard deviation of `sigma_px` pixels.  Opacity `base`, except the records at `positions`:
    `marker` (one value, or one per position), with the colours of _marker_colours; the base records' colours are random."""
    w, h = viewport
    rng = np.random.default_rng(k if seed is None else seed)
    z = np.linspace(z_range[0], z_range[1], k) if k > 1 else np.array([0.5 * (z_range[0] + z_range[1])])
    depth = CAM_DIST + z
    xyz = np.stack([(centre_px[0] - 0.5 * w) * depth / FOCAL, (centre_px[1] - 0.5 * h) * depth / FOCAL, z], axis=1).astype(np.float32)
    colour = rng.uniform(0.2, 0.8, size=(k, 3))
    opacity = np.full(k, float(base))
    positions = list(positions)
    if positions:
        colour[positions] = _marker_colours(len(positions), rng)
        opacity[positions] = np.broadcast_to(np.asarray(marker, dtype=np.float64), (len(positions),))
    f_dc = ((colour - 0.5) / SH_C0).astype(np.float32)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (k, 1))
    log_scale = np.repeat(np.log(sigma_px * depth / FOCAL)[:, None], 3, axis=1).astype(np.float32)
    logit = np.log(opacity / (1.0 - opacity)).astype(np.float32)
    return synth._rows(xyz, f_dc, np.zeros((k, 45), np.float32), logit, log_scale, rot)


def place(stacks, viewport):
    """Several marker stacks in one viewport: `stacks` = keyword dicts of marker_stack (without viewport); a stack of k = 0 is
    left out.  Stack s lies z_shift = s * 1e-4 behind stack 0, so no two records of the frame share a depth.  Returns
    (rows, spans): spans[s] = (first row, one past the last row) of stack s."""
    rows, spans, at = [], [], 0
    for s, kw in enumerate(stacks):
        kw = dict(kw)
        k = kw.pop("k")
        if k:
            kw.setdefault("seed", 1000 * s + k)
            rows.append(marker_stack(k, viewport=viewport, z_range=(-0.25 + s * 1e-4, 0.25 + s * 1e-4), **kw))
        spans.append((at, at + k))
        at += k
    return np.concatenate(rows, axis=0), spans


def camera_json(viewport):
    return synth.look_at_camera(0, [0.0, 0.0, -CAM_DIST], [0.0, 0.0, 0.0], viewport[0], viewport[1], FOCAL, FOCAL)


def device_scene(ws, rows, viewport):
    """(GenericGaussianPointCloud, SplattingArgs) of `rows` under the stack camera, as test_gpu_contrib sets its stack up."""
    w, h = viewport
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, 3)
    cj = camera_json(viewport)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
    # (the cloud's own box is a segment of the optical axis, for k = 1 a point: near / far fitted to it touch the Gaussians)
    cam.fit_near_far(ws.Aabb([-1, -1, -1], [1, 1, 1]))
    return gpc, ws.SplattingArgs(camera=cam, viewport=(w, h), max_sh_deg=3)


def oracle_frame(oracle, rows, viewport):
    """The frame of device_scene without a device: K1 and the depth sort of the oracle.  dict(splats, sorted, src_index, z):
    as ws.GaussianRenderer.download_frame(with_src_index=True) has them, and z = the f32 view-space depth per store slot."""
    w, h = viewport
    g, sh = oracle.ply_rows_convert(rows, 3)
    bbox, center, _ = oracle.pointcloud_stats(g, 28, oracle.make_aabb([0, 0, 0], [0, 0, 0]))
    cj = camera_json(viewport)
    cam = oracle.scene_camera_to_perspective(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
    oracle.fit_near_far(cam, oracle.make_aabb([-1, -1, -1], [1, 1, 1]))
    cu = oracle.camera_uniform(cam, w, h)
    splats, keys, src = oracle.preprocess(g, sh, cu, oracle.settings_uniform(bbox, center))
    _, order = oracle.sort_pairs(keys, np.arange(len(keys), dtype=np.uint32))
    v = np.array(list(cu.view), dtype=np.float32)  # view[c * 4 + r], column-major
    xyz = np.ascontiguousarray(rows[:, :3], dtype=np.float32)[src]
    z = ((v[2] * xyz[:, 0] + v[6] * xyz[:, 1]) + v[10] * xyz[:, 2]) + v[14]
    return {"splats": splats, "sorted": order, "src_index": src, "z": z.astype(np.float32)}


def list_position(frame, gaussian):
    """Where Gaussian `gaussian` (a row of the cloud) stands in the frame's draw order, counted from the near end."""
    near_to_far = frame["src_index"][frame["sorted"].astype(np.int64)[::-1]]
    (hit,) = np.nonzero(near_to_far == gaussian)
    assert len(hit) == 1, f"Gaussian {gaussian} is not in the frame"
    return int(hit[0])


def falloff(frame, width, height, slot):
    """exp(-a) of the record in store slot `slot` at every pixel, 0 outside its cut-off: the share of its opacity it has there."""
    one = {"splats": np.ascontiguousarray(frame["splats"][slot:slot + 1]).copy(), "sorted": np.zeros(1, dtype=np.uint32)}
    h16 = one["splats"].view(np.float16).reshape(1, 10)
    alpha = float(h16[0, 9])
    _, T, _ = composite_ref.composite_f64(one, None, width, height)
    return (1.0 - T) / min(alpha, 0.99) if alpha > 0 else np.zeros((height, width))


def quadrants(mask_or_plane, reduce=np.max):
    """[H / 8, W / 8] of `reduce` over the 8 x 8 blocks (one wave of the FAST blend each) of an [H, W] plane."""
    h, w = mask_or_plane.shape
    return reduce(reduce(mask_or_plane.reshape(h // 8, 8, w // 8, 8), axis=3), axis=1)


# ---- the reference -----------------------------------------------------------------------------------------------------------
_REF_CACHE = {}  # (frame bytes, z, occluder, drop, swap) -> reference: K1 and the depth sort do not depend on the launch form


def _digest(*arrays):
    d = hashlib.sha1()
    for a in arrays:
        d.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


def reference(frame, z, width, height, occluder=None, drop=None, swap=None):
    """The float64 walk of a frame over a transparent black target: dict(C [H, W, 4] premultiplied, T, undecided) and, with a z
    plane, (wz, wsum, depth, median, tcross, first_below) of composite_f64's `planes`.  over() puts C over a target."""
    key = (_digest(frame["splats"], frame["sorted"], z, occluder), width, height, drop, swap)
    hit = _REF_CACHE.get(key)
    if hit is not None:
        return hit
    planes = {} if z is not None else None
    C, T, undecided = composite_ref.composite_f64(frame, z, width, height, occluder=occluder, drop=drop, swap=swap, planes=planes)
    ref = {"C": C, "T": T, "undecided": undecided}
    if planes is not None:
        ref.update(planes)
        ref["depth"] = np.where(planes["wsum"] > 0, planes["wz"] / np.where(planes["wsum"] > 0, planes["wsum"], 1.0), 0.0)
    _REF_CACHE[key] = ref
    return ref


def record_weights(frame, width, height):
    """b[slot] = min(0.99, exp(-a) alpha) of every record at every pixel, [n, H, W]: composite_f64 of each record alone."""
    n = len(frame["splats"])
    b = np.zeros((n, height, width))
    for s in range(n):
        one = {"splats": frame["splats"][s:s + 1], "sorted": np.zeros(1, dtype=np.uint32)}
        b[s] = 1.0 - composite_ref.composite_f64(one, None, width, height)[1]
    return b


def walk(frame, b, drop=None, swap=None, box=None):
    """(C, T) of composite_f64(frame, drop=, swap=) from record_weights' planes, without walking record by record: what the CPU
    test tries every marker and marker pair of a frame with (it checks this walk against composite_f64's, mutated and not).
    box = (rows, columns), two slices: only those pixels, and only the records that reach them."""
    order = frame["sorted"].astype(np.int64)[::-1].copy()
    if swap is not None:
        order[swap[0]], order[swap[1]] = order[swap[1]], order[swap[0]]
    if drop is not None:
        order = np.delete(order, drop)
    if box is not None:
        b = b[:, box[0], box[1]]
        order = order[b[order].any(axis=(1, 2))]
    if not len(order):
        return np.zeros(b.shape[1:] + (4,)), np.ones(b.shape[1:])
    bb = b[order]
    after = np.cumprod(1.0 - bb, axis=0)
    w = bb.copy()
    w[1:] *= after[:-1]
    rgb = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)[order, 6:9]
    C = np.concatenate([np.tensordot(w, rgb, axes=(0, 0)), w.sum(axis=0)[..., None]], axis=2)
    return C, after[-1]


def footprint_box(g):
    """The smallest box of whole 8 x 8 quadrants around the pixels where `g` (falloff) is not 0, as (rows, columns)."""
    ys, xs = np.nonzero(g)
    return slice(ys.min() // 8 * 8, ys.max() // 8 * 8 + 8), slice(xs.min() // 8 * 8, xs.max() // 8 * 8 + 8)


def over(ref, target, fmt="rgba32float"):
    """C + T dst: dst = a background (4 values) or an [H, W, 4] image already decoded to float; unorm targets clamp."""
    out = ref["C"] + ref["T"][..., None] * np.asarray(target, dtype=np.float64)
    return np.clip(out, 0.0, 1.0) if fmt == "rgba8unorm" else out


# ---- the gate ------------------------------------------------------------------------------------------------------------------
def decode(fmt, image):
    """A downloaded target as float64."""
    if fmt == "rgba8unorm":
        return image.astype(np.float64) / 255.0
    return image.astype(np.float64)


def colour_tolerance(fmt, want):
    """2e-4 against float64, plus -- on the 16-bit and 8-bit targets -- half a unit in the last place of the target format at
    the reference's value: the one rounding at the store."""
    if fmt == "rgba32float":
        return np.full(np.shape(want), GATE)
    if fmt == "rgba8unorm":
        return np.full(np.shape(want), GATE + 0.5 / 255.0)
    mag = np.maximum(np.abs(want), 2.0 ** -14)  # (below the smallest normal binary16 the spacing stays 2^-24)
    return GATE + 0.5 * 2.0 ** (np.floor(np.log2(mag)) - 10.0)


def colour_errors(fmt, image, want):
    """(largest |device - reference|, largest excess over the tolerance -- <= 0 passes) over every pixel and channel."""
    d = np.abs(decode(fmt, image) - want)
    return float(d.max()), float((d - colour_tolerance(fmt, want)).max())


def plane_errors(got, ref, zmax):
    """The planes of render_aux against the reference: dict of (largest error, passes) per plane present in `got`.  alpha
    within 2e-4; depth within 1e-4 zmax; the median the exact f32 z, except where the reference's crossing lies within 1e-4 of
    T = 0.5 (there either neighbour of the crossing is right, and nothing is asserted)."""
    out = {}
    if "alpha" in got:
        e = float(np.abs(got["alpha"].astype(np.float64) - (1.0 - ref["T"])).max())
        out["alpha"] = (e, e <= GATE)
    if "depth" in got:
        e = float(np.abs(got["depth"].astype(np.float64) - ref["depth"]).max())
        out["depth"] = (e, e <= GATE_DEPTH * zmax)
    if "median_depth" in got:
        wrong = (got["median_depth"] != ref["median"].astype(np.float32)) & ~(ref["tcross"] < NEAR_HALF)
        out["median_depth"] = (float(wrong.sum()), not wrong.any())
    return out


# ---- the frames of the boundary tests --------------------------------------------------------------------------------------
# One registry for the CPU test (which shows, from the reference alone, that every frame exposes a lost or exchanged marker) and
# the device test (which renders them): a frame is named by its builder and arguments, and built once.
SHAPES = {"4x4": (4, 4), "4x2": (4, 2), "2x2": (2, 2)}
SWEEP = {"4x4": (1, 255, 256, 257, 511, 512, 513, 768, 769, 1024, 1025), "4x2": (1, 255, 256, 257, 511, 512, 513, 768, 769, 1024, 1025),
         "2x2": (1, 255, 256, 257, 512, 513)}
MARKER_C = 0.09      # marker_opacities' c of the faint frames: 19 markers leave T = 0.02 at the centre
BASE = 1e-4          # the base records' opacity: 1025 of them leave T = 0.9
COVERED = 0.6        # a quadrant counts as covered by a stack where some pixel gives its records this share of their opacity
FULL_SIGMA = 16.0    # pixels: the corner quadrants of a 32 x 32 viewport still get 0.75 of a centred record's opacity


class Spec:
    """rows + viewport of one frame, and what the tests need to know of it: `stacks` = dicts(first, k, positions, centre, sigma)
    per stack, `stage` = the batch size its markers stand around, `faint` = nothing saturates."""

    def __init__(self, name, rows, viewport, stacks, stage, faint=True):
        self.name, self.rows, self.viewport, self.stacks, self.stage, self.faint = name, rows, viewport, stacks, stage, faint

    def reach(self, st):
        """How far from its centre the kept ellipse of a stack's records ends, in pixels: sqrt(2 CUT_A) standard deviations of
        the dilated Gaussian (K1 adds the 0.3 px^2 kernel)."""
        return np.sqrt(2.0 * 2.0 * 2.3539888583335364 * (st["sigma"] ** 2 + 0.3))

    def list_lengths(self, shape, coarse=False):
        """What tile_stats()["list_len"] has to be, row-major over the binning tiles (the blend's tile of `shape`, or 2 x 2 of
        them): the records of every stack whose kept ellipse reaches a pixel centre of the tile (footprint.h).  Every frame keeps
        its ellipses at least 0.25 px clear of the nearest pixel centre of a tile they do not reach and 0.25 px past it where they
        do, by the distance and along each axis alike, so that an exact footprint and a bounding-box one list the same records."""
        tw, th = (t * (2 if coarse else 1) for t in tile_px(shape))
        w, h = self.viewport
        out = []
        for ty in range(-(-h // th)):
            for tx in range(-(-w // tw)):
                n = 0
                for st in self.stacks:
                    dx = max(tx * tw + 0.5 - st["centre"][0], 0.0, st["centre"][0] - (tx + 1) * tw + 0.5)
                    dy = max(ty * th + 0.5 - st["centre"][1], 0.0, st["centre"][1] - (ty + 1) * th + 0.5)
                    r = self.reach(st)
                    for d in (np.hypot(dx, dy), max(dx, dy)):
                        assert abs(d - r) >= 0.25, (self.name, shape, tx, ty, d, r)
                    n += st["k"] if np.hypot(dx, dy) < r else 0
                out.append(n)
        return np.array(out, dtype=np.uint32)


_SPECS = {}


def _spec(name, build):
    if name not in _SPECS:
        _SPECS[name] = build(name)
    return _SPECS[name]


def _one(name, k, stage, sigma, centre, viewport=(32, 32), c=MARKER_C, base=BASE, positions=None):
    pos = marker_positions(k, stage) if positions is None else positions
    if k == 1:
        # ONE Gaussian at the world's origin is a cloud whose bounding box has radius 0: K1's fade-in divides by it, and the
        # NaN scales the Gaussian down to the dilation kernel.  Half a pixel off the axis the box (grown from the origin) has a
        # radius, and the Gaussian sits on a pixel centre.
        centre = (centre[0] - 0.5, centre[1] - 0.5)
    rows = marker_stack(k, base, marker_opacities(len(pos), c), pos, sigma, centre, viewport)
    return Spec(name, rows, viewport, [dict(first=0, k=k, positions=pos, centre=centre, sigma=sigma)], stage)


def _several(name, stacks, viewport, stage):
    """stacks: dicts(k, sigma, centre [, positions]); markers as _one."""
    kws, info = [], []
    for s in stacks:
        pos = s.get("positions", marker_positions(s["k"], stage))
        kws.append(dict(k=s["k"], base=BASE, marker=marker_opacities(len(pos), MARKER_C), positions=pos, sigma_px=s["sigma"],
                        centre_px=s["centre"]))
        info.append(dict(k=s["k"], positions=pos, centre=s["centre"], sigma=s["sigma"]))
    rows, spans = place(kws, viewport)
    for i, sp in zip(info, spans):
        i["first"] = sp[0]
    return Spec(name, rows, viewport, info, stage)


def full(k, stage):
    """Case a (and d, g): one stack over the whole 32 x 32 viewport; every quadrant of every tile walks all k."""
    return _spec(f"full-s{stage}-k{k}", lambda n: _one(n, k, stage, FULL_SIGMA, (16.0, 16.0)))


def tile_px(shape):
    return 8 * SHAPES[shape][0], 8 * SHAPES[shape][1]


def sparse(k, shape, sigma):
    """Case b: a narrow stack centred on the pixel corner at the centre of tile (0, 0).  sigma = 5 px: the cut-off (3.07 sigma)
    reaches every quadrant of a 32 x 32 tile, but only the four central ones get a visible share; sigma = 2.4 px (the cut-off ends 7.6 px
    from the centre): only those four quadrants' bits are set, the others only stage."""
    tw, th = tile_px(shape)
    return _spec(f"sparse-{shape}-sigma{sigma:g}-k{k}", lambda n: _one(n, k, STAGE[SHAPES[shape]], sigma, (0.5 * tw, 0.5 * th)))


SPARSE_SIGMAS = (5.0, 2.4)
SHORT = (1, 2, 3, 5)


def single(shape, short):
    """Case b: a stack of STAGE + 1 centred in ONE quadrant of tile (0, 0) and a second one of `short` records, all markers, in
    another: that wave's list has a length that is no multiple of four inside a batch of the tile's that is."""
    tw, th = tile_px(shape)
    stage = STAGE[SHAPES[shape]]
    main = (4.0, 4.0) if shape == "2x2" else (12.0, 4.0 if shape == "4x2" else 12.0)
    other = (tw - 4.0, th - 4.0)
    return _spec(f"single-{shape}-short{short}", lambda n: _several(n, [
        dict(k=stage + 1, sigma=2.4, centre=main), dict(k=short, sigma=2.4, centre=other, positions=list(range(short)))], (32, 32), stage))


MEDIAN_CASES = [("4x4", 513), ("4x4", 769), ("4x4", 1025), ("2x2", 257), ("2x2", 513)]


def median(shape, k):
    """Case c: markers at 0 and from STAGE - 1 on, c = 0.19, base 2e-5: at the stack's centre T is 0.63 behind the marker at
    STAGE - 1 and 0.48 behind the one at STAGE -- the median crossing of the centre pixels lies ON the first record of the
    second batch, everywhere else behind it."""
    stage = STAGE[SHAPES[shape]]
    pos = [p for p in marker_positions(k, stage) if p == 0 or p >= stage - 1]
    return _spec(f"median-{shape}-k{k}", lambda n: _one(n, k, stage, FULL_SIGMA, (16.0, 16.0), c=0.19, base=2e-5, positions=pos))


SHARED_4X4 = {"a": (513, 0, 1, 512), "b": (0, 513, 512, 1)}
SHARED_2X2 = (257, 0, 256, 1, 0, 257, 1, 256, 256, 1, 257, 0, 1, 256, 0, 257)


def shared(shape, which="a"):
    """Case e: a 64 x 64 viewport, one narrow stack per tile (four 32 x 32 tiles, sigma = 5 px; sixteen 16 x 16 ones, 2.4 px), of
    the lengths above, row-major over the tiles."""
    tw, th = tile_px(shape)
    lens = SHARED_4X4[which] if shape == "4x4" else SHARED_2X2
    nx = 64 // tw
    stacks = [dict(k=k, sigma=5.0 if shape == "4x4" else 2.4, centre=((t % nx + 0.5) * tw, (t // nx + 0.5) * th)) for t, k in enumerate(lens)]
    return _spec(f"shared-{shape}-{which}", lambda n: _several(n, stacks, (64, 64), STAGE[SHAPES[shape]]))


SATURATING = {"4x4": (600, 100.0, (-2.0, 12.0), (0, 1), (3, 1)), "4x2": (600, 100.0, (-2.0, 4.0), (0, 0), (3, 0)),
              "2x2": (400, 20.0, (-2.0, 4.0), (0, 0), (1, 0))}


def saturating(shape):
    """Case f: no markers, one wide stack centred just left of the viewport (further out K1 culls it), so that b falls from left
    to right over tile (0, 0); one opacity for all, chosen so that T reaches T_MIN half way between list positions STAGE - 1 and
    STAGE for a b half way (geometric mean) between the smallest b of quadrant `lo` and the largest of quadrant `hi` of that tile:
    (1 - opacity g)^(STAGE - 1/2) = T_MIN.  sigma = 100 px at 4x4 and 4x2 (lo and hi are 16 px apart: their b differ by 1.9 %).
    At 2x2 the tile has two quadrant columns that touch; with sigma = 100 px their b would differ by 0.05 %, as much as the f16
    rounding of the record's opacity and far less than one record's step of 1 / 256, so that frame takes sigma = 20 px (1 %)."""
    k, sigma, centre, lo, hi = SATURATING[shape]
    stage = STAGE[SHAPES[shape]]

    def build(name):
        def g_of(q):
            x = np.arange(8 * q[0], 8 * q[0] + 8)[None, :] + 0.5 - centre[0]
            y = np.arange(8 * q[1], 8 * q[1] + 8)[:, None] + 0.5 - centre[1]
            return np.exp(-(x ** 2 + y ** 2) / (2.0 * sigma ** 2))

        g = np.sqrt(g_of(lo).min() * g_of(hi).max())
        opacity = (1.0 - T_MIN ** (1.0 / (stage - 0.5))) / g
        rows = marker_stack(k, opacity, 0.0, [], sigma, centre)
        s = Spec(name, rows, (32, 32), [dict(first=0, k=k, positions=[], centre=centre, sigma=sigma)], stage, faint=False)
        s.quadrants = (lo, hi)
        return s

    return _spec(f"saturating-{shape}", build)


STRICT_K = (1, 63, 64, 65, 129)


def strict(k):
    """Case g: k_blend_strict stages 64 records at a time."""
    return full(k, 64)


def all_specs():
    """Every frame the device tests render."""
    out = []
    for shape, ks in SWEEP.items():
        stage = STAGE[SHAPES[shape]]
        out += [full(k, stage) for k in ks]
        out += [sparse(k, shape, sigma) for k in ks for sigma in SPARSE_SIGMAS]
        out += [single(shape, n) for n in SHORT]
        out.append(saturating(shape))
    out += [median(shape, k) for shape, k in MEDIAN_CASES]
    out += [shared("4x4", "a"), shared("4x4", "b"), shared("2x2")]
    out += [strict(k) for k in STRICT_K]
    seen, uniq = set(), []
    for s in out:
        if s.name not in seen:
            seen.add(s.name)
            uniq.append(s)
    return uniq
