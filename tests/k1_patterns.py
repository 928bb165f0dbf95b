"""Visibility patterns for K1's ordered compaction (web-splat_amd/csrc/preprocess.hip k_preprocess), the clouds that realise
them, and the checker that compares two prepared frames.  Pure numpy plus websplat.synth (and the ulp distance of
tests/scenes.py); the library (`ws`) and the oracle (`oracle`) are handed in by the caller, and nothing here needs a GPU.

Every frame the other K1 tests compare comes from a random cloud, where visibility is an independent coin per Gaussian: no
empty wave, no full wave, no empty item row, no empty workgroup.  Here the CALLER decides which Gaussians survive:

  mask(name, n)   bool[n], True = must survive.  K1 today: one workgroup = B = 1024 consecutive Gaussians (T = 256 threads x 4
                  items), index in block = item * 256 + thread, wave = thread >> 6 (W = 64 lanes); the exclusive prefix over
                  workgroups is a look-back of 64 predecessors per poll.  The patterns are built around these numbers and,
                  so that a kernel of another geometry is stressed as well, around periods that are not tied to them.
  cloud(...)      a point cloud whose survivors are at least 10 % INSIDE every cull threshold of K1 and whose culled are at
                  least 10 % PAST one of them (threshold_ratios() measures it, tests/test_k1_patterns.py asserts it), so no
                  f32 rounding decides visibility and `visible set == mask` holds by construction.
  compare_frame   every difference between two frames, "bitwise" or within the project's oracle bounds ("oracle")."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

from scenes import half_ulp_diff
from websplat import synth

B, T, W = 1024, 256, 64
N_BIG = 67 * B + 17                      # 68 workgroups (a look-back of two polls), the last one with 17 Gaussians
N_EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
VIEWPORTS = ((640, 480), (8256, 80))     # packed footprint rectangles | more than 256 tiles on an axis: tile counts
LAYOUTS = ("uncompressed", "compressed")
SH_DEG = 3

PATTERNS = ["all", "none", "first_only", "last_only", "lane63", "lane0", "odd_lanes", "one_wave_per_block", "alt_waves",
            "item_0", "item_1", "item_2", "item_3", "block0_only", "last_block_only", "alt_blocks", "tail_after_66_empty",
            "one_per_block", "ramp", "period_192", "period_997", "random_1", "random_50", "random_99"]
REDUCED = ["none", "last_only", "lane63", "one_wave_per_block", "item_2", "tail_after_66_empty", "ramp", "period_997",
           "random_50"]
EDGE_PATTERNS = ["all", "last_only", "random_50", "lane63"]

# ramp: block b keeps its first (RAMP_STEP * b) % 1025 Gaussians.  The step decides which counts the 67 whole blocks of N_BIG
# reach: 61 gives, of the multiples of 64, only 0, 256, 512 and 768.  363 = 64 / 3 (mod 1025): blocks 3, 6, 9 ... 48 keep
# 64, 128, 192 ... 1024 (every multiple of 64 up to the full block), blocks 51, 54 ... keep 63, 127 ... (one short of a
# multiple), block 0 keeps none and the blocks between keep counts of no particular shape (363, 726, 427, ...).
RAMP_STEP = 363


def ramp_count(b):
    return (RAMP_STEP * np.asarray(b)) % (B + 1)


def mask(name, n):
    i = np.arange(n, dtype=np.int64)
    b = i // B
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "first_only":
        return i == 0
    if name == "last_only":
        return i == n - 1
    if name == "lane63":
        return i % W == 63
    if name == "lane0":
        return i % W == 0
    if name == "odd_lanes":
        return (i & 1) == 1
    if name == "one_wave_per_block":             # 15 of the 16 (item, wave) ballots of a block are 0, one is full
        return (i % B) // W == (5 * b) % 16
    if name == "alt_waves":
        return ((i // W) & 1) == 0
    if name.startswith("item_"):                 # three item rows of every block are empty
        return (i % B) // T == int(name[5:])
    if name == "block0_only":
        return b == 0
    if name == "last_block_only":
        return b == (n - 1) // B
    if name == "alt_blocks":
        return (b & 1) == 1
    if name == "tail_after_66_empty":            # 66 workgroups of aggregate 0 in front of the first survivor
        return i >= 66 * B
    if name == "one_per_block":
        return i % B == (7 * b + 3) % B
    if name == "ramp":
        return (i % B) < ramp_count(b)
    if name == "period_192":
        return (i % 192) < 64
    if name == "period_997":
        return (i % 997) < 499
    if name.startswith("random_"):
        pct = int(name[7:])
        return np.random.default_rng(1000 + pct).random(n) < pct / 100.0
    raise KeyError(name)


def variants(name):
    """The cull causes a pattern's cloud is built with: the patterns alternate, random_50 runs in both."""
    if name == "random_50":
        return ("clip", "frustum")
    return (("clip", "frustum")[PATTERNS.index(name) & 1],)


def cases(names):
    return [(name, v) for name in names for v in variants(name)]


# ---- clouds ----------------------------------------------------------------------------------------------------------------
CAM_Z = -3.0                 # synth.camera_c1: at (0, 0, -3), looking along +z, no rotation
INSIDE = 0.9                 # survivors: at most 0.9 x every threshold
CLIP_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@functools.lru_cache(maxsize=4)
def _base_rows(n):
    rows = synth.scene_c1(n=n, seed=77, sh_deg=SH_DEG)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=4)
def _base_blobs(n):
    # the shapes of tests/test_gpu_preprocess.py::test_k1c_vs_oracle; scaling_factor = exp(0 * i8) = 1 on both sides: no libm
    # call is left, every field compares to the ulp.  The codebook then holds the absolute covariances, so it is scaled by
    # 2^-10 (exact in f16 but for subnormals, which both sides read alike): sigma <= 1/32 of a unit, the size of scene_c1's.
    blobs = synth.compressed_blobs(n=n, n_geometry=1024, n_sh=777, seed=78, sh_deg=SH_DEG)
    blobs["sh"][:64] = 0x80
    blobs["quant"]["scaling_factor"] = (0, 0.0)
    cov = blobs["covars"].view(np.float16).astype(np.float32) * np.float32(2.0 ** -10)
    blobs["covars"] = cov.astype(np.float16).view(np.uint8).reshape(-1, 12)
    for a in (blobs["gaussians"], blobs["covars"], blobs["sh"]):
        a.setflags(write=False)
    return blobs


def _tans(viewport):
    w, h = viewport
    return 0.5, h / (2.0 * w)          # (w / 2) / fx and (h / 2) / fy with fx = fy = w


tans, base_blobs = _tans, _base_blobs      # (used by tests/k1_edges.py as well)


def _positions(base_xyz, m, variant, viewport):
    """Survivors: base_xyz (in [-1, 1]^3) shrunk into [-0.9, 0.9]^3 and, in y, into 0.9 x the 1.2 w cull bound at the nearest
    depth (0.85 at 640 x 480, 0.011 at 8256 x 80).  Culled: the same, then moved past ONE threshold, the cause going round
    over the culled indices."""
    tx, ty = _tans(viewport)
    zmin = -INSIDE - CAM_Z                                            # nearest view depth of a survivor: 2.1
    ext = np.array([min(INSIDE, INSIDE * 1.2 * tx * zmin), min(INSIDE, INSIDE * 1.2 * ty * zmin), INSIDE])
    xyz = base_xyz.astype(np.float64) * ext
    culled = np.nonzero(~m)[0]
    j = np.arange(len(culled))
    frac = (j * 0.6180339887498949) % 1.0                             # how far past the threshold, spread over [0, 1)
    p = xyz[culled]
    if variant == "clip":
        # 10-20 % beyond one of the six faces of the clipping box [-1, 1]^3 in turn, and (where the viewport is wide enough
        # for that at all: every face at 640 x 480, the x and z faces at 8256 x 80) still inside the frustum
        cause = j % 6
        axis, sign = cause // 2, np.where(cause & 1, -1.0, 1.0)
        side = axis < 2
        p[side, 2] = np.abs(p[side, 2])                               # x / y faces: view depth >= 3, where 1.2 is inside
        near = cause == 5                                             # z = -1.1 .. -1.2: view depth 1.8, a narrower frustum
        p[near, 0] *= 0.8
        p[near, 1] *= 0.8
        p[j, axis] = sign * (1.1 + 0.1 * frac)
    elif variant == "frustum":
        # behind the camera | beyond +1.2 w in x | -1.2 w in x | +1.2 w in y | -1.2 w in y, each 10-30 % past
        cause = j % 5
        behind = cause == 0
        p[behind, 2] = CAM_Z - (0.3 + 0.6 * frac[behind])
        zc = p[:, 2] - CAM_Z
        for c, ax, sg, t in ((1, 0, 1.0, tx), (2, 0, -1.0, tx), (3, 1, 1.0, ty), (4, 1, -1.0, ty)):
            k = cause == c
            p[k, ax] = sg * 1.2 * t * zc[k] * (1.1 + 0.2 * frac[k])
    else:
        raise KeyError(variant)
    xyz[culled] = p
    return xyz.astype(np.float32)


def _bbox(ws, variant, viewport):
    """One bounding box per (variant, viewport), holding every position _positions() can produce: the uniforms (near / far,
    scene extend, the default clip box) are then the same for every pattern and every size."""
    if variant == "clip":
        return ws.Aabb([-1.25, -1.25, -1.25], [1.25, 1.25, 1.25])
    tx, ty = _tans(viewport)
    zmax = INSIDE - CAM_Z
    bx = 1.2 * tx * zmax * 1.3 + 0.1
    by = max(INSIDE, 1.2 * ty * zmax * 1.3) + 0.1
    return ws.Aabb([-bx, -by, CAM_Z - 1.0], [bx, by, 1.5])


@dataclass
class Cloud:
    name: str
    n: int
    layout: str
    variant: str
    viewport: tuple
    mask: np.ndarray          # bool[n]
    xyz: np.ndarray           # float32 [n, 3], as the device reads them
    gpc: object               # ws.GenericGaussianPointCloud (the host cloud)
    blobs: Optional[dict]     # compressed: synth.compressed_blobs' dict with the moved positions
    camera: object            # ws.PerspectiveCamera
    args: object              # ws.SplattingArgs

    @property
    def compressed(self):
        return self.layout == "compressed"

    def uniforms(self, oracle, args=None):
        """(camera uniform, settings uniform) for the oracle, built on the host alone; the GPU tests assert that the settings
        uniform is byte-equal to the library's (PointCloud.settings_uniform)."""
        args = args or self.args
        cu = oracle.copy_struct(oracle.CameraUniform, args.camera.uniform(args.viewport))
        rs = oracle.settings_uniform(oracle.make_aabb(self.gpc.aabb.min, self.gpc.aabb.max), self.gpc.center,
                                     max_sh_deg=args.max_sh_deg, clipping_box=args.clipping_box)
        return cu, rs

    def oracle_frame(self, oracle, args=None):
        cu, rs = self.uniforms(oracle, args)
        if self.compressed:
            q = oracle.make_quantization(self.blobs["quant"])
            splats, keys, src = oracle.preprocess_compressed(self.blobs["gaussians"], self.blobs["sh"], self.blobs["covars"], q,
                                                             SH_DEG, cu, rs)
        else:
            splats, keys, src = oracle.preprocess(self.gpc.gaussians, self.gpc.sh_coefs, cu, rs)
        _, order = oracle.sort_pairs(keys, np.arange(len(keys), dtype=np.uint32))
        return {"num_visible": len(keys), "splats": splats, "keys": keys, "src_index": src, "sorted": order}


def cloud(ws, name, n, layout="uncompressed", variant=None, viewport=(640, 480)):
    """The cloud of pattern `name` over n Gaussians: (host cloud, camera, SplattingArgs, mask) and what the tests need beside
    them, as one Cloud.  Visible Gaussians are rows of synth.scene_c1 (compressed: synth.compressed_blobs, built into a point
    cloud as tests/test_gpu_preprocess.py::_compressed_pc does); culled ones keep every other field and get a new position."""
    variant = variant or variants(name)[0]
    viewport = (int(viewport[0]), int(viewport[1]))
    m = mask(name, n)
    bbox = _bbox(ws, variant, viewport)
    center = bbox.center()
    blobs = None
    if layout == "uncompressed":
        rows = _base_rows(n).copy()
        xyz = _positions(rows[:, 0:3], m, variant, viewport)
        rows[:, 0:3] = xyz
        gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, SH_DEG)
        gpc.aabb, gpc.center = bbox, center
    elif layout == "compressed":
        base = _base_blobs(n)
        g = base["gaussians"].copy()
        xyz = _positions(g[:, 0:12].copy().view(np.float32).reshape(n, 3), m, variant, viewport)
        g[:, 0:12] = xyz.view(np.uint8).reshape(n, 12)
        blobs = dict(base, gaussians=g)
        q = ws.ws_gaussian_quantization()
        for field in ("color_dc", "color_rest", "opacity", "scaling_factor"):
            zp, s = blobs["quant"][field]
            getattr(q, field).zero_point = int(zp)
            getattr(q, field).scale = float(s)
        gpc = ws.GenericGaussianPointCloud(g, blobs["sh"], SH_DEG, n, bbox, center, compressed=True, covars=blobs["covars"],
                                           quantization=q, up=None)
    else:
        raise KeyError(layout)
    cj = synth.camera_c1(*viewport)
    cj.fx = cj.fy = float(viewport[0])
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, *viewport)
    cam.fit_near_far(bbox)
    box = ws.Aabb(list(CLIP_BOX[0]), list(CLIP_BOX[1])) if variant == "clip" else None
    args = ws.SplattingArgs(camera=cam, viewport=viewport, max_sh_deg=SH_DEG, clipping_box=box)
    return Cloud(name, n, layout, variant, viewport, m, xyz, gpc, blobs, cam, args)


def orbit_views(ws, cl, count=9):
    """`count` views of cl from synth.orbit_cameras, near / far fitted to its bbox, all with cl's clipping box: for a "clip"
    cloud the box alone decides visibility, so the mask holds for every one of them."""
    w, h = cl.viewport
    views = []
    for cj in synth.orbit_cameras(count, w, h, float(w), float(w)):
        cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
        cam.fit_near_far(cl.gpc.aabb)
        views.append(ws.SplattingArgs(camera=cam, viewport=cl.viewport, max_sh_deg=SH_DEG, clipping_box=cl.args.clipping_box))
    return views


def threshold_ratios(cl, oracle, args=None):
    """float64 [n, 9]: how far each Gaussian stands from each cull test of K1, as value / threshold (< 1 = passes, > 1 = culled):
    the six faces of the clip box, |x| and |y| against 1.2 w, and the depth range (the larger of znear / z and z / zfar: z = 0
    and z = 1 of the projected depth).  A Gaussian behind the camera gets inf in the last three."""
    args = args or cl.args
    cu, rs = cl.uniforms(oracle, args)
    view = np.array(list(cu.view), dtype=np.float64).reshape(4, 4).T      # uniform: view[c * 4 + r]
    proj = np.array(list(cu.proj), dtype=np.float64).reshape(4, 4).T
    p = np.concatenate([cl.xyz.astype(np.float64), np.ones((cl.n, 1))], axis=1)
    cs = p @ view.T
    clip = cs @ proj.T
    w = clip[:, 3]
    lo, hi = np.array(list(rs.clip_min)[:3], dtype=np.float64), np.array(list(rs.clip_max)[:3], dtype=np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    box = (cl.xyz.astype(np.float64) - mid) / half                        # in [-1, 1] inside the box
    out = np.empty((cl.n, 9))
    out[:, 0:3], out[:, 3:6] = box, -box
    front = w > 0
    safe_w = np.where(front, w, 1.0)
    out[:, 6] = np.where(front, np.abs(clip[:, 0]) / (1.2 * safe_w), np.inf)
    out[:, 7] = np.where(front, np.abs(clip[:, 1]) / (1.2 * safe_w), np.inf)
    zc = cs[:, 2]
    cam = args.camera
    out[:, 8] = np.where(front, np.maximum(cam.znear / np.where(front, zc, 1.0), zc / cam.zfar), np.inf)
    return out


# ---- the checker -----------------------------------------------------------------------------------------------------------
FIELDS = ("v1x", "v1y", "v2x", "v2y", "cx", "cy", "r", "g", "b", "a")


def _first(cond):
    return int(np.nonzero(cond)[0][0])


def compare_frame(got, want, mode="bitwise", key_ulp=2, tally=None, nan_keys=False):
    """Every difference between two frames (dicts of num_visible, splats [V, 20] u8, keys, src_index, sorted and optionally z),
    as a list of messages; empty = equal.

    mode "bitwise": every array is identical.
    mode "oracle":  the project's K1 bounds (tests/test_gpu_preprocess.py): num_visible and src_index identical, equal NaN
                    pattern, every f16 half within 1 ulp, keys within `key_ulp` units (2 for K1, 1 for K1c); `sorted` is a
                    permutation along which got's OWN keys do not decrease, ties in store order (keys that may differ by a unit
                    may legitimately order differently); z, where both frames carry one, is positive and within want["z_tol"]
                    (per slot; the oracle has no z plane: the caller puts numpy's there, tests/test_gpu_aux.py::_numpy_z).
    nan_keys (oracle mode, K1's keys = the bits of an f32): a key that is a NaN in BOTH frames counts as equal, whatever its
                    sign and payload (neither IEEE 754 nor WGSL fixes those for the result of an operation); the slots that
                    hold a NaN key must be the same.  tests/k1_edges.py: the depth of a Gaussian with a NaN position.
    tally: a dict that receives halves / halves_inexact / keys / keys_inexact / key_max of this pair (oracle mode), for the
    pooled 2 % caps the caller applies over many frames."""
    diffs = []
    v = int(want["num_visible"])
    if int(got["num_visible"]) != v:
        diffs.append(f"num_visible {got['num_visible']} != {v}")
    for name in ("splats", "keys", "src_index", "sorted"):
        if len(got[name]) != len(want[name]):
            diffs.append(f"{name}: {len(got[name])} entries != {len(want[name])}")
    if diffs:
        return diffs
    gs, ws_ = np.asarray(got["src_index"]), np.asarray(want["src_index"])
    if not np.array_equal(gs, ws_):
        s = _first(gs != ws_)
        diffs.append(f"src_index differs from slot {s}: {gs[s]} != {ws_[s]} ({int((gs != ws_).sum())} slots)")
    g = np.ascontiguousarray(got["splats"]).view(np.uint16).reshape(-1, 10)
    o = np.ascontiguousarray(want["splats"]).view(np.uint16).reshape(-1, 10)
    gk, ok = np.asarray(got["keys"]).astype(np.int64), np.asarray(want["keys"]).astype(np.int64)
    gso, wso = np.asarray(got["sorted"]), np.asarray(want["sorted"])
    if mode == "bitwise":
        if not np.array_equal(g, o):
            s = _first((g != o).any(axis=1))
            diffs.append(f"splats differ from slot {s} ({int((g != o).any(axis=1).sum())} slots)")
        if not np.array_equal(gk, ok):
            s = _first(gk != ok)
            diffs.append(f"keys differ from slot {s}: {gk[s]:#x} != {ok[s]:#x} ({int((gk != ok).sum())} slots)")
        if not np.array_equal(gso, wso):
            diffs.append(f"sorted differs from position {_first(gso != wso)}")
        if ("z" in got) != ("z" in want):
            diffs.append("z plane present in one frame only")
        elif "z" in got:
            gz, wz = np.asarray(got["z"], dtype=np.float32).view(np.uint32), np.asarray(want["z"], dtype=np.float32).view(np.uint32)
            if gz.shape != wz.shape:
                diffs.append(f"z: {gz.shape} != {wz.shape}")
            elif not np.array_equal(gz, wz):
                s = _first(gz != wz)
                diffs.append(f"z differs from slot {s} ({int((gz != wz).sum())} slots)")
        return diffs
    assert mode == "oracle", mode
    nan_g, nan_o = (g & 0x7FFF) > 0x7C00, (o & 0x7FFF) > 0x7C00
    if not np.array_equal(nan_g, nan_o):
        diffs.append(f"NaN pattern differs from slot {_first((nan_g != nan_o).any(axis=1))}")
    d = half_ulp_diff(g, o)
    d[nan_g | nan_o] = 0
    if v and d.max() > 1:
        s = _first((d > 1).any(axis=1))
        diffs.append(f"f16 field off by more than 1 ulp from slot {s}: {dict(zip(FIELDS, d.max(axis=0).tolist()))} "
                     f"({int((d > 1).any(axis=1).sum())} slots)")
    kd = np.abs(gk - ok)
    if nan_keys:
        knan_g, knan_o = (gk & 0x7FFFFFFF) > 0x7F800000, (ok & 0x7FFFFFFF) > 0x7F800000
        if not np.array_equal(knan_g, knan_o):
            diffs.append(f"NaN keys in different slots, from slot {_first(knan_g != knan_o)}")
        if tally is not None:
            tally["nan_keys_of_other_bits"] = tally.get("nan_keys_of_other_bits", 0) + int(((gk != ok) & knan_g & knan_o).sum())
        kd[knan_g & knan_o] = 0
    if v and kd.max() > key_ulp:
        diffs.append(f"keys differ by {int(kd.max())} > {key_ulp} from slot {_first(kd > key_ulp)} ({int((kd > key_ulp).sum())} slots)")
    if not np.array_equal(np.sort(gso), np.arange(v, dtype=gso.dtype)):
        diffs.append("sorted is not a permutation of 0 .. V-1")
    elif v > 1:
        k = gk[gso]
        if not np.all(k[1:] >= k[:-1]):
            diffs.append(f"keys decrease along sorted at position {_first(k[1:] < k[:-1])}")
        ties = k[1:] == k[:-1]
        if not np.all(gso[1:][ties] > gso[:-1][ties]):
            diffs.append("sorted: equal keys not in store order")
    if "z" in got and "z" in want:
        gz, wz = np.asarray(got["z"], dtype=np.float64), np.asarray(want["z"], dtype=np.float64)
        tol = np.asarray(want.get("z_tol", 0.0), dtype=np.float64)
        if gz.shape != wz.shape:
            diffs.append(f"z: {gz.shape} != {wz.shape}")
        elif v and not np.all(np.abs(gz - wz) <= tol):
            bad = ~(np.abs(gz - wz) <= tol)
            diffs.append(f"z off by more than its bound from slot {_first(bad)}: {gz[_first(bad)]!r} != {wz[_first(bad)]!r} "
                         f"({int(bad.sum())} slots)")
        if v and not np.all(gz > 0):
            diffs.append(f"z <= 0 at slot {_first(~(gz > 0))}")
    if tally is not None:
        tally["halves"] = tally.get("halves", 0) + int(d.size)
        tally["halves_inexact"] = tally.get("halves_inexact", 0) + int((d > 0).sum())
        tally["keys"] = tally.get("keys", 0) + int(kd.size)
        tally["keys_inexact"] = tally.get("keys_inexact", 0) + int((kd > 0).sum())
        tally["key_max"] = max(tally.get("key_max", 0), int(kd.max()) if v else 0)
    return diffs
