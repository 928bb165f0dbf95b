"""Python mirror of the reference's render-path API on top of the C ABI.

Names follow the reference so that tests read like web-splat code:
  WGPUContext         (src/lib.rs:57-125)        -> Context
  PerspectiveCamera   (src/camera.rs:6-35)       -> PerspectiveCamera
  Aabb                (src/pointcloud.rs:398-470)-> Aabb
  SplattingArgs       (src/renderer.rs:585-599)  -> SplattingArgs
  PointCloud          (src/pointcloud.rs:72-222) -> PointCloud
  GaussianRenderer    (src/renderer.rs:17-283)   -> GaussianRenderer
  GPURSSorter         (src/gpu_rs.rs:63-885)     -> GPURSSorter
No compute happens here; every method is one call into libwebsplat_hip.so.
"""
import contextlib
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from ._lib import lib, check
from .devmem import DeviceArray, ViewportPlanes, staged

FORMATS = {
    "rgba8unorm": (L.WS_FORMAT_RGBA8_UNORM, np.uint8, 4),
    "rgba16float": (L.WS_FORMAT_RGBA16_FLOAT, np.float16, 8),
    "rgba32float": (L.WS_FORMAT_RGBA32_FLOAT, np.float32, 16),
}


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


@dataclass
class Aabb:
    min: Sequence[float]
    max: Sequence[float]

    def to_c(self):
        a = L.ws_aabb()
        a.min[:] = [float(x) for x in self.min]
        a.max[:] = [float(x) for x in self.max]
        return a

    @staticmethod
    def from_c(a):
        return Aabb(list(a.min), list(a.max))

    def radius(self):
        a = self.to_c()
        return lib.ws_aabb_radius(C.byref(a))

    def center(self):
        return [lo + (hi - lo) / 2.0 for lo, hi in zip(self.min, self.max)]


@dataclass
class PerspectiveCamera:
    position: Sequence[float] = (0.0, 0.0, -1.0)
    rotation: Sequence[float] = (1.0, 0.0, 0.0, 0.0)  # quaternion (s, x, y, z)
    fovx: float = float(np.deg2rad(45.0))
    fovy: float = float(np.deg2rad(45.0))
    znear: float = 0.1
    zfar: float = 100.0
    fov2view_ratio: float = 1.0

    def to_c(self):
        c = L.ws_camera()
        c.position[:] = [float(x) for x in self.position]
        c.rotation[:] = [float(x) for x in self.rotation]
        c.fovx, c.fovy, c.znear, c.zfar = self.fovx, self.fovy, self.znear, self.zfar
        c.fov2view_ratio = self.fov2view_ratio
        return c

    @staticmethod
    def from_c(c):
        return PerspectiveCamera(list(c.position), list(c.rotation), c.fovx, c.fovy, c.znear, c.zfar,
                                 c.fov2view_ratio)

    def fit_near_far(self, aabb: Aabb):
        c = self.to_c()
        a = aabb.to_c()
        check(lib.ws_camera_fit_near_far(C.byref(c), C.byref(a)))
        self.znear, self.zfar = c.znear, c.zfar
        return self

    @staticmethod
    def from_scene_camera(position, rotation_rows, fx, fy, width, height):
        """scene.rs:85-108 `impl Into<PerspectiveCamera> for SceneCamera`."""
        out = L.ws_camera()
        pos = _f3(position)
        rot = (C.c_float * 9)(*[float(x) for row in rotation_rows for x in row])
        check(lib.ws_camera_from_scene(pos, rot, float(fx), float(fy), int(width), int(height), C.byref(out)))
        return PerspectiveCamera.from_c(out)

    def uniform(self, viewport):
        u = L.ws_camera_uniform()
        c = self.to_c()
        vp = (C.c_uint32 * 2)(int(viewport[0]), int(viewport[1]))
        check(lib.ws_build_camera_uniform(C.byref(c), vp, C.byref(u)))
        return u


@dataclass
class SplattingArgs:
    camera: PerspectiveCamera
    viewport: Sequence[int]
    gaussian_scaling: float = 1.0
    max_sh_deg: int = 3
    mip_splatting: Optional[bool] = None
    kernel_size: Optional[float] = None
    clipping_box: Optional[Aabb] = None
    walltime: float = 100.0  # seconds; offline callers pass Duration::from_secs(100)
    scene_center: Optional[Sequence[float]] = None
    scene_extend: Optional[float] = None
    background_color: Sequence[float] = (0.0, 0.0, 0.0, 0.0)

    def to_c(self):
        a = L.ws_splatting_args()
        a.camera = self.camera.to_c()
        a.viewport[:] = [int(self.viewport[0]), int(self.viewport[1])]
        a.gaussian_scaling = float(self.gaussian_scaling)
        a.max_sh_deg = int(self.max_sh_deg)
        a.has_mip_splatting = int(self.mip_splatting is not None)
        a.mip_splatting = int(bool(self.mip_splatting))
        a.has_kernel_size = int(self.kernel_size is not None)
        a.kernel_size = float(self.kernel_size or 0.0)
        a.has_clipping_box = int(self.clipping_box is not None)
        if self.clipping_box is not None:
            a.clipping_box = self.clipping_box.to_c()
        a.walltime_secs = float(self.walltime)
        a.has_scene_center = int(self.scene_center is not None)
        if self.scene_center is not None:
            a.scene_center[:] = [float(x) for x in self.scene_center]
        a.has_scene_extend = int(self.scene_extend is not None)
        a.scene_extend = float(self.scene_extend or 0.0)
        a.background_color[:] = [float(x) for x in self.background_color]
        return a


def stage_splat(words, viewport, tile_origin, tile_size=(16, 16)):
    """Host-side twin of the compositing pass's staging step (test hook): (rec[10], quadrant mask)."""
    w = (C.c_uint32 * 5)(*[int(x) for x in words])
    rec = (C.c_float * 10)()
    mask = C.c_uint32()
    check(lib.ws_debug_stage_splat(w, float(viewport[0]), float(viewport[1]), float(tile_origin[0]),
                                   float(tile_origin[1]), int(tile_size[0]), int(tile_size[1]), rec, C.byref(mask)))
    return np.array(rec[:], dtype=np.float32), mask.value


def footprint_tiles(words, viewport, tile_size=(32, 32)):
    """Host-side twin of the binning footprint (test hook): tile ids the splat's kept ellipse reaches, emission order."""
    w = (C.c_uint32 * 3)(*[int(x) for x in words[:3]])
    n = C.c_uint32()
    check(lib.ws_debug_footprint(w, float(viewport[0]), float(viewport[1]), int(tile_size[0]), int(tile_size[1]), 0, None,
                                 C.byref(n)))
    out = np.empty(max(n.value, 1), dtype=np.uint32)
    check(lib.ws_debug_footprint(w, float(viewport[0]), float(viewport[1]), int(tile_size[0]), int(tile_size[1]),
                                 len(out), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
    return out[:n.value]


def packed_rect(rect):
    """Test hook: (tiles, tiles at 2 x 2, the rectangle in units of 2 x 2 tiles) of a packed tile rectangle."""
    t, tc, rc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib.ws_debug_packed_rect(int(rect), C.byref(t), C.byref(tc), C.byref(rc)))
    return t.value, tc.value, rc.value


def binning_decision(request, sums, sums_coarse):
    """Test hook: 0 / 1 = the frame bins at the compositing tile / at 2 x 2 of them, from K1's per-slot sums."""
    n = len(sums)
    a = (C.c_uint32 * max(n, 1))(*[int(x) for x in sums])
    b = (C.c_uint32 * max(n, 1))(*[int(x) for x in sums_coarse])
    sh = C.c_uint32()
    check(lib.ws_debug_binning_decision(int(request), a, b, n, C.byref(sh)))
    return sh.value


def config_from_env(env=None, **overrides):
    """The harness-side translation of the WS_* environment switches into a ws_context_config (bench.py, tests, scripts).
    The LIBRARY reads no environment variable (include/websplat.h); include/websplat_env.h is the same table for C callers.
    Keyword overrides name struct fields directly (config_from_env(blend_order=1))."""
    env = os.environ if env is None else env
    c = L.ws_context_config()
    lib.ws_context_config_init(C.byref(c))

    def num(name, field):
        v = env.get(name)
        if v not in (None, ""):
            setattr(c, field, int(v))

    for name, field in (("WS_GRAPH", "use_graph"), ("WS_DEPTH_SKIP_TOP", "depth_skip_top"), ("WS_BLEND_ORDER", "blend_order"),
                        ("WS_BLEND_SPLIT", "blend_split"), ("WS_BATCH_THREADS", "batch_threads"),
                        ("WS_BATCH_QUEUE_DEPTH", "batch_queue_depth"), ("WS_BLEND_TPW_LOG2", "blend_tpw_log2"),
                        ("WS_BLEND_LDS_PAD_KB", "blend_lds_pad_kb"), ("WS_DEBUG_CUT", "debug_cut"), ("WS_CAPTURE", "capture"),
                        ("WS_DEPTH_DIGIT_BITS", "depth_digit_bits"), ("WS_DEPTH_TILE_KPT", "depth_tile_kpt"), ("WS_BLEND_ASYNC", "blend_async"), ("WS_DSORT_FAT_GRID", "exp_dsort_fat_grid"),
                        ("WS_BLEND_VARIANT", "exp_blend_variant"), ("WS_BATCH_K1", "exp_batch_k1")):
        num(name, field)
    if env.get("WS_BLEND_DMA") not in (None, ""):
        c.exp_blend_dma = 1 if int(env["WS_BLEND_DMA"]) else 0
    bs = env.get("WS_BIN_SHIFT")
    if bs is not None:
        c.bin_request = 2 if bs == "1" else (0 if bs == "0" else 1)
    shape = env.get("WS_TILE_SHAPE")
    if shape:
        qw, _, qh = shape.partition("x")
        c.tile_qw, c.tile_qh = (int(qw), int(qh)) if qw.isdigit() and qh.isdigit() else (-1, -1)  # (the library refuses what it does not have)
    c.render_views_fast_blend = 1 if env.get("WS_RENDER_VIEWS_BLEND") == "fast" else 0
    c.ply_decode_host = 1 if env.get("WS_PLY_DECODE") == "host" else 0
    c.exp_depth_sort = {"onesweep": 1, "coop": 2}.get(env.get("WS_DEPTH_SORT", ""), 0)
    c.exp_footprint_ellipse = 1 if env.get("WS_FOOTPRINT") == "ellipse" else 0
    c.exp_tile_sort_wide = 1 if env.get("WS_TILE_SORT") == "wide" else 0
    for k, v in overrides.items():
        setattr(c, k, int(v))
    return c


class Context:
    def __init__(self, device: int = 0, config=None):
        """config: a ws_context_config (config_from_env(...)); None = this process's WS_* environment, translated HERE -- the
        harness side -- because the library itself reads no environment variable."""
        h = C.c_void_p()
        cfg = config_from_env() if config is None else config
        check(lib.ws_context_create_with_config(int(device), C.byref(cfg), C.byref(h)))
        self.handle = h
        self.device = device
        self.config = cfg

    def close(self):
        if self.handle:
            lib.ws_context_destroy(self.handle)
            self.handle = None

    def sync(self, stream=None):
        check(lib.ws_sync(self.handle, C.c_void_p(stream or 0)))

    def set_host_wait(self, mode):
        """'block' (sleep until the completion interrupt: device.poll(Wait), bin/measure.rs:147) or 'spin' (HIP's default)."""
        check(lib.ws_context_set_host_wait(self.handle, {"spin": 0, "block": 1}[mode]))

    def tile_size(self):
        """(width, height) of the binning tile in pixels (32x32 unless WS_TILE_SHAPE says otherwise)."""
        w, h = C.c_uint32(), C.c_uint32()
        check(lib.ws_context_tile_size(self.handle, C.byref(w), C.byref(h)))
        return w.value, h.value

    def device_info(self):
        name = C.create_string_buffer(128)
        cus = C.c_uint32()
        mem = C.c_uint64()
        check(lib.ws_device_info(self.handle, name, 128, C.byref(cus), C.byref(mem)))
        return {"arch": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}

    # plain device buffers -------------------------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(lib.ws_device_malloc(self.handle, int(nbytes), C.byref(p)))
        return p.value

    def free(self, ptr: int):
        check(lib.ws_device_free(self.handle, C.c_void_p(ptr)))

    def upload(self, ptr: int, arr: np.ndarray, stream=None):
        arr = np.ascontiguousarray(arr)
        check(lib.ws_memcpy_h2d(self.handle, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes,
                                C.c_void_p(stream or 0)))

    def download(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(lib.ws_memcpy_d2h(self.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, None))
        return out

    def sort_selftest(self) -> bool:
        ok = C.c_int(0)
        check(lib.ws_sort_selftest(self.handle, C.byref(ok)))
        return bool(ok.value)


@dataclass
class GenericGaussianPointCloud:
    """io/mod.rs:27-43: what a loader produces (host byte blobs + metadata)."""
    gaussians: np.ndarray  # uint8, N x 28 (or N x 24 compressed)
    sh_coefs: np.ndarray   # uint8, N x 96 (or packed int8)
    sh_deg: int
    num_points: int
    aabb: Aabb
    center: Sequence[float]
    compressed: bool = False
    covars: Optional[np.ndarray] = None          # uint8, M x 12
    quantization: Optional[L.ws_gaussian_quantization] = None
    up: Optional[Sequence[float]] = None
    kernel_size: Optional[float] = None
    mip_splatting: Optional[bool] = None
    background_color: Optional[Sequence[float]] = None

    @staticmethod
    def from_ply_rows(rows: np.ndarray, sh_deg: int, **meta):
        """io/ply.rs:50-100 + io/mod.rs:63-105 through the library's host-side loader code."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        want = 14 + 3 * (int(sh_deg) + 1) ** 2  # x,y,z, n*, f_dc*, f_rest*, opacity, scale*, rot*  (io/ply.rs:54-88)
        if rows.ndim != 2 or rows.shape[1] != want:
            raise ValueError(f"from_ply_rows: sh_deg {sh_deg} needs rows of {want} floats, got shape {rows.shape}")
        n = rows.shape[0]
        g = np.empty((n, 28), dtype=np.uint8)
        s = np.empty((n, 96), dtype=np.uint8)
        check(lib.ws_ply_rows_convert(rows.ctypes.data_as(C.c_void_p), n, int(sh_deg),
                                      g.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
        aabb, center, up = pointcloud_stats(g, 28, Aabb([0, 0, 0], [0, 0, 0]))
        return GenericGaussianPointCloud(g, s, sh_deg, n, aabb, center, up=up, **meta)


def read_ply(path: str) -> GenericGaussianPointCloud:
    """io/ply.rs:28-196 PlyReader::read + io/mod.rs:63-105 through the library's host-side reader (no GPU)."""
    pp = C.POINTER(L.ws_ply_cloud)()
    check(lib.ws_ply_read(str(path).encode(), C.byref(pp)))
    try:
        c = pp.contents
        if c.num_points == 0:  # an empty vertex list reads fine in the reference too (it cannot be uploaded)
            g, sh = np.empty((0, 28), np.uint8), np.empty((0, 96), np.uint8)
        else:
            g = np.ctypeslib.as_array((C.c_uint8 * c.gaussians_bytes).from_address(c.gaussians)).copy().reshape(-1, 28)
            sh = np.ctypeslib.as_array((C.c_uint8 * c.sh_coefs_bytes).from_address(c.sh_coefs)).copy().reshape(-1, 96)
        return GenericGaussianPointCloud(
            g, sh, int(c.sh_deg), int(c.num_points), Aabb(list(c.bbox.min), list(c.bbox.max)), list(c.center),
            up=list(c.up) if c.has_up else None,
            kernel_size=c.kernel_size if c.has_kernel_size else None,
            mip_splatting=bool(c.mip_splatting) if c.has_mip_splatting else None,
            background_color=list(c.background_color) if c.has_background_color else None)
    finally:
        lib.ws_ply_free(pp)


def _hints_desc(kernel_size=None, mip_splatting=None, background_color=None):
    """a ws_pointcloud_desc that carries only the three optional header values"""
    d = L.ws_pointcloud_desc()
    d.has_mip_splatting = int(mip_splatting is not None)
    d.mip_splatting = int(bool(mip_splatting))
    d.has_kernel_size = int(kernel_size is not None)
    d.kernel_size = float(kernel_size or 0.0)
    d.has_background_color = int(background_color is not None)
    if background_color is not None:
        d.background_color[:] = [float(x) for x in background_color]
    return d


def write_ply_rows(path: str, rows: np.ndarray, sh_deg: int, **meta):
    """Raw INRIA vertex rows (N x (14 + 3 (sh_deg + 1)^2) float32) as a binary little-endian .ply through the library's host-side
    writer (ws_ply_write, no GPU); meta: kernel_size, mip_splatting, background_color, each written as a comment when given."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    want = 14 + 3 * (int(sh_deg) + 1) ** 2
    if rows.ndim != 2 or rows.shape[1] != want:
        raise ValueError(f"write_ply_rows: sh_deg {sh_deg} needs rows of {want} floats, got shape {rows.shape}")
    d = _hints_desc(**meta)
    check(lib.ws_ply_write(str(path).encode(), rows.ctypes.data_as(C.c_void_p), rows.shape[0], int(sh_deg), C.byref(d)))


def encode_ply_rows(gaussians: np.ndarray, sh_coefs: np.ndarray, sh_deg: int) -> np.ndarray:
    """The loader's blobs (N x 28, N x 96 uint8) back to INRIA vertex rows on the host (ws_ply_rows_encode, the twin of the
    kernel behind PointCloud.to_ply_rows)."""
    g = np.ascontiguousarray(gaussians, dtype=np.uint8).reshape(-1, 28)
    s = np.ascontiguousarray(sh_coefs, dtype=np.uint8).reshape(-1, 96)
    if g.shape[0] != s.shape[0]:
        raise ValueError("encode_ply_rows: gaussians and sh_coefs differ in length")
    rows = np.empty((g.shape[0], 14 + 3 * (int(sh_deg) + 1) ** 2), dtype=np.float32)
    check(lib.ws_ply_rows_encode(g.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), g.shape[0], int(sh_deg),
                                 rows.ctypes.data_as(C.c_void_p)))
    return rows


def read_npz(path: str) -> GenericGaussianPointCloud:
    """io/npz.rs:59-225 NpzReader::read + io/mod.rs:107-150 new_compressed, through the library's native reader."""
    pp = C.POINTER(L.ws_npz_cloud)()
    check(lib.ws_npz_read(str(path).encode(), C.byref(pp)))
    try:
        c = pp.contents
        g = np.ctypeslib.as_array((C.c_uint8 * c.gaussians_bytes).from_address(c.gaussians)).copy().reshape(-1, 24)
        sh = np.ctypeslib.as_array((C.c_uint8 * c.sh_coefs_bytes).from_address(c.sh_coefs)).copy()
        cv = np.ctypeslib.as_array((C.c_uint8 * c.covars_bytes).from_address(c.covars)).copy().reshape(-1, 12)
        q = L.ws_gaussian_quantization()
        C.memmove(C.byref(q), C.byref(c.quantization), C.sizeof(q))
        aabb, center, up = pointcloud_stats(g, 24, Aabb([-1, -1, -1], [1, 1, 1]))  # Aabb::unit(), io/mod.rs:119
        return GenericGaussianPointCloud(
            g, sh, int(c.sh_deg), int(c.num_points), aabb, center, compressed=True, covars=cv, quantization=q, up=up,
            kernel_size=c.kernel_size if c.has_kernel_size else None,
            mip_splatting=bool(c.mip_splatting) if c.has_mip_splatting else None,
            background_color=list(c.background_color) if c.has_background_color else None)
    finally:
        lib.ws_npz_free(pp)


def write_png(path: str, rgba: np.ndarray):
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    check(lib.ws_png_write_rgba8(str(path).encode(), w, h, rgba.ctypes.data_as(C.c_void_p), w * 4))


@dataclass
class SceneCamera:
    """scene.rs:13-24."""
    id: int
    img_name: str
    width: int
    height: int
    position: Sequence[float]
    rotation: Sequence[Sequence[float]]
    fx: float
    fy: float
    split: str = "train"

    @staticmethod
    def from_c(c):
        rot = [list(c.rotation[3 * k:3 * k + 3]) for k in range(3)]
        return SceneCamera(c.id, c.img_name.decode(), c.width, c.height, list(c.position), rot, c.fx, c.fy,
                           "test" if c.split == L.WS_SPLIT_TEST else "train")

    def to_perspective(self) -> "PerspectiveCamera":
        return PerspectiveCamera.from_scene_camera(self.position, self.rotation, self.fx, self.fy, self.width, self.height)


_SPLITS = {None: L.WS_SPLIT_ALL, "train": L.WS_SPLIT_TRAIN, "test": L.WS_SPLIT_TEST}


class Scene:
    """scene.rs:113-194 Scene."""

    def __init__(self, handle):
        self.handle = handle

    @staticmethod
    def from_json(path: str):
        h = C.c_void_p()
        check(lib.ws_scene_load_json(str(path).encode(), C.byref(h)))
        return Scene(h)

    @staticmethod
    def from_json_text(text: str):
        raw = text.encode()
        h = C.c_void_p()
        check(lib.ws_scene_from_json_text(raw, len(raw), C.byref(h)))
        return Scene(h)

    def close(self):
        if self.handle:
            lib.ws_scene_destroy(self.handle)
            self.handle = None

    def num_cameras(self):
        return lib.ws_scene_num_cameras(self.handle)

    def extend(self):
        return lib.ws_scene_extend(self.handle)

    def cameras(self, split=None):
        n = lib.ws_scene_cameras(self.handle, _SPLITS[split], 0, None)
        buf = (L.ws_scene_camera * max(n, 1))()
        lib.ws_scene_cameras(self.handle, _SPLITS[split], n, buf)
        return [SceneCamera.from_c(buf[i]) for i in range(n)]

    def camera(self, cam_id: int):
        c = L.ws_scene_camera()
        return SceneCamera.from_c(c) if lib.ws_scene_get_camera(self.handle, int(cam_id), C.byref(c)) else None

    def nearest_camera(self, pos, split=None):
        out = C.c_uint32()
        return out.value if lib.ws_scene_nearest_camera(self.handle, _f3(pos), _SPLITS[split], C.byref(out)) else None


def render_views(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, out_dir: str) -> int:
    """bin/render.rs:33-128 render_views."""
    n = C.c_uint32()
    check(lib.ws_render_views(ctx.handle, pc.handle, scene.handle, _SPLITS[split], str(out_dir).encode(), C.byref(n)))
    return n.value


def measure(ctx: "Context", pc: "PointCloud", scene: Scene, num_samples: int = 10, frames_in_flight: int = 1) -> float:
    """bin/measure.rs:27-154: average FPS over the training cameras at 2048x2048."""
    fps = C.c_float()
    check(lib.ws_measure(ctx.handle, pc.handle, scene.handle, int(num_samples), int(frames_in_flight), C.byref(fps)))
    return fps.value


def pointcloud_stats(gaussians: np.ndarray, stride: int, start: Aabb):
    start_c = start.to_c()
    bbox = L.ws_aabb()
    center = (C.c_float * 3)()
    has_up = C.c_int32()
    up = (C.c_float * 3)()
    n = gaussians.shape[0]
    check(lib.ws_pointcloud_stats(gaussians.ctypes.data_as(C.c_void_p), n, stride, C.byref(start_c), C.byref(bbox),
                                  center, C.byref(has_up), up))
    return Aabb.from_c(bbox), list(center), (list(up) if has_up.value else None)


class PointCloud:
    """pointcloud.rs:99-222 PointCloud::new(device, GenericGaussianPointCloud)."""

    def __init__(self, ctx: Context, pc: GenericGaussianPointCloud = None, _handle=None):
        self.ctx = ctx
        if _handle is not None:
            self.handle = _handle
            return
        d = L.ws_pointcloud_desc()
        g = np.ascontiguousarray(pc.gaussians)
        s = np.ascontiguousarray(pc.sh_coefs)
        d.num_points = pc.num_points
        d.sh_deg = pc.sh_deg
        d.compressed = int(pc.compressed)
        d.gaussians = g.ctypes.data
        d.gaussians_bytes = g.nbytes
        d.sh_coefs = s.ctypes.data
        d.sh_coefs_bytes = s.nbytes
        keep = [g, s]
        if pc.compressed:
            cv = np.ascontiguousarray(pc.covars)
            keep.append(cv)
            d.covars = cv.ctypes.data
            d.covars_bytes = cv.nbytes
            d.quantization = C.pointer(pc.quantization)
        d.bbox = pc.aabb.to_c()
        d.center[:] = [float(x) for x in pc.center]
        d.has_up = int(pc.up is not None)
        if pc.up is not None:
            d.up[:] = [float(x) for x in pc.up]
        d.has_mip_splatting = int(pc.mip_splatting is not None)
        d.mip_splatting = int(bool(pc.mip_splatting))
        d.has_kernel_size = int(pc.kernel_size is not None)
        d.kernel_size = float(pc.kernel_size or 0.0)
        d.has_background_color = int(pc.background_color is not None)
        if pc.background_color is not None:
            d.background_color[:] = [float(x) for x in pc.background_color]
        h = C.c_void_p()
        check(lib.ws_pointcloud_create(ctx.handle, C.byref(d), C.byref(h)))
        self.handle = h

    @staticmethod
    def from_ply_rows(ctx: Context, rows: np.ndarray, sh_deg: int, kernel_size=None, mip_splatting=None,
                      background_color=None):
        """Raw PLY vertex rows -> resident scene with the conversion (io/ply.rs:50-100) on the GPU."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        want = 14 + 3 * (int(sh_deg) + 1) ** 2
        if rows.ndim != 2 or rows.shape[1] != want:
            raise ValueError(f"from_ply_rows: sh_deg {sh_deg} needs rows of {want} floats, got shape {rows.shape}")
        d = _hints_desc(kernel_size, mip_splatting, background_color)
        h = C.c_void_p()
        check(lib.ws_pointcloud_create_from_ply_rows(ctx.handle, rows.ctypes.data_as(C.c_void_p), rows.shape[0], int(sh_deg),
                                                     C.byref(d), C.byref(h)))
        return PointCloud(ctx, _handle=h)

    def download(self):
        """(gaussians N x 28 | N x 24, sh N x 96 | None): the resident scene as loader blobs (parity tooling)."""
        n = self.num_points()
        if self.compressed():
            g = np.empty((n, 24), dtype=np.uint8)
            s = np.empty((1,), dtype=np.uint8)
            check(lib.ws_pointcloud_download(self.handle, g.ctypes.data_as(C.c_void_p), g.nbytes, s.ctypes.data_as(C.c_void_p), 0))
            return g, None
        g = np.empty((n, 28), dtype=np.uint8)
        s = np.empty((n, 96), dtype=np.uint8)
        check(lib.ws_pointcloud_download(self.handle, g.ctypes.data_as(C.c_void_p), g.nbytes, s.ctypes.data_as(C.c_void_p), s.nbytes))
        return g, s

    def to_ply_rows(self) -> np.ndarray:
        """(N, 14 + 3 (sh_deg + 1)^2) float32: the resident cloud as INRIA vertex rows, encoded on the device (websplat.h "Saving a
        point cloud"); the inverse of from_ply_rows."""
        rows = np.empty((self.num_points(), 14 + 3 * (self.sh_deg() + 1) ** 2), dtype=np.float32)
        check(lib.ws_pointcloud_encode_ply_rows(self.handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes))
        return rows

    def encode_ply_rows_device(self, d_rows: int, nbytes: int, stream=None):
        """to_ply_rows into device memory of the caller's; only enqueues on `stream` (ws_pointcloud_encode_ply_rows_device)"""
        check(lib.ws_pointcloud_encode_ply_rows_device(self.handle, C.c_void_p(d_rows), int(nbytes), C.c_void_p(stream or 0)))

    def decode_ply_rows_device(self, d_rows: int, nbytes: int, stream=None):
        """num_points device rows of this cloud's degree decoded INTO its planes; only enqueues on `stream`"""
        check(lib.ws_pointcloud_decode_ply_rows_device(self.handle, C.c_void_p(d_rows), int(nbytes), C.c_void_p(stream or 0)))

    def save_ply(self, path: str):
        """the resident cloud as an INRIA 3DGS .ply with its mip / kernel_size / background_color comments (ws_pointcloud_save_ply)"""
        check(lib.ws_pointcloud_save_ply(self.handle, str(path).encode()))

    @staticmethod
    def load_ply(ctx: Context, path: str):
        h = C.c_void_p()
        check(lib.ws_pointcloud_load_ply(ctx.handle, path.encode(), C.byref(h)))
        return PointCloud(ctx, _handle=h)

    @staticmethod
    def load_npz(ctx: Context, path: str):
        h = C.c_void_p()
        check(lib.ws_pointcloud_load_npz(ctx.handle, str(path).encode(), C.byref(h)))
        return PointCloud(ctx, _handle=h)

    @staticmethod
    def load(ctx: Context, path: str):
        """io/mod.rs:45-61 GenericGaussianPointCloud::load (magic-byte sniffing) + PointCloud::new."""
        h = C.c_void_p()
        check(lib.ws_pointcloud_load(ctx.handle, str(path).encode(), C.byref(h)))
        return PointCloud(ctx, _handle=h)

    def close(self):
        if self.handle:
            lib.ws_pointcloud_destroy(self.handle)
            self.handle = None

    def num_points(self):
        return lib.ws_pointcloud_num_points(self.handle)

    def sh_deg(self):
        return lib.ws_pointcloud_sh_deg(self.handle)

    def compressed(self):
        return bool(lib.ws_pointcloud_compressed(self.handle))

    def bbox(self) -> Aabb:
        a = L.ws_aabb()
        check(lib.ws_pointcloud_bbox(self.handle, C.byref(a)))
        return Aabb.from_c(a)

    def center(self):
        c = (C.c_float * 3)()
        check(lib.ws_pointcloud_center(self.handle, c))
        return list(c)

    def up(self):
        c = (C.c_float * 3)()
        return list(c) if lib.ws_pointcloud_up(self.handle, c) else None

    def mip_splatting(self):
        v = C.c_int32()
        return bool(v.value) if lib.ws_pointcloud_mip_splatting(self.handle, C.byref(v)) else None

    def dilation_kernel_size(self):
        v = C.c_float()
        return v.value if lib.ws_pointcloud_kernel_size(self.handle, C.byref(v)) else None

    def background_color(self):
        c = (C.c_float * 3)()
        return list(c) if lib.ws_pointcloud_background_color(self.handle, c) else None

    def settings_uniform(self, args: SplattingArgs):
        u = L.ws_settings_uniform()
        a = args.to_c()
        check(lib.ws_build_settings_uniform(C.byref(a), self.handle, C.byref(u)))
        return u

    def subset(self, indices) -> "PointCloud":
        """The Gaussians `indices` (strictly ascending) as a point cloud of its own, gathered on the device; bbox, centre, up
        and the metadata are the parent's, which may be closed first (ws_pointcloud_create_subset)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        h = C.c_void_p()
        check(lib.ws_pointcloud_create_subset(self.ctx.handle, self.handle, idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size,
                                              C.byref(h)))
        return PointCloud(self.ctx, _handle=h)


class _GaussianSums:
    """What Contrib, Grad and ShGrad share (csrc/gaussian_sums.h): the handle's life, reset and the two counters, by the entry
    points' prefix.  A subclass has its constructor's arguments, download and add."""
    _prefix = None   # "ws_contrib" | "ws_grad" | "ws_shgrad"
    _create_args = ()   # what the creator takes between num_points and the handle

    def __init__(self, ctx: Context, num_points: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(getattr(lib, self._prefix + "_create")(ctx.handle, int(num_points), *self._create_args, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            getattr(lib, self._prefix + "_destroy")(self.handle)
            self.handle = None

    def reset(self, stream=None):
        check(getattr(lib, self._prefix + "_reset")(self.handle, C.c_void_p(stream or 0)))

    def num_points(self) -> int:
        return getattr(lib, self._prefix + "_num_points")(self.handle)

    @property
    def frames(self) -> int:
        """frames added since creation / the last reset"""
        return getattr(lib, self._prefix + "_frames")(self.handle)


class Contrib(_GaussianSums):
    """Per-Gaussian contribution accumulators over frames (websplat.h "Per-Gaussian contributions"): for every Gaussian of a
    cloud of num_points, the q32 sum of its blend weights over all pixels of all frames added, and its largest weight."""
    _prefix = "ws_contrib"

    def download(self):
        """(sum float64 = sum_q32 / 2^32, sum_q32 uint64, max_weight float32), one value per Gaussian (syncs)."""
        n = self.num_points()
        q = np.empty(n, dtype=np.uint64)
        m = np.empty(n, dtype=np.float32)
        check(lib.ws_contrib_download(self.handle, n, q.ctypes.data_as(C.POINTER(C.c_uint64)), m.ctypes.data_as(C.POINTER(C.c_float))))
        return q.astype(np.float64) / L.WS_CONTRIB_SUM_SCALE, q, m

    def add(self, sum_q32, max_weight):
        """Exact merge of another accumulator's (or rank's) downloaded arrays; either may be None."""
        q = None if sum_q32 is None else np.ascontiguousarray(sum_q32, dtype=np.uint64)
        m = None if max_weight is None else np.ascontiguousarray(max_weight, dtype=np.float32)
        n = min(a.size for a in (q, m) if a is not None) if (q is not None or m is not None) else self.num_points()
        check(lib.ws_contrib_add(self.handle, q.ctypes.data_as(C.POINTER(C.c_uint64)) if q is not None else None,
                                 m.ctypes.data_as(C.POINTER(C.c_float)) if m is not None else None, n))


class Grad(_GaussianSums):
    """Per-Gaussian gradient accumulators over frames (websplat.h "Gradients of an image loss"): for every Gaussian of a cloud
    of num_points, four signed q32 sums -- dL/d(colour r, g, b) and dL/d(ln opacity) times 2^32 and the calls' scales."""
    _prefix = "ws_grad"

    def download(self) -> np.ndarray:
        """(N, 4) int64: the q32 sums of colour r, g, b and ln-opacity per Gaussian (syncs)."""
        n = self.num_points()
        q = np.empty((n, L.WS_GRAD_CHANNELS), dtype=np.int64)
        check(lib.ws_grad_download(self.handle, n, q.ctypes.data_as(C.POINTER(C.c_int64))))
        return q

    def add(self, q32):
        """Exact merge of another accumulator's (or rank's) downloaded (N, 4) int64 sums."""
        q = np.ascontiguousarray(q32, dtype=np.int64)
        if q.ndim != 2 or q.shape[1] != L.WS_GRAD_CHANNELS:
            raise ValueError(f"Grad.add: want an (N, {L.WS_GRAD_CHANNELS}) int64 array, got {q.shape}")
        check(lib.ws_grad_add(self.handle, q.ctypes.data_as(C.POINTER(C.c_int64)), q.shape[0]))


_i64p = C.POINTER(C.c_int64)


class ShGrad(_GaussianSums):
    """Per-Gaussian, per-coefficient gradient accumulators over frames (websplat.h "SH gradients"): for every Gaussian of a
    cloud of num_points and degree sh_deg, 3 (sh_deg + 1)^2 signed q32 sums dL/d(sh[k][ch]) -- coefficient 0 holds the plain
    colour sums of a Grad -- and dL/d(ln opacity)."""
    _prefix = "ws_shgrad"

    def __init__(self, ctx: Context, num_points: int, sh_deg: int):
        self._create_args = (int(sh_deg),)
        super().__init__(ctx, num_points)

    @property
    def sh_deg(self) -> int:
        return lib.ws_shgrad_sh_deg(self.handle)

    def download(self) -> dict:
        """{"sh": (N, ncoef, 3) int64, "opacity": (N,) int64}: the q32 sums per Gaussian (syncs)."""
        n, ncoef = self.num_points(), (self.sh_deg + 1) ** 2
        out = {"sh": np.empty((n, ncoef, 3), dtype=np.int64), "opacity": np.empty(n, dtype=np.int64)}
        check(lib.ws_shgrad_download(self.handle, n, out["sh"].ctypes.data_as(_i64p), out["opacity"].ctypes.data_as(_i64p)))
        return out

    def add(self, sh=None, opacity=None):
        """Exact merge of another accumulator's (or rank's) downloaded sums; either array may be left out."""
        ncoef = (self.sh_deg + 1) ** 2
        rows = []
        if sh is not None:
            sh = np.ascontiguousarray(sh, dtype=np.int64)
            if sh.ndim != 3 or sh.shape[1:] != (ncoef, 3):
                raise ValueError(f"ShGrad.add: want an (N, {ncoef}, 3) int64 array, got {sh.shape}")
            rows.append(sh.shape[0])
        if opacity is not None:
            opacity = np.ascontiguousarray(opacity, dtype=np.int64)
            if opacity.ndim != 1:
                raise ValueError(f"ShGrad.add: want an (N,) int64 array of opacity sums, got {opacity.shape}")
            rows.append(opacity.shape[0])
        if not rows:
            return
        check(lib.ws_shgrad_add(self.handle, sh.ctypes.data_as(_i64p) if sh is not None else None,
                                opacity.ctypes.data_as(_i64p) if opacity is not None else None, min(rows)))


def sh_spread_rows(q4, xyz, cam, sh_deg: int, active_deg: int) -> dict:
    """The host twin of the SH spread (ws_sh_spread_rows, no GPU needed): one frame's (N, 4) int64 Grad-layout sums, the (N, 3)
    float32 positions and the camera position (view_inv[12:15]) -> {"sh": (N, ncoef, 3) int64, "opacity": (N,) int64}."""
    q4 = np.ascontiguousarray(q4, dtype=np.int64)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    if q4.ndim != 2 or q4.shape[1] != 4 or xyz.shape != (q4.shape[0], 3) or cam.shape != (3,):
        raise ValueError("sh_spread_rows: want (N, 4) sums, (N, 3) positions and a camera position of 3")
    n, ncoef = q4.shape[0], (int(sh_deg) + 1) ** 2
    out = {"sh": np.zeros((n, ncoef, 3), dtype=np.int64), "opacity": np.zeros(n, dtype=np.int64)}
    fp = C.POINTER(C.c_float)
    check(lib.ws_sh_spread_rows(q4.ctypes.data_as(_i64p), xyz.ctypes.data_as(fp), cam.ctypes.data_as(fp), n, int(sh_deg), int(active_deg),
                                out["sh"].ctypes.data_as(_i64p), out["opacity"].ctypes.data_as(_i64p)))
    return out


class GeomGrad(_GaussianSums):
    """Per-Gaussian geometry gradient accumulators over frames (websplat.h "Geometry gradients"): for every Gaussian of a cloud
    of num_points, float64 sums of dL/d(position), dL/d(the six stored covariance elements) and the norm of the screen-space
    positional gradient, and the number of frames that counted a pair of it."""
    _prefix = "ws_geomgrad"
    _FIELDS = (("position", (3,), np.float64), ("covariance", (6,), np.float64), ("screen_norm", (), np.float64), ("seen", (), np.uint64))

    def download(self) -> dict:
        """{"position": (N, 3), "covariance": (N, 6), "screen_norm": (N,) float64, "seen": (N,) uint64} (syncs)."""
        n = self.num_points()
        out = {k: np.empty((n,) + shape, dtype=dt) for k, shape, dt in self._FIELDS}
        check(lib.ws_geomgrad_download(self.handle, n, *(out[k].ctypes.data_as(L._u64p if dt is np.uint64 else L._f64p) for k, _, dt in self._FIELDS)))
        return out

    def add(self, position=None, covariance=None, screen_norm=None, seen=None):
        """Add another accumulator's (or rank's) downloaded sums, in the order given (float64 addition: exact only for `seen`);
        any array may be left out."""
        given = {"position": position, "covariance": covariance, "screen_norm": screen_norm, "seen": seen}
        ptrs, rows = [], []
        for k, shape, dt in self._FIELDS:
            a = given[k]
            if a is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape[1:] != shape:
                raise ValueError(f"GeomGrad.add: want an (N,{' ' + str(shape[0]) if shape else ''}) {np.dtype(dt).name} array for {k}, got {a.shape}")
            given[k] = a   # (keeps the converted array alive through the call)
            rows.append(a.shape[0])
            ptrs.append(a.ctypes.data_as(L._u64p if dt is np.uint64 else L._f64p))
        if not rows:
            return
        check(lib.ws_geomgrad_add(self.handle, *ptrs, min(rows)))

    def _debug_scratch(self) -> np.ndarray:
        """(N, 5) int64: the scratch sums m0, m1, S00, S01, S11 (tests; syncs)."""
        q = np.empty((self.num_points(), 5), dtype=np.int64)
        check(lib.ws_debug_geomgrad_scratch(self.handle, q.shape[0], q.ctypes.data_as(_i64p)))
        return q

    def _debug_clear_scratch(self, stream=None):
        check(lib.ws_debug_geomgrad_clear_scratch(self.handle, C.c_void_p(stream or 0)))


def geom_spread_rows(q5, rec, xyz, cov, camera_uniform, settings_uniform, geometry_scale=1.0) -> dict:
    """The host twin of the geometry spread (ws_geom_spread_rows, no GPU needed): one frame's (N, 5) int64 scratch sums, the
    (N, 4) uint16 halves 0..3 of each Gaussian's Splat record, the (N, 3) float32 positions, the (N, 6) uint16 covariance halves
    and the frame's two uniforms -> a dict as GeomGrad.download() gives it."""
    q5 = np.ascontiguousarray(q5, dtype=np.int64)
    rec = np.ascontiguousarray(rec, dtype=np.uint16)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    cov = np.ascontiguousarray(cov, dtype=np.uint16)
    n = q5.shape[0]
    if q5.shape != (n, 5) or rec.shape != (n, 4) or xyz.shape != (n, 3) or cov.shape != (n, 6):
        raise ValueError("geom_spread_rows: want (N, 5) sums, (N, 4) record halves, (N, 3) positions and (N, 6) covariance halves")
    out = {k: np.zeros((n,) + shape, dtype=dt) for k, shape, dt in GeomGrad._FIELDS}
    check(lib.ws_geom_spread_rows(q5.ctypes.data_as(_i64p), rec.ctypes.data_as(L._u16p), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                  cov.ctypes.data_as(L._u16p), C.byref(camera_uniform), C.byref(settings_uniform), float(geometry_scale), n,
                                  out["position"].ctypes.data_as(L._f64p), out["covariance"].ctypes.data_as(L._f64p),
                                  out["screen_norm"].ctypes.data_as(L._f64p), out["seen"].ctypes.data_as(L._u64p)))
    return out


def _refit_params(lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999, eps=1e-15, opacity_min=0.0, colour_unit=1.0,
                  opacity_unit=1.0):
    p = L.ws_refit_params()
    p.lr_colour, p.lr_opacity, p.beta1, p.beta2, p.eps, p.opacity_min = lr_colour, lr_opacity, beta1, beta2, eps, opacity_min
    p.colour_unit, p.opacity_unit = colour_unit, opacity_unit
    return p


class Refit:
    """f32 masters and Adam moments of the DC colours and the opacities of one uncompressed resident cloud (websplat.h "Refitting
    colour and opacity"): step() moves the cloud's stored halves in place along a Grad's sums."""

    def __init__(self, ctx: Context, pc: "PointCloud"):
        self.ctx = ctx
        h = C.c_void_p()
        check(lib.ws_refit_create(ctx.handle, pc.handle, C.byref(h)))
        self.handle = h
        self._ncoef = (pc.sh_deg() + 1) ** 2

    def close(self):
        if self.handle:
            lib.ws_refit_destroy(self.handle)
            self.handle = None

    def num_points(self) -> int:
        return lib.ws_refit_num_points(self.handle)

    @property
    def steps(self) -> int:
        """steps taken since creation"""
        return lib.ws_refit_steps(self.handle)

    def step(self, pc: "PointCloud", grad: "Grad", lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999, eps=1e-15, opacity_min=0.0,
             colour_unit=None, opacity_unit=None, scale=1.0, opacity_scale=1.0, stream=None):
        """One Adam step along grad's sums (enqueues only).  A unit left None makes the step one along the MEAN gradient of the
        frames in `grad`, accumulated through `scale` and `opacity_scale` (taken as the float32 values the accumulation used):
        1 / (2^32 * scale [* opacity_scale] * grad.frames)."""
        colour_unit, opacity_unit = self._units("Refit.step", grad, colour_unit, opacity_unit, scale, opacity_scale)
        p = _refit_params(lr_colour, lr_opacity, beta1, beta2, eps, opacity_min, colour_unit, opacity_unit)
        check(lib.ws_refit_step(self.handle, pc.handle, grad.handle, C.byref(p), C.c_void_p(stream or 0)))

    @staticmethod
    def _units(who, grad, colour_unit, opacity_unit, scale, opacity_scale):
        if colour_unit is None or opacity_unit is None:
            per = L.WS_GRAD_SUM_SCALE * float(np.float32(scale))
            frames = grad.frames
            if frames == 0:
                raise ValueError(f"{who}: the accumulator holds no frame: give colour_unit and opacity_unit")
            if colour_unit is None:
                colour_unit = 1.0 / (per * frames)
            if opacity_unit is None:
                opacity_unit = 1.0 / (per * float(np.float32(opacity_scale)) * frames)
        return colour_unit, opacity_unit

    def enable_sh(self, pc: "PointCloud", stream=None):
        """The rest SH coefficients of `pc` join the step: masters and moments of their own (ws_refit_enable_sh; enqueues
        only).  Before the first step; a second call is a no-op."""
        check(lib.ws_refit_enable_sh(self.handle, pc.handle, C.c_void_p(stream or 0)))

    def step_sh(self, pc: "PointCloud", shgrad: "ShGrad", lr_sh=None, lr_colour=0.0025, lr_opacity=0.01, beta1=0.9, beta2=0.999,
                eps=1e-15, opacity_min=0.0, colour_unit=None, opacity_unit=None, scale=1.0, opacity_scale=1.0, stream=None):
        """One Adam step along an ShGrad's sums (ws_refit_step_sh; enqueues only): the DC triple and the opacity as step() moves
        them, the rest coefficients at the rate lr_sh (None: lr_colour / 20, the 3DGS convention; 0 freezes them).  Units as
        step()."""
        colour_unit, opacity_unit = self._units("Refit.step_sh", shgrad, colour_unit, opacity_unit, scale, opacity_scale)
        p = L.ws_refit_sh_params()
        p.base = _refit_params(lr_colour, lr_opacity, beta1, beta2, eps, opacity_min, colour_unit, opacity_unit)
        p.lr_sh = p.base.lr_colour / 20.0 if lr_sh is None else lr_sh   # (of the float32 rate, as refit_scene takes it)
        check(lib.ws_refit_step_sh(self.handle, pc.handle, shgrad.handle, C.byref(p), C.c_void_p(stream or 0)))

    def download_sh(self) -> dict:
        """{"master", "m", "v"}: (N, ncoef - 1, 3) float32 each -- the rest coefficients and their moments (syncs)."""
        n, rest = self.num_points(), self._ncoef - 1
        out = {k: np.empty((n, rest, 3), dtype=np.float32) for k in ("master", "m", "v")}
        check(lib.ws_refit_download_sh(self.handle, n, *(out[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ("master", "m", "v"))))
        return out

    def download(self) -> dict:
        """{"master", "m", "v"}: (N, 4) float32 each -- DC r, g, b and the opacity; their first and second moments (syncs)."""
        n = self.num_points()
        out = {k: np.empty((n, L.WS_GRAD_CHANNELS), dtype=np.float32) for k in ("master", "m", "v")}
        check(lib.ws_refit_download(self.handle, n, *(out[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ("master", "m", "v"))))
        return out


def accumulate_contrib_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, contrib: "Contrib") -> int:
    """Every camera of `split`, set up as render_views sets its frames up, added to `contrib`; returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_contrib(ctx.handle, pc.handle, scene.handle, _SPLITS[split], contrib.handle, C.byref(n)))
    return n.value


@dataclass
class ImageView:
    """One image as the metrics see it (ws_image_view): device pointer, format name ("rgba8unorm" / "rgba16float" / "rgba32float"),
    row pitch in bytes, and the background colour the premultiplied texels go over (None: the colour channels as stored)."""
    ptr: int
    format: str
    pitch: int
    background: Optional[Sequence[float]] = None

    def to_c(self):
        v = L.ws_image_view()
        v.d_pixels = self.ptr
        v.format = FORMATS[self.format][0]
        v.row_pitch_bytes = int(self.pitch)
        v.over_background = 0 if self.background is None else 1
        if self.background is not None:
            v.background[:] = [float(x) for x in self.background[:3]]
        return v


def _as_view(v) -> ImageView:
    return v if isinstance(v, ImageView) else ImageView(*v)


class Metrics:
    """PSNR / SSIM records of up to max_images image pairs, computed on the device (websplat.h "Image metrics").  One
    accumulator is used from one stream at a time."""

    def __init__(self, ctx: Context, max_images: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(lib.ws_metrics_create(ctx.handle, int(max_images), C.byref(h)))
        self.handle = h
        self.max_images = int(max_images)
        self._maps = []  # DeviceArray (H x W float32) of the adds that asked for the SSIM map, in add order

    def _drop_maps(self):
        while self._maps:
            self._maps.pop().free()

    def close(self):
        if self.handle:
            lib.ws_metrics_destroy(self.handle)  # (waits for the device)
            self.handle = None
            self._drop_maps()

    def reset(self, stream=None):
        check(lib.ws_metrics_reset(self.handle, C.c_void_p(stream or 0)))
        self.ctx.sync(stream)
        self._drop_maps()

    @property
    def count(self) -> int:
        """image pairs added since creation / the last reset"""
        return lib.ws_metrics_count(self.handle)

    def add(self, a, b, width: int, height: int, quantize_u8=False, ssim_map=False, stream=None):
        """Enqueue the comparison of views a and b (ImageView, or (ptr, format, pitch, background-or-None) tuples).  ssim_map:
        also keep the W x H map, returned by maps()."""
        va, vb = _as_view(a).to_c(), _as_view(b).to_c()
        m = DeviceArray(self.ctx, (height, width), np.float32) if ssim_map else None
        try:
            check(lib.ws_metrics_add(self.handle, C.byref(va), C.byref(vb), int(width), int(height),
                                     L.WS_METRICS_QUANTIZE_U8 if quantize_u8 else 0, C.c_void_p(m.ptr if m else 0),
                                     m.pitch if m else 0, C.c_void_p(stream or 0)))
        except Exception:
            if m:
                m.free()
            raise
        if m:
            self._maps.append(m)

    def download(self):
        """One dict per image pair, in add order: mse, psnr, ssim, sse_u8, width, height, flags (syncs)."""
        n = self.count
        buf = (L.ws_image_metrics * max(n, 1))()
        got = C.c_uint32()
        check(lib.ws_metrics_download(self.handle, n, buf, C.byref(got)))
        return [{k: getattr(buf[i], k) for k in ("mse", "psnr", "ssim", "sse_u8", "width", "height", "flags")} for i in range(got.value)]

    def maps(self):
        """The SSIM maps (H x W float32) of the adds that asked for one, in add order (call after download(), which syncs)."""
        return [m.download() for m in self._maps]


_NP_FORMATS = {np.dtype(np.uint8): "rgba8unorm", np.dtype(np.float16): "rgba16float", np.dtype(np.float32): "rgba32float"}


def _upload_pair(ctx: Context, who: str, img_a, img_b, background_a, background_b):
    """(the two images as DeviceArrays, their ImageViews, w, h) of `who`'s two H x W x 4 numpy images; the caller frees the
    arrays once the device is done with them."""
    imgs = [np.ascontiguousarray(im) for im in (img_a, img_b)]
    for im in imgs:
        if im.ndim != 3 or im.shape[2] != 4 or im.dtype not in _NP_FORMATS or im.shape != imgs[0].shape:
            raise ValueError(f"{who}: two H x W x 4 arrays of one size, uint8 / float16 / float32")
    arrays = []
    try:
        for im in imgs:
            arrays.append(DeviceArray.from_host(ctx, im))
    except Exception:
        for a in arrays:
            a.free()
        raise
    views = [ImageView(a.ptr, _NP_FORMATS[a.dtype], a.pitch, bg) for a, bg in zip(arrays, (background_a, background_b))]
    h, w = imgs[0].shape[:2]
    return arrays, views, w, h


def image_metrics(ctx: Context, img_a: np.ndarray, img_b: np.ndarray, background_a=None, background_b=None, quantize_u8=False,
                  ssim_map=False):
    """PSNR / SSIM of two H x W x 4 numpy images (uint8, float16 or float32, each its own format): upload, add, download.
    Returns the record's dict, or (dict, H x W float32 map) with ssim_map."""
    arrays, views, w, h = _upload_pair(ctx, "image_metrics", img_a, img_b, background_a, background_b)
    m = None
    try:
        m = Metrics(ctx, 1)
        m.add(views[0], views[1], w, h, quantize_u8=quantize_u8, ssim_map=ssim_map)
        rec = m.download()[0]
        return (rec, m.maps()[0]) if ssim_map else rec
    finally:
        if m:
            m.close()
        for a in arrays:
            a.free()


def read_png(path: str) -> np.ndarray:
    """An 8-bit grey / grey + alpha / RGB / RGBA PNG as H x W x 4 uint8 (ws_png_read_rgba8)."""
    w, h = C.c_uint32(), C.c_uint32()
    p = C.POINTER(C.c_uint8)()
    check(lib.ws_png_read_rgba8(str(path).encode(), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
    finally:
        lib.ws_host_free(p)


def evaluate_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, metrics: "Metrics", ref: "PointCloud" = None,
                   gt_dir: str = None, quantize_u8=False) -> int:
    """Every camera of `split` adds one record to `metrics`: `pc` against the cloud `ref` (set up as render_views sets its
    frames up) or against the PNGs <gt_dir>/<img_name>[.png], rendered at each PNG's size.  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_evaluate(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
                                None if gt_dir is None else str(gt_dir).encode(), L.WS_METRICS_QUANTIZE_U8 if quantize_u8 else 0,
                                metrics.handle, C.byref(n)))
    return n.value


ERROR_KINDS = {"sq": L.WS_ERROR_SQ, "abs": L.WS_ERROR_ABS, "dssim": L.WS_ERROR_DSSIM}


def image_error_plane(ctx: Context, img_a: np.ndarray, img_b: np.ndarray, kind="sq", quantize_u8=False, background_a=None,
                      background_b=None) -> np.ndarray:
    """The per-pixel error plane (H x W float32) of two H x W x 4 numpy images (uint8, float16 or float32, each its own format):
    the mean over the colour channels of d * d ("sq") or |d| ("abs") on the pixel values of image_metrics
    (ws_image_error_plane): upload, one launch, download."""
    arrays, views, w, h = _upload_pair(ctx, "image_error_plane", img_a, img_b, background_a, background_b)
    try:
        va, vb = views[0].to_c(), views[1].to_c()
        out = DeviceArray(ctx, (h, w), np.float32)
        arrays.append(out)
        check(lib.ws_image_error_plane(ctx.handle, C.byref(va), C.byref(vb), w, h, ERROR_KINDS[kind],
                                       L.WS_METRICS_QUANTIZE_U8 if quantize_u8 else 0, C.c_void_p(out.ptr), out.pitch, None))
        return out.download()
    finally:
        ctx.sync()
        for a in arrays:
            a.free()


def image_error_gradient(ctx: Context, img_a: np.ndarray, img_b: np.ndarray, kind="sq", background_a=None, background_b=None) -> np.ndarray:
    """The derivative of image_error_plane's value with respect to image a's pixel values (H x W x 4 float32, the fourth
    component 0; ws_image_error_gradient) of two H x W x 4 numpy images: upload, one launch, download."""
    arrays, views, w, h = _upload_pair(ctx, "image_error_gradient", img_a, img_b, background_a, background_b)
    try:
        va, vb = views[0].to_c(), views[1].to_c()
        out = DeviceArray(ctx, (h, w, 4), np.float32)
        arrays.append(out)
        check(lib.ws_image_error_gradient(ctx.handle, C.byref(va), C.byref(vb), w, h, ERROR_KINDS[kind], 0,
                                          C.c_void_p(out.ptr), out.pitch, None))
        return out.download()
    finally:
        ctx.sync()
        for a in arrays:
            a.free()


def accumulate_gradient_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, grad: "Grad", ref: "PointCloud" = None,
                              gt_dir: str = None, kind="sq", scale=1.0, opacity_scale=1.0) -> int:
    """Every camera of `split`, set up as accumulate_error_scene sets it up: the colour and ln-opacity gradients of the frames'
    error ("sq" or "abs") against the cloud `ref` or the PNGs of `gt_dir`, per Gaussian of `pc`, into `grad`
    (ws_scene_accumulate_gradient).  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_gradient(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
                                           None if gt_dir is None else str(gt_dir).encode(), ERROR_KINDS[kind], float(scale),
                                           float(opacity_scale), grad.handle, C.byref(n)))
    return n.value


def accumulate_sh_gradient_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, shgrad: "ShGrad", ref: "PointCloud" = None,
                                 gt_dir: str = None, kind="sq", scale=1.0, opacity_scale=1.0) -> int:
    """accumulate_gradient_scene's frames into an ShGrad: per Gaussian the gradients with respect to every SH coefficient and
    the ln-opacity (ws_scene_accumulate_sh_gradient).  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_sh_gradient(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
                                              None if gt_dir is None else str(gt_dir).encode(), ERROR_KINDS[kind], float(scale),
                                              float(opacity_scale), shgrad.handle, C.byref(n)))
    return n.value


def accumulate_geometry_gradient_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, geomgrad: "GeomGrad",
                                       ref: "PointCloud" = None, gt_dir: str = None, kind="sq", scale=1.0, geometry_scale=1.0) -> int:
    """accumulate_gradient_scene's frames into a GeomGrad: per Gaussian the gradients with respect to position and covariance and
    the densification statistic (ws_scene_accumulate_geometry_gradient).  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_geometry_gradient(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
                                                    None if gt_dir is None else str(gt_dir).encode(), ERROR_KINDS[kind], float(scale),
                                                    float(geometry_scale), geomgrad.handle, C.byref(n)))
    return n.value


def refit_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, refit: "Refit", ref: "PointCloud" = None, gt_dir: str = None,
                kind="sq", opacity_scale=1.0 / 128, epochs=1, views_per_step=0, sh=False, lr_sh=None, **adam) -> int:
    """`epochs` passes over the cameras of `split`, set up as accumulate_gradient_scene sets them up: the gradients of the frames'
    error against the cloud `ref` or the PNGs of `gt_dir`, and an Adam step of `refit` on `pc` after every `views_per_step` frames
    (0 = one step per epoch) along their mean (ws_scene_refit).  **adam: Refit.step's rates, betas, eps and opacity_min.
    sh=True: the rest SH coefficients move too, at the rate lr_sh (None: lr_colour / 20) -- ws_scene_refit_sh, which enables them
    on `refit` if that has not been done.  Returns the steps taken."""
    p = _refit_params(**adam)
    n = C.c_uint32()
    tail = (int(epochs), int(views_per_step), C.byref(n))
    head = (ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
            None if gt_dir is None else str(gt_dir).encode(), ERROR_KINDS[kind], float(opacity_scale), refit.handle)
    if sh:
        sp = L.ws_refit_sh_params()
        sp.base = p
        sp.lr_sh = p.lr_colour / 20.0 if lr_sh is None else lr_sh
        check(lib.ws_scene_refit_sh(*head, C.byref(sp), *tail))
    else:
        if lr_sh is not None:
            raise ValueError("refit_scene: lr_sh needs sh=True")
        check(lib.ws_scene_refit(*head, C.byref(p), *tail))
    return n.value


def accumulate_error_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, err: "Contrib", weight: "Contrib" = None,
                           ref: "PointCloud" = None, gt_dir: str = None, kind="sq", quantize_u8=False) -> int:
    """Every camera of `split`, set up as evaluate_scene sets it up: the per-pixel error of `pc` against the cloud `ref` or the
    PNGs of `gt_dir` ("sq", "abs" or "dssim"), attributed to the Gaussians of `pc` into `err`; `weight` (optional) receives the
    plain contribution sums of the same frames, so err / weight is the mean error under a Gaussian.  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_error(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ref.handle if ref is not None else None,
                                        None if gt_dir is None else str(gt_dir).encode(), ERROR_KINDS[kind],
                                        L.WS_METRICS_QUANTIZE_U8 if quantize_u8 else 0, err.handle,
                                        weight.handle if weight is not None else None, C.byref(n)))
    return n.value


def accumulate_removal_scene(ctx: "Context", pc: "PointCloud", scene: Scene, split: str, effect: "Contrib", weight: "Contrib" = None,
                             kind="sq", scale=1.0) -> int:
    """Every camera of `split`, set up as accumulate_contrib_scene sets it up: what deleting each Gaussian of `pc` alone would do
    to the frames ("sq" or "abs", ws_scene_accumulate_removal), over the cloud's own background colour or black, into `effect`;
    `weight` (optional) receives the plain contribution sums of the same frames.  Returns the frames added."""
    n = C.c_uint32()
    check(lib.ws_scene_accumulate_removal(ctx.handle, pc.handle, scene.handle, _SPLITS[split], ERROR_KINDS[kind], float(scale),
                                          effect.handle, weight.handle if weight is not None else None, C.byref(n)))
    return n.value


class GaussianRenderer:
    """renderer.rs:33-283.  `prepare` + `render` enqueue on a HIP stream; nothing syncs except the
    read-back helpers (num_visible_points, frame_stats, stage_times, download_*)."""

    def __init__(self, ctx: Context, color_format: str = "rgba32float", sh_deg: int = 3, compressed: bool = False):
        h = C.c_void_p()
        check(lib.ws_renderer_create(ctx.handle, FORMATS[color_format][0], int(sh_deg), int(compressed), C.byref(h)))
        self._set_state(ctx, h, color_format, owns_handle=True)

    @classmethod
    def _view(cls, ctx: Context, handle, color_format: str):
        """A renderer object on a handle somebody else owns (ViewBatch.renderer): close() frees its planes, not the handle."""
        r = cls.__new__(cls)
        r._set_state(ctx, handle, color_format, owns_handle=False)
        return r

    def _set_state(self, ctx, handle, color_format, owns_handle):
        self.ctx = ctx
        self.handle = handle
        self._owns_handle = owns_handle
        self.color_format_name = color_format
        _, self.np_dtype, self.texel_bytes = FORMATS[color_format]
        self._viewport = (0, 0)   # of the last prepare(); (0, 0): not prepared -- the library says so
        # renderer-owned planes, one set per group: each is let go when ITS next use sees another viewport
        self._target = ViewportPlanes(ctx)    # "target": H x W x 4 of the colour format
        self._aux = ViewportPlanes(ctx)       # plane name -> H x W f32 of render_aux / render_composite
        self._aux_last = ()                   # the planes the last render_aux wrote
        self._val = ViewportPlanes(ctx)       # 0..3 -> H x W f32, "winner" -> H x W u32 of render_values
        self._val_last = (0, False)           # (channels, winner) the last render_values wrote
        self._base = ViewportPlanes(ctx)      # "base": H x W float4 of accumulate_removal / _gradient(base=True)
        self._occluder = ViewportPlanes(ctx)  # "occluder": H x W f32 copy of render_composite's numpy occluder

    def close(self):
        for planes in (self._aux, self._val, self._base, self._occluder, self._target):
            planes.free()
        if self.handle and self._owns_handle:
            lib.ws_renderer_destroy(self.handle)
        self.handle = None

    def color_format(self):
        return self.color_format_name

    def enable_timers(self, on=True):
        """0/False = off, 1/True = stage times, 2 = additionally per-kernel times."""
        check(lib.ws_renderer_enable_timers(self.handle, int(on)))

    def kernel_times(self):
        """[(label, ms)] of every kernel launch of the last frame, launch order (needs enable_timers(2))."""
        n = C.c_uint32()
        buf = (L.ws_kernel_time * 64)()
        check(lib.ws_renderer_kernel_times(self.handle, 64, buf, C.byref(n)))
        return [(buf[i].name.decode(), buf[i].ms) for i in range(min(n.value, 64))]

    def tile_lists(self):
        """(begin[T], end[T], entries[D]): tile t's far -> near splat list is entries[begin[t]:end[t]] (store indices)."""
        nt = C.c_uint32()
        check(lib.ws_renderer_download_tile_stats(self.handle, 0, None, None, C.byref(nt)))
        d = C.c_uint32()
        check(lib.ws_renderer_download_tile_lists(self.handle, 0, None, None, 0, None, C.byref(d)))
        begin = np.empty(nt.value, dtype=np.uint32)
        end = np.empty(nt.value, dtype=np.uint32)
        entries = np.empty(max(d.value, 1), dtype=np.uint32)
        check(lib.ws_renderer_download_tile_lists(self.handle, nt.value, begin.ctypes.data_as(C.c_void_p),
                                                  end.ctypes.data_as(C.c_void_p), entries.size,
                                                  entries.ctypes.data_as(C.c_void_p), C.byref(d)))
        return begin, end, entries[:d.value]

    def wave_stats(self):
        """[tiles, 17] uint32 (capture mode): records composited per wave; column 16 = lock-step cost (see websplat.h)."""
        nt = C.c_uint32()
        check(lib.ws_renderer_download_tile_stats(self.handle, 0, None, None, C.byref(nt)))
        out = np.zeros((nt.value, 17), dtype=np.uint32)
        check(lib.ws_renderer_download_wave_stats(self.handle, nt.value, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def depth_sort_passes(self) -> int:
        """digit passes the last prepared frame's depth sort executed (websplat.h)."""
        v = C.c_uint32()
        check(lib.ws_renderer_depth_sort_passes(self.handle, C.byref(v)))
        return v.value

    def enable_frame_trace(self, frames: int):
        """K1 and the blend of the next `frames` frames leave (start, end) on the device clock (websplat.h)."""
        check(lib.ws_renderer_enable_frame_trace(self.handle, int(frames)))

    def frame_trace(self):
        """[frames, 4] uint64 ticks of the 100-MHz device clock: K1 start, K1 end, blend start, blend end (syncs)."""
        n = C.c_uint32()
        check(lib.ws_renderer_download_frame_trace(self.handle, 0, None, C.byref(n)))
        out = np.zeros((n.value, 4), dtype=np.uint64)
        if n.value:
            check(lib.ws_renderer_download_frame_trace(self.handle, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def depth_sort_digit_bits(self) -> int:
        """digit width (8 | 9) of the last prepared frame's depth sort (websplat.h)."""
        v = C.c_uint32()
        check(lib.ws_renderer_depth_sort_digit_bits(self.handle, C.byref(v)))
        return v.value

    def blend_order(self):
        """[blocks, 4] uint32 (tx | ty << 16, begin, end, 0): the compositing workgroups' tiles, longest list first; empty when
        the last prepared frame was not ordered (websplat.h)."""
        nb = C.c_uint32()
        check(lib.ws_renderer_download_blend_order(self.handle, 0, None, C.byref(nb)))
        out = np.zeros((nb.value, 4), dtype=np.uint32)
        if nb.value:
            check(lib.ws_renderer_download_blend_order(self.handle, nb.value, out.ctypes.data_as(C.c_void_p), C.byref(nb)))
        return out

    def enable_blend_timing(self, on=True):
        check(lib.ws_renderer_enable_blend_timing(self.handle, 1 if on else 0))

    def blend_timing(self):
        """[tiles, 16 waves, 16 words] uint32 of the last render() under enable_blend_timing (layout: websplat.h)."""
        nt = C.c_uint32()
        check(lib.ws_renderer_download_blend_timing(self.handle, 0, None, C.byref(nt)))
        out = np.zeros((nt.value, 16, 16), dtype=np.uint32)
        check(lib.ws_renderer_download_blend_timing(self.handle, nt.value, out.ctypes.data_as(C.c_void_p), None))
        return out

    def tile_stats(self, with_consumed=False):
        nt = C.c_uint32()
        check(lib.ws_renderer_download_tile_stats(self.handle, 0, None, None, C.byref(nt)))
        ll = np.empty(nt.value, dtype=np.uint32)
        cons = np.empty(nt.value, dtype=np.uint32) if with_consumed else None
        check(lib.ws_renderer_download_tile_stats(
            self.handle, nt.value, ll.ctypes.data_as(C.c_void_p),
            cons.ctypes.data_as(C.c_void_p) if cons is not None else None, C.byref(nt)))
        return {"list_len": ll, "consumed": cons}

    def enable_capture(self, on=True):
        check(lib.ws_renderer_enable_capture(self.handle, int(on)))

    def binning_tile(self):
        """(width, height) in pixels of the binning tile the last prepared frame used (the device decides per frame)."""
        w, h = C.c_uint32(), C.c_uint32()
        check(lib.ws_renderer_binning_tile(self.handle, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_blend_mode(self, mode="fast"):
        """"fast" (front to back, early-out, one rounding at the store) or "target" (the reference's fixed-function blend
        literally: back to front, the destination rounded to the target's precision after every splat)."""
        check(lib.ws_renderer_set_blend_mode(self.handle, {"fast": 0, "target": 1, "fast_exact_cut": 2}[mode]))

    def set_tile_entry_capacity(self, entries: int):
        check(lib.ws_renderer_set_tile_entry_capacity(self.handle, int(entries)))

    def prepare(self, pc: PointCloud, args: SplattingArgs, stream=None):
        a = args.to_c()
        check(lib.ws_renderer_prepare(self.handle, pc.handle, C.byref(a), C.c_void_p(stream or 0)))
        self._viewport = (int(args.viewport[0]), int(args.viewport[1]))

    def render(self, pc: PointCloud, target_ptr: int = None, pitch: int = None, background=(0.0, 0.0, 0.0, 0.0),
               stream=None):
        if target_ptr is None:
            target_ptr = self._own_target().ptr
        if pitch is None:
            pitch = self._viewport[0] * self.texel_bytes
        bg = (C.c_float * 4)(*[float(x) for x in background])
        check(lib.ws_renderer_render(self.handle, pc.handle, bg, C.c_void_p(target_ptr), pitch, C.c_void_p(stream or 0)))
        return target_ptr

    def _own_target(self) -> DeviceArray:
        """The renderer-owned target (H x W x 4 of the colour format) of the prepared viewport."""
        self._target.fit(*self._viewport)
        return self._target.plane("target", self.np_dtype, 4)

    def enable_depth(self, on=True):
        """K1 also writes each visible splat's view-space depth (4 B per splat) from the next prepare() on: what the depth and
        median_depth planes of render_aux() are built from."""
        check(lib.ws_renderer_enable_depth(self.handle, int(bool(on))))

    def enable_contrib(self, on=True):
        """K1 also keeps each visible splat's index into the point cloud (4 B per splat) from the next prepare() on: what
        accumulate_contrib() attributes the frame's weights through.  Changes no pixel."""
        check(lib.ws_renderer_enable_contrib(self.handle, int(bool(on))))

    def accumulate_contrib(self, pc: PointCloud, contrib: "Contrib", stream=None):
        """Add the prepared frame's per-Gaussian weights to `contrib` (enqueues; render() is not needed)."""
        check(lib.ws_renderer_accumulate_contrib(self.handle, pc.handle, contrib.handle, C.c_void_p(stream or 0)))

    def _plane_view(self, who, what, plane, pitch, scale, bias, view):
        """(ws_plane_view, array to stage | None) of an H x W float32 numpy plane of the viewport `view` -- its d_values is
        the caller's to set from staged() -- or of a device pointer with its row `pitch` in bytes."""
        v = L.ws_plane_view()
        v.scale, v.bias = float(scale), float(bias)
        if not isinstance(plane, np.ndarray):
            if pitch is None:
                raise ValueError(f"{who}: a device {what} needs its row pitch")
            v.d_values, v.row_pitch_bytes = int(plane), int(pitch)
            return v, None
        a = np.ascontiguousarray(plane, dtype=np.float32)
        if a.ndim != 2 or (view is not None and view[0] and (a.shape[0] != view[1] or a.shape[1] < view[0])):  # (wider rows: padding)
            raise ValueError(f"{who}: want an H x W float32 {what} of the viewport {view}, got {a.shape}")
        v.row_pitch_bytes = int(pitch) if pitch is not None else a.shape[1] * 4
        return v, a

    def accumulate_weighted(self, pc: PointCloud, contrib: "Contrib", plane, scale=1.0, bias=0.0, pitch=None, stream=None):
        """Add the prepared frame's per-Gaussian weights times E(p) = clamp(scale * plane[p] + bias, 0, 1) to `contrib`
        (ws_renderer_accumulate_weighted).  `plane`: an H x W float32 numpy array of the viewport's shape (uploaded for the
        call, which then waits for the launch), or a device pointer with its row `pitch` in bytes (enqueues only)."""
        v, host = self._plane_view("accumulate_weighted", "plane", plane, pitch, scale, bias, self._viewport)
        with staged(self.ctx, host, stream) as d:
            if d is not None:
                v.d_values = d
            check(lib.ws_renderer_accumulate_weighted(self.handle, pc.handle, contrib.handle, C.byref(v), C.c_void_p(stream or 0)))

    def _set_base(self, p, base, base_ptr, base_pitch):
        """d_base / base_pitch_bytes of a ws_removal_params or ws_gradient_params: the caller's device plane, the
        renderer-owned H x W float4 plane of the prepared viewport (base=True), or none."""
        w, h = self._viewport
        if base_ptr is not None:
            p.d_base, p.base_pitch_bytes = int(base_ptr), int(base_pitch if base_pitch is not None else w * 16)
        elif base:
            self._base.fit(w, h)
            own = self._base.plane("base", np.float32, 4)
            p.d_base, p.base_pitch_bytes = own.ptr, own.pitch

    def accumulate_removal(self, pc: PointCloud, contrib: "Contrib", background=(0.0, 0.0, 0.0), kind="sq", scale=1.0, weight=None,
                           weight_scale=1.0, weight_bias=0.0, base=False, stream=None, weight_pitch=None, base_ptr=None,
                           base_pitch=None):
        """Add to `contrib`, per Gaussian, what deleting it alone would do to the prepared frame over `background`
        (ws_renderer_accumulate_removal): the sum over its pairs of min(scale * mean_ch e(D), 1 - 2^-24), e = D * D ("sq") or |D|
        ("abs"), D the change of the pixel.  Needs enable_contrib() before prepare(); render() is not needed, no target changes.

        `weight`: None, an H x W float32 numpy plane (uploaded for the call, which then waits for the launches) or a device
        pointer with `weight_pitch` bytes per row; every pair counts times E(p) = clamp(weight_scale * weight[p] + weight_bias, 0, 1).
        base=True: the frame's f32 image over `background` and the final transmittance go to a renderer-owned H x W float4
        buffer that download_removal_base() reads back; `base_ptr` / `base_pitch`: a caller's device plane instead."""
        p = L.ws_removal_params()
        for i in range(3):
            p.background[i] = float(background[i])
        p.kind = ERROR_KINDS[kind] if isinstance(kind, str) else int(kind)
        p.scale = float(scale)
        self._set_base(p, base, base_ptr, base_pitch)
        v, host = None, None
        if weight is not None:
            v, host = self._plane_view("accumulate_removal", "weight plane", weight, weight_pitch, weight_scale, weight_bias,
                                       self._viewport)
            p.weight = C.pointer(v)
        with staged(self.ctx, host, stream) as d:
            if d is not None:
                v.d_values = d
            check(lib.ws_renderer_accumulate_removal(self.handle, pc.handle, contrib.handle, C.byref(p), C.c_void_p(stream or 0)))

    def accumulate_gradient(self, pc: PointCloud, grad: "Grad", plane, background=(0.0, 0.0, 0.0), scale=1.0, opacity_scale=1.0,
                            base=False, stream=None, plane_pitch=None, base_ptr=None, base_pitch=None):
        """Add to `grad`, per Gaussian, the gradients of an image loss over the prepared frame (ws_renderer_accumulate_gradient):
        colour[ch] += sum of w * G_ch, opacity += -sum of (G . D + G_T r T_end), G = clamp(scale * plane, -1, 1).  `plane`: the
        loss's derivative (dL/dF_r, dL/dF_g, dL/dF_b, dL/dT_end) per pixel, an H x W x 4 float32 numpy array (uploaded for the
        call, which then waits for the launches) or a device pointer with `plane_pitch` bytes per row.  Needs enable_contrib()
        before prepare(); render() is not needed, no target changes.  base / base_ptr / base_pitch: as accumulate_removal."""
        self._accumulate_gradient(lib.ws_renderer_accumulate_gradient, pc, grad, plane, background, scale, opacity_scale, base, stream,
                                  plane_pitch, base_ptr, base_pitch)

    def accumulate_sh_gradient(self, pc: PointCloud, shgrad: "ShGrad", plane, background=(0.0, 0.0, 0.0), scale=1.0, opacity_scale=1.0,
                               base=False, stream=None, plane_pitch=None, base_ptr=None, base_pitch=None):
        """accumulate_gradient into an ShGrad (ws_renderer_accumulate_sh_gradient): the same two launches into the accumulator's
        scratch, then per Gaussian the colour sums times the SH basis of this frame's view direction, added to every coefficient
        up to the prepared frame's degree.  Arguments as accumulate_gradient."""
        self._accumulate_gradient(lib.ws_renderer_accumulate_sh_gradient, pc, shgrad, plane, background, scale, opacity_scale, base,
                                  stream, plane_pitch, base_ptr, base_pitch)

    def accumulate_geometry_gradient(self, pc: PointCloud, geomgrad: "GeomGrad", plane, background=(0.0, 0.0, 0.0), scale=1.0,
                                     geometry_scale=1.0, base=False, stream=None, plane_pitch=None, base_ptr=None, base_pitch=None,
                                     _stage_a_only=False):
        """Add to `geomgrad`, per Gaussian, dL/d(position), dL/d(covariance) and the norm of the screen-space positional gradient
        of an image loss over the prepared frame (ws_renderer_accumulate_geometry_gradient).  `plane` and the other arguments as
        accumulate_gradient; geometry_scale scales the five screen-space sums before they are made fixed-point (finite, > 0)."""
        call = lib.ws_debug_geometry_stage_a if _stage_a_only else lib.ws_renderer_accumulate_geometry_gradient
        self._accumulate_gradient(call, pc, geomgrad, plane, background, scale, geometry_scale, base, stream, plane_pitch, base_ptr,
                                  base_pitch, params=L.ws_geometry_params)

    def _accumulate_gradient(self, call, pc, grad, plane, background, scale, opacity_scale, base, stream, plane_pitch, base_ptr,
                             base_pitch, params=L.ws_gradient_params):
        p = params()
        for i in range(3):
            p.background[i] = float(background[i])
        p.scale = float(scale)
        setattr(p, "geometry_scale" if params is L.ws_geometry_params else "opacity_scale", float(opacity_scale))
        w, h = self._viewport
        self._set_base(p, base, base_ptr, base_pitch)
        host = None
        if isinstance(plane, np.ndarray):
            a = np.ascontiguousarray(plane, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 4 or (w and (a.shape[0] != h or a.shape[1] < w)):  # (wider rows: padding)
                raise ValueError(f"accumulate_gradient: want an H x W x 4 float32 plane of the viewport {(w, h)}, got {a.shape}")
            p.grad_pitch_bytes = int(plane_pitch) if plane_pitch is not None else a.shape[1] * 16
            host = a
        else:
            if plane is not None and plane_pitch is None:
                raise ValueError("accumulate_gradient: a device plane needs its row pitch")
            p.d_grad, p.grad_pitch_bytes = (int(plane) if plane is not None else None), int(plane_pitch or 0)
        with staged(self.ctx, host, stream, min_bytes=16) as d:
            if d is not None:
                p.d_grad = d
            check(call(self.handle, pc.handle, grad.handle, C.byref(p), C.c_void_p(stream or 0)))

    def download_removal_base(self) -> np.ndarray:
        """H x W x 4 float32 (F_r, F_g, F_b, T_end) of what the last accumulate_removal(base=True) or accumulate_gradient(base=True) wrote (syncs)."""
        base = self._base.get("base")
        if base is None:
            raise ValueError("download_removal_base: no accumulate_removal(base=True) since the viewport changed")
        self.ctx.sync()
        return base.download()

    def render_values(self, pc: PointCloud, values=None, winner=False, stream=None, stride=None, channels=None):
        """Draw per-Gaussian values through the prepared frame's weights (ws_renderer_render_values): per pixel and channel the sum
        over the kept pairs of w * values[j][c], and with winner=True the index of the Gaussian with the largest w at the pixel
        (0xFFFFFFFF: none).  Needs enable_contrib() before prepare(); render() is not needed and no target changes.

        `values`: an (N,) or (N, C) float32 numpy array, C <= 4, over the cloud's Gaussians (uploaded for the call, which then
        waits for the launch); or a device pointer with `stride` bytes per Gaussian and `channels` (enqueues only); or None with
        winner=True.  The planes go to renderer-owned H x W buffers: download_values() reads them back."""
        if self._val.viewport != self._viewport:
            self._val_last = (0, False)  # (the planes it names are let go)
        self._val.fit(*self._viewport)
        v, host = None, None
        if isinstance(values, np.ndarray):
            a = np.ascontiguousarray(values, dtype=np.float32)
            if a.ndim == 1:
                a = a[:, None]
            if a.ndim != 2 or not 1 <= a.shape[1] <= 4:
                raise ValueError(f"render_values: want (N,) or (N, C <= 4) float32 values, got {values.shape}")
            v = L.ws_values_view()
            v.stride_bytes, v.num_points, v.channels = a.shape[1] * 4, a.shape[0], a.shape[1]
            host = a
        elif values is not None:
            if stride is None or channels is None:
                raise ValueError("render_values: device values need their stride in bytes and their number of channels")
            v = L.ws_values_view()
            v.d_values, v.stride_bytes, v.num_points, v.channels = int(values), int(stride), pc.num_points(), int(channels)
        nch = int(v.channels) if v is not None else 0
        t = L.ws_value_targets()
        for c in range(min(nch, 4)):
            own = self._val.plane(c, np.float32)
            t.plane[c], t.pitch[c] = own.ptr, own.pitch
        if winner:
            own = self._val.plane("winner", np.uint32)
            t.winner, t.winner_pitch = own.ptr, own.pitch
        vref = C.byref(v) if v is not None else None
        with staged(self.ctx, host, stream) as d:
            if d is not None:
                v.d_values = d
            check(lib.ws_renderer_render_values(self.handle, pc.handle, vref, C.byref(t), C.c_void_p(stream or 0)))
        self._val_last = (nch, bool(winner))

    def download_values(self) -> dict:
        """{"values": H x W x C float32, "winner": H x W uint32} of what the last render_values() wrote (syncs); a key is
        absent when the call did not ask for it."""
        nch, winner = self._val_last
        self.ctx.sync()
        out = {}
        if nch:
            out["values"] = np.stack([self._val.get(c).download() for c in range(nch)], axis=-1)
        if winner:
            out["winner"] = self._val.get("winner").download()
        return out

    def _aux_targets(self, depth, median_depth, alpha):
        """(ws_aux_targets, names) of the asked-for planes among the renderer-owned H x W f32 ones of the prepared viewport."""
        self._aux.fit(*self._viewport)
        want = tuple(name for name, on in (("depth", depth), ("median_depth", median_depth), ("alpha", alpha)) if on)
        t = L.ws_aux_targets()
        for name in want:
            own = self._aux.plane(name, np.float32)
            setattr(t, name, C.c_void_p(own.ptr))
            setattr(t, name + "_pitch", own.pitch)
        return t, want

    def render_aux(self, pc: PointCloud, depth=True, median_depth=False, alpha=False, background=(0.0, 0.0, 0.0, 0.0),
                   stream=None):
        """render() into the renderer-owned target plus the asked-for auxiliary planes (websplat.h ws_renderer_render_aux) into
        renderer-owned H x W float32 buffers; download_aux() reads them back."""
        target = self._own_target()
        t, want = self._aux_targets(depth, median_depth, alpha)
        bg = (C.c_float * 4)(*[float(x) for x in background])
        check(lib.ws_renderer_render_aux(self.handle, pc.handle, bg, C.c_void_p(target.ptr), target.pitch, C.byref(t),
                                         C.c_void_p(stream or 0)))
        self._aux_last = want
        return target.ptr

    def upload_target(self, image: np.ndarray, stream=None):
        """Copy a host image into the renderer-owned target (prepared viewport; H x W x 4 of the target's dtype: float32,
        float16 or uint8), e.g. the sky or mesh pass that render_composite(load=True) puts the splats over.  Ordered on
        `stream` and waited for."""
        w, h = self._viewport
        img = np.ascontiguousarray(image)
        if img.shape != (h, w, 4) or img.dtype != self.np_dtype:
            raise ValueError(f"upload_target: want a ({h}, {w}, 4) {np.dtype(self.np_dtype).name} image, got {img.shape} {img.dtype}")
        target = self._own_target()
        target.upload(img, stream)
        return target.ptr

    def render_composite(self, pc: PointCloud, target_ptr: int = None, pitch: int = None, load=True, occluder=None,
                         occluder_kind="view_z", occluder_pitch: int = None, depth=False, median_depth=False, alpha=False,
                         background=(0.0, 0.0, 0.0, 0.0), stream=None):
        """ws_renderer_render_composite: the splats over the texels the target holds (load=True: out = C + T * dst, dst decoded
        from the target's format; load=False: over `background`, as render()) and, with an occluder, behind an opaque depth
        buffer: splat i takes part at pixel p iff z_i < D(p) (its centre depth, in f32).

        occluder: None, an (H, W) float32 numpy array (uploaded on `stream` into a renderer-owned buffer), or a device pointer
        with `occluder_pitch` bytes per row (default 4 x W).  occluder_kind "view_z": D = the value (view-space depth, positive
        in front of the camera; +inf = nothing there, NaN keeps no splat); "ndc": a [0, 1] depth-buffer value d under the
        frame's own projection, D = (n f) / (f - d (f - n)) in f32 with no FMA, d >= 1 = +inf.  An occluder needs
        enable_depth() before prepare().  target_ptr None = the renderer-owned target (fill it with upload_target()).
        depth / median_depth / alpha: the planes of render_aux(), over the unoccluded splats (download_aux())."""
        w, h = self._viewport
        if target_ptr is None:
            target_ptr = self._own_target().ptr
        if pitch is None:
            pitch = w * self.texel_bytes
        desc = L.ws_composite_desc()
        desc.load = 1 if load else 0
        desc.occluder_kind = {"view_z": L.WS_OCCLUDER_VIEW_Z, "ndc": L.WS_OCCLUDER_NDC_DEPTH}[occluder_kind]
        if occluder is not None:
            if isinstance(occluder, np.ndarray):
                occ = np.ascontiguousarray(occluder, dtype=np.float32)
                if occ.shape != (h, w):
                    raise ValueError(f"render_composite: want an ({h}, {w}) occluder, got {occ.shape}")
                self._occluder.fit(w, h)
                own = self._occluder.plane("occluder", np.float32)
                own.upload(occ, stream)  # (on the frame's stream: a frame still in flight there reads the previous plane)
                desc.occluder, desc.occluder_pitch = own.ptr, own.pitch
            else:
                desc.occluder, desc.occluder_pitch = int(occluder), int(occluder_pitch if occluder_pitch is not None else w * 4)
        t, want = self._aux_targets(depth, median_depth, alpha)
        bg = (C.c_float * 4)(*[float(x) for x in background])
        check(lib.ws_renderer_render_composite(self.handle, pc.handle, bg, C.c_void_p(target_ptr), pitch, C.byref(t),
                                               C.byref(desc), C.c_void_p(stream or 0)))
        self._aux_last = want
        return target_ptr

    def download_aux(self) -> dict:
        """{plane name: H x W float32} of the planes the last render_aux() wrote (syncs)."""
        self.ctx.sync()
        return {name: self._aux.get(name).download() for name in self._aux_last}

    def download_depths(self) -> np.ndarray:
        """The prepared frame's view-space depth per visible splat, store order (needs enable_depth before prepare; syncs)."""
        nv = C.c_uint32()
        check(lib.ws_renderer_download_depths(self.handle, 0, None, C.byref(nv)))
        z = np.empty(nv.value, dtype=np.float32)
        if nv.value:
            check(lib.ws_renderer_download_depths(self.handle, nv.value, z.ctypes.data_as(C.POINTER(C.c_float)), C.byref(nv)))
        return z

    def download_target_rgba8(self) -> np.ndarray:
        """bin/render.rs:187-246 download_texture of the renderer-owned target: H x W x 4 uint8 (truncating)."""
        target = self._target.get("target")
        h, w = target.shape[:2]
        out = np.empty((h, w, 4), dtype=np.uint8)
        check(lib.ws_download_texture_rgba8(self.ctx.handle, C.c_void_p(target.ptr), FORMATS[self.color_format_name][0],
                                            w, h, target.pitch, out.ctypes.data_as(C.c_void_p), None))
        return out

    def display(self, background=(0.0, 0.0, 0.0, 1.0), surface="rgba8unorm") -> np.ndarray:
        """Display::render (renderer.rs:548-582) of the renderer-owned target into an 8-bit surface: H x W x 4."""
        target = self._target.get("target")
        h, w = target.shape[:2]
        with DeviceArray(self.ctx, (h, w, 4), np.uint8) as dst:
            bg = (C.c_float * 4)(*[float(x) for x in background])
            sf = {"rgba8unorm": L.WS_SURFACE_RGBA8_UNORM, "bgra8unorm": L.WS_SURFACE_BGRA8_UNORM}[surface]
            check(lib.ws_display_composite(self.ctx.handle, C.c_void_p(target.ptr), FORMATS[self.color_format_name][0],
                                           target.pitch, w, h, bg, sf, C.c_void_p(dst.ptr), dst.pitch, None))
            self.ctx.sync()
            return dst.download()

    def download_target(self) -> np.ndarray:
        """download_texture (bin/render.rs:187-246) for the renderer-owned target: H x W x 4."""
        self.ctx.sync()
        return self._target.get("target").download()

    def num_visible_points(self) -> int:
        v = C.c_uint32()
        check(lib.ws_renderer_num_visible(self.handle, C.byref(v)))
        return v.value

    def frame_stats(self):
        s = L.ws_frame_stats()
        check(lib.ws_renderer_frame_stats(self.handle, C.byref(s)))
        return {"num_visible": s.num_visible, "num_tile_entries": s.num_tile_entries,
                "tile_entries_capacity": s.tile_entries_capacity, "overflow": s.overflow}

    def errors(self, reset=False):
        """(bits, entries_needed): error bits of every frame drawn since creation / the last reset (syncs)."""
        bits, need = C.c_uint32(), C.c_uint32()
        check(lib.ws_renderer_errors(self.handle, C.byref(bits), C.byref(need), int(bool(reset))))
        return bits.value, need.value

    def stage_times(self):
        s = L.ws_stage_times()
        check(lib.ws_renderer_stage_times(self.handle, C.byref(s)))
        return {"preprocess": s.preprocess_ms, "sorting": s.sorting_ms, "binning": s.binning_ms,
                "rasterization": s.rasterization_ms}

    def download_frame(self, with_src_index=False):
        v = self.num_visible_points()
        splats = np.empty((v, 20), dtype=np.uint8)
        keys = np.empty(v, dtype=np.uint32)
        sorted_idx = np.empty(v, dtype=np.uint32)
        src = np.empty(v, dtype=np.uint32) if with_src_index else None
        nv = C.c_uint32()
        check(lib.ws_renderer_download_frame(
            self.handle, v, splats.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p),
            src.ctypes.data_as(C.c_void_p) if src is not None else None, sorted_idx.ctypes.data_as(C.c_void_p),
            C.byref(nv)))
        return {"num_visible": nv.value, "splats": splats, "keys": keys, "sorted": sorted_idx, "src_index": src}


class ViewBatch:
    """Several frames in flight over one resident scene (ws_view_batch_*): the unit a rank renders its shard of views with."""

    def __init__(self, ctx: Context, color_format: str = "rgba32float", sh_deg: int = 3, compressed: bool = False,
                 frames_in_flight: int = 4):
        self.ctx = ctx
        self.color_format_name = color_format
        fmt, self.np_dtype, self.texel_bytes = FORMATS[color_format]
        h = C.c_void_p()
        check(lib.ws_view_batch_create(ctx.handle, fmt, int(sh_deg), int(compressed), int(frames_in_flight), C.byref(h)))
        self.handle = h
        self.frames_in_flight = lib.ws_view_batch_frames_in_flight(h)

    def close(self):
        if self.handle:
            lib.ws_view_batch_destroy(self.handle)
            self.handle = None

    @staticmethod
    def pack_views(views):
        """SplattingArgs list -> contiguous ws_splatting_args array (convert once, render many times)."""
        arr = (L.ws_splatting_args * len(views))()
        for i, v in enumerate(views):
            arr[i] = v.to_c()
        return arr

    def render(self, pc: "PointCloud", views, target_ptrs, row_pitch: int, background=(0.0, 0.0, 0.0, 0.0)):
        """Enqueue len(views) frames (views: list of SplattingArgs or a pack_views() array); returns immediately."""
        arr = views if isinstance(views, C.Array) else ViewBatch.pack_views(views)
        n = len(arr)
        tp = target_ptrs if isinstance(target_ptrs, C.Array) else (C.c_void_p * n)(*[int(p) for p in target_ptrs])
        bg = (C.c_float * 4)(*[float(x) for x in background])
        check(lib.ws_view_batch_render(self.handle, pc.handle, arr, n, tp, int(row_pitch), bg))

    def sync(self):
        check(lib.ws_view_batch_sync(self.handle))

    def errors(self, reset=False):
        """OR of the slots' sticky error bits (tile-entry overflow, look-back time-outs); syncs."""
        bits = C.c_uint32()
        check(lib.ws_view_batch_errors(self.handle, C.byref(bits), int(bool(reset))))
        return bits.value

    def host_waits(self) -> int:
        """times render() slept because a slot's host side was queue_depth frames ahead of the device (websplat.h)."""
        return int(lib.ws_view_batch_host_waits(self.handle))

    def renderer(self, slot: int) -> "GaussianRenderer":
        """A non-owning view of slot's renderer (frame_stats, timers): its close() leaves the slot's renderer alone."""
        return GaussianRenderer._view(self.ctx, C.c_void_p(lib.ws_view_batch_renderer(self.handle, int(slot))),
                                      self.color_format_name)


class GPURSSorter:
    """gpu_rs.rs: GPURSSorter::new + create_sort_stuff(max_n); sort() = record_sort / record_sort_indirect."""

    def __init__(self, ctx: Context, max_n: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(lib.ws_sorter_create(ctx.handle, int(max_n), C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            lib.ws_sorter_destroy(self.handle)
            self.handle = None

    def sort(self, d_keys: int, d_payload: int, n: int, d_count: int = None, stream=None):
        check(lib.ws_sorter_sort(self.handle, C.c_void_p(d_keys), C.c_void_p(d_payload),
                                 C.c_void_p(d_count) if d_count else None, int(n), C.c_void_p(stream or 0)))

    def sort_depth(self, d_keys: int, d_payload: int, n: int, d_aux: int = None, d_count: int = None, stream=None):
        """The renderer's depth sort as a stand-alone call: same result as sort(), a 4-byte companion value rides along."""
        check(lib.ws_sorter_sort_depth(self.handle, C.c_void_p(d_keys), C.c_void_p(d_payload),
                                       C.c_void_p(d_aux) if d_aux else None, C.c_void_p(d_count) if d_count else None,
                                       int(n), C.c_void_p(stream or 0)))

    def depth_range(self):
        """(base, skip, span_class) the device decided in the last sort_depth (ws_sorter_depth_range); raises when that sort did
        not fold its key range (WS_DEPTH_SKIP_TOP=0, the fat-tile form)."""
        b, s, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.ws_sorter_depth_range(self.handle, C.byref(b), C.byref(s), C.byref(c)))
        return b.value, s.value, c.value

    def sort_host(self, keys: np.ndarray, payload: np.ndarray, count: int = None, depth: bool = False, aux: np.ndarray = None):
        """Convenience for tests: upload, sort, download. `count` exercises the device-side count path; `depth`
        selects the depth-sort specialisation, `aux` its companion values (returned as a third array)."""
        n = keys.shape[0]
        with contextlib.ExitStack() as held:
            def dev(a):
                return None if a is None else held.enter_context(DeviceArray.from_host(self.ctx, np.asarray(a).astype(np.uint32)))

            dk, dv, da, dc = dev(keys), dev(payload), dev(aux), dev(None if count is None else [count])
            if depth:
                self.sort_depth(dk.ptr, dv.ptr, n, da and da.ptr, dc and dc.ptr)
            else:
                self.sort(dk.ptr, dv.ptr, n, dc and dc.ptr)
            self.ctx.sync()
            return tuple(d.download() for d in (dk, dv, da) if d is not None)
