/*
 * websplat.h -- C ABI of libwebsplat_hip.so, the MI355X (gfx950) drop-in for
 * web-splat's render hot path (GaussianRenderer::prepare + render and the
 * GPURSSorter they drive).
 *
 * Every entry point names the reference interface it replaces (file:line under
 * /root/reference).  Plain pointers and sizes only; no C++ / torch types.
 * All functions return WS_OK (0) or a negative ws_status; the message of the
 * last failure on the calling thread is available from ws_last_error().
 * Nothing throws across this boundary.
 *
 * Threading: handles are not thread-safe; use one context / renderer per host
 * thread (the reference records single-threaded, renderer.rs:191-260).
 * Async: prepare/render/sort only ENQUEUE work on the given HIP stream
 * (hipStream_t passed as void*; NULL = the default stream) and return; the
 * caller observes completion with ws_sync() -- the analogue of
 * queue.submit + device.poll(Wait) (bin/measure.rs:147).
 */
#ifndef WEBSPLAT_H
#define WEBSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WS_ABI_VERSION 3 /* 3: ws_context_config / ws_context_create_with_config; the library reads no environment variable */

typedef enum ws_status {
    WS_OK = 0,
    WS_ERR_INVALID = -1,     /* bad argument / layout mismatch */
    WS_ERR_HIP = -2,         /* a HIP runtime call failed (text in ws_last_error) */
    WS_ERR_OOM = -3,
    WS_ERR_UNSUPPORTED = -4, /* e.g. sh_deg > 3 */
    WS_ERR_STATE = -5,       /* e.g. render() before prepare() */
    WS_ERR_IO = -6,          /* loaders */
    WS_ERR_OVERFLOW = -7     /* device-side capacity exceeded (tile entries) */
} ws_status;

/* wgpu::TextureFormat choices the reference's front-ends use for the splat target:
 * Rgba8Unorm (lib.rs / bin/measure.rs), Rgba16Float (bin/render.rs:140), Rgba32Float (bin/video.rs). */
typedef enum ws_color_format {
    WS_FORMAT_RGBA8_UNORM = 0,
    WS_FORMAT_RGBA16_FLOAT = 1,
    WS_FORMAT_RGBA32_FLOAT = 2
} ws_color_format;

typedef struct ws_context ws_context;       /* wgpu Device+Queue      (lib.rs:57-125 WGPUContext) */
typedef struct ws_pointcloud ws_pointcloud; /* pointcloud.rs:72-88    PointCloud */
typedef struct ws_renderer ws_renderer;     /* renderer.rs:17-30      GaussianRenderer */
typedef struct ws_sorter ws_sorter;         /* gpu_rs.rs:23-42        GPURSSorter + PointCloudSortStuff */

/* pointcloud.rs:398-403 Aabb<f32> */
typedef struct ws_aabb {
    float min[3];
    float max[3];
} ws_aabb;

/* pointcloud.rs:360-396 Quantization / GaussianQuantization (64 B, uniform layout) */
typedef struct ws_quantization {
    int32_t zero_point;
    float scale;
    uint32_t _pad[2];
} ws_quantization;
typedef struct ws_gaussian_quantization {
    ws_quantization color_dc, color_rest, opacity, scaling_factor;
} ws_gaussian_quantization;

/* What io/mod.rs:27-43 GenericGaussianPointCloud hands to PointCloud::new (pointcloud.rs:99-199):
 * the loader's byte blobs, verbatim, in HOST memory.
 *   uncompressed: gaussians = num_points x 28 B  (pointcloud.rs:38-45 Gaussian)
 *                 sh_coefs  = num_points x 96 B  ([[f16;3];16], io/mod.rs:65)
 *   compressed:   gaussians = num_points x 24 B  (pointcloud.rs:14-22 GaussianCompressed)
 *                 sh_coefs  = packed int8, 3*(sh_deg+1)^2 B per SH entry (io/npz.rs:183-196)
 *                 covars    = n_covars x 12 B (pointcloud.rs:61-63 Covariance3D)
 *                 quantization = 64 B block */
typedef struct ws_pointcloud_desc {
    uint32_t num_points;
    uint32_t sh_deg;
    int32_t compressed;
    const void* gaussians;
    size_t gaussians_bytes;
    const void* sh_coefs;
    size_t sh_coefs_bytes;
    const void* covars; /* compressed only */
    size_t covars_bytes;
    const ws_gaussian_quantization* quantization; /* compressed only */
    ws_aabb bbox;
    float center[3];
    int32_t has_up;
    float up[3];
    int32_t has_mip_splatting;
    int32_t mip_splatting;
    int32_t has_kernel_size;
    float kernel_size;
    int32_t has_background_color;
    float background_color[3];
} ws_pointcloud_desc;

/* camera.rs:6-11 PerspectiveCamera + camera.rs:85-94 PerspectiveProjection */
typedef struct ws_camera {
    float position[3];
    float rotation[4]; /* cgmath Quaternion (s, x, y, z) */
    float fovx, fovy;  /* radians */
    float znear, zfar;
    float fov2view_ratio;
} ws_camera;

/* renderer.rs:585-599 SplattingArgs; Option<T> fields carry explicit has_* flags */
typedef struct ws_splatting_args {
    ws_camera camera;
    uint32_t viewport[2];
    float gaussian_scaling;
    uint32_t max_sh_deg;
    int32_t has_mip_splatting;
    int32_t mip_splatting;
    int32_t has_kernel_size;
    float kernel_size;
    int32_t has_clipping_box;
    ws_aabb clipping_box;
    double walltime_secs; /* Duration */
    int32_t has_scene_center;
    float scene_center[3]; /* ignored, like the reference (renderer.rs:644) */
    int32_t has_scene_extend;
    float scene_extend;
    double background_color[4]; /* wgpu::Color; used by callers for the clear only */
} ws_splatting_args;

/* renderer.rs:290-306 CameraUniform (272 B) and renderer.rs:602-618 SplattingArgsUniform (80 B) */
typedef struct ws_camera_uniform {
    float view[16], view_inv[16], proj[16], proj_inv[16];
    float viewport[2], focal[2];
} ws_camera_uniform;
typedef struct ws_settings_uniform {
    float clip_min[4], clip_max[4];
    float gaussian_scaling;
    uint32_t max_sh_deg;
    uint32_t mip_splatting;
    float kernel_size;
    float walltime;
    float scene_extend;
    uint32_t _pad[2];
    float scene_center[4];
} ws_settings_uniform;

/* per-stage GPU time, the reference's GPUStopwatch labels (renderer.rs:221,230; lib.rs:448) plus binning */
typedef struct ws_stage_times {
    float preprocess_ms;
    float sorting_ms;
    float binning_ms;
    float rasterization_ms;
} ws_stage_times;

/* one kernel launch of the last frame, in launch order (utils.rs:26-134 GPUStopwatch at kernel granularity) */
typedef struct ws_kernel_time {
    char name[40];
    float ms;
} ws_kernel_time;

/* device-side statistics of the last prepared frame (forces a sync) */
typedef struct ws_frame_stats {
    uint32_t num_visible;      /* V: renderer.rs:170-189 num_visible_points */
    uint32_t num_tile_entries; /* D: sum over visible splats of tiles touched */
    uint32_t tile_entries_capacity;
    uint32_t overflow;         /* 1 if D exceeded the capacity (entries dropped) */
} ws_frame_stats;

const char* ws_last_error(void);
uint32_t ws_abi_version(void);
/* bit 0: this is the EXPERIMENTAL build (make experimental, lib_exp/): it also carries the measured-and-lost variants the
 * exp_* fields of ws_context_config select; the product library refuses them with WS_ERR_UNSUPPORTED */
#define WS_BUILD_EXPERIMENTAL 1u
uint32_t ws_build_flags(void);

/* ---- context: lib.rs:68-125 WGPUContext::new_instance / new --------------------------------- */
/* ws_context_create uses the defaults of ws_context_config_init.  THE LIBRARY READS NO ENVIRONMENT VARIABLE: a drop-in
 * library must not be steered by the environment of whoever loads it.  Tuning / analysis switches travel in this struct;
 * bench.py, the tests and the tools/ mains translate their WS_* environment into it OUTSIDE the library
 * (include/websplat_env.h, web-splat_amd/websplat/api.py config_from_env). */
typedef struct ws_context_config {
    uint32_t struct_size;      /* sizeof(ws_context_config) of the caller: the struct may grow at its end */
    int32_t use_graph;         /* 0; 1 = prepare() on a real stream replays a captured frame graph (opt-in: ROCm 7.2 fault) */
    int32_t depth_skip_top;    /* 1; 0 = the depth sort always runs all of its passes (A/B) */
    int32_t blend_order;       /* -1 automatic; 0 image order; 1 longest list first; 2 / 3 measured experiments */
    int32_t blend_split;       /* -1 automatic (tiles < 2 x CUs); 0 / 1 never / always two half-tile workgroups per binning tile */
    int32_t bin_request;       /* 1 = decided per frame on the device (default); 0 never / 2 always bin at twice the blend's tile */
    int32_t batch_threads;     /* -1 automatic; 0 / 1 = a view batch never / always enqueues every slot from its own host thread */
    int32_t batch_queue_depth; /* -1 = default (5): frames a slot's host side may run ahead of the device; 0 = unbounded */
    int32_t blend_tpw_log2;    /* -1 automatic; tiles per blend workgroup = 2^n (4K-class tile counts) */
    int32_t blend_lds_pad_kb;  /* 0; unused dynamic LDS per blend workgroup (occupancy experiments) */
    int32_t tile_qw, tile_qh;  /* 4, 4: 8x8-px quadrants per compositing tile (2x2, 4x2 or 4x4) */
    int32_t debug_cut;         /* 0; analysis: stop every frame after stage n (1 = K1 ... 4 = tile sort) */
    int32_t capture;           /* 0; 1 = renderers keep per-splat source indices / per-tile debug words (tests) */
    int32_t render_views_fast_blend; /* 0; 1 = ws_render_views composites with the throughput blend instead of target precision */
    int32_t ply_decode_host;   /* 0; 1 = ws_load_ply converts the vertex rows on the host instead of on the device */
    int32_t depth_digit_bits;  /* 0 = default; 8 = four 8-bit passes (the reference's shape), 9 = three 9-bit passes over key - base */
    int32_t depth_tile_kpt;    /* 0 = by input size; 4 / 8 = keys per thread of the 9-bit depth sort's tiles (A/B) */
    int32_t blend_async;       /* -1 / 0 = k_blend (two workgroup barriers per staged batch); 1 = k_blend2 (double-buffered staging, LDS
                                * arrival counters, no per-batch barrier: bit-identical images, measured slower -- experimental build only) */
    /* measured-and-lost variants: honoured by the EXPERIMENTAL build only (lib_exp); the product library refuses non-defaults */
    int32_t exp_depth_sort;    /* 0 scan (default) | 1 fat-tile one-sweep | 2 one cooperative launch */
    int32_t exp_dsort_fat_grid;
    int32_t exp_blend_variant; /* 1 = k_blend_q */
    int32_t exp_blend_dma;     /* 1 = LDS-DMA staging */
    int32_t exp_batch_k1;      /* 1 (default) .. 4 views per K1 launch */
    int32_t exp_footprint_ellipse;
    int32_t exp_tile_sort_wide;
    int32_t reserved[6];       /* zero */
} ws_context_config;
void ws_context_config_init(ws_context_config* cfg); /* fills in the defaults above */
int ws_context_create(int hip_device, ws_context** out);
int ws_context_create_with_config(int hip_device, const ws_context_config* cfg, ws_context** out);
void ws_context_destroy(ws_context* ctx);
int ws_sync(ws_context* ctx, void* stream); /* device.poll(Wait) */
/* How a host thread of this process waits for the context's device in ws_sync / hipStreamSynchronize / the read-backs:
 * WS_HOST_WAIT_BLOCK sleeps until the completion interrupt -- what device.poll(wgpu::PollType::Wait) does behind
 * queue.submit (bin/measure.rs:147) -- WS_HOST_WAIT_SPIN polls (the HIP runtime's default: lowest wake-up latency, one
 * host core busy for as long as the wait lasts).  A process-wide property of the HIP device (hipSetDeviceFlags): eight
 * ranks of one node that wait spinning keep eight cores busy doing nothing. */
typedef enum ws_host_wait { WS_HOST_WAIT_SPIN = 0, WS_HOST_WAIT_BLOCK = 1 } ws_host_wait;
int ws_context_set_host_wait(ws_context* ctx, ws_host_wait mode);
int ws_device_info(ws_context* ctx, char* name, size_t name_len, uint32_t* num_cus, uint64_t* hbm_bytes);
/* plain device buffers for callers without their own allocator (tests, C++ drivers);
 * the analogue of device.create_buffer + queue.write_buffer + DownloadBuffer */
int ws_device_malloc(ws_context* ctx, size_t bytes, void** d_ptr);
int ws_device_free(ws_context* ctx, void* d_ptr);
int ws_memcpy_h2d(ws_context* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream);
int ws_memcpy_d2h(ws_context* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream);

/* ---- host-side boundary math (no GPU needed) ------------------------------------------------- */
/* camera.rs:26-35 PerspectiveCamera::fit_near_far */
int ws_camera_fit_near_far(ws_camera* cam, const ws_aabb* bbox);
/* scene.rs:85-108 impl Into<PerspectiveCamera> for SceneCamera (rotation = 3 rows of 3, as in cameras.json) */
int ws_camera_from_scene(const float position[3], const float rotation[9], float fx, float fy, uint32_t width,
                         uint32_t height, ws_camera* out);
/* renderer.rs:136-141 + 321-343 CameraUniform::set_camera / set_viewport / set_focal */
int ws_build_camera_uniform(const ws_camera* cam, const uint32_t viewport[2], ws_camera_uniform* out);
/* renderer.rs:620-651 SplattingArgsUniform::from_args_and_pc */
int ws_build_settings_uniform(const ws_splatting_args* args, const ws_pointcloud* pc, ws_settings_uniform* out);
/* pointcloud.rs:444-452 Aabb::center / radius */
float ws_aabb_radius(const ws_aabb* b);

/* ---- loaders' data prep (io/ply.rs:50-100, io/mod.rs:63-105, utils.rs:194-212) ---------------- */
/* Convert INRIA-layout PLY vertex rows (f32, little-endian, property order of io/ply.rs:54-88;
 * row length 3+3+3*(sh_deg+1)^2+1+3+4) into Gaussian (28 B) + SH (96 B) records. */
int ws_ply_rows_convert(const float* rows, uint32_t n, uint32_t sh_deg, void* gaussians_out, void* sh_out);
/* bbox (grown from `start`: Aabb::zeroed() for PLY io/mod.rs:74, Aabb::unit() for NPZ io/mod.rs:119),
 * centroid and plane-fit up vector.  stride = 28 or 24. */
int ws_pointcloud_stats(const void* gaussians, uint32_t n, uint32_t stride, const ws_aabb* start, ws_aabb* bbox,
                        float center[3], int32_t* has_up, float up[3]);
/* io/mod.rs:45-61 GenericGaussianPointCloud::load for a binary PLY file, then PointCloud::new */
int ws_pointcloud_load_ply(ws_context* ctx, const char* path, ws_pointcloud** out);
/* io/ply.rs:28-196 PlyReader::read + GenericGaussianPointCloud::new (io/mod.rs:63-105) on the HOST: the INRIA 3DGS
 * .ply decoded into the loader's byte blobs (Gaussian 28 B x N, SH 96 B x N; host memory owned by the returned
 * object), bbox grown from Aabb::zeroed(), centroid, plane fit, header comments.  No GPU needed. */
typedef struct ws_ply_cloud {
    uint32_t num_points;
    uint32_t sh_deg;
    const void* gaussians;
    size_t gaussians_bytes;
    const void* sh_coefs;
    size_t sh_coefs_bytes;
    ws_aabb bbox;
    float center[3];
    int32_t has_up;
    float up[3];
    int32_t has_mip_splatting;
    int32_t mip_splatting;
    int32_t has_kernel_size;
    float kernel_size;
    int32_t has_background_color;
    float background_color[3];
} ws_ply_cloud;
int ws_ply_read(const char* path, ws_ply_cloud** out);
void ws_ply_free(ws_ply_cloud* pc);

/* io/npz.rs:59-225 NpzReader::read: a c3dgs .npz decoded into the loader's byte blobs (HOST memory, owned by the
 * returned object): GaussianCompressed 24 B x N, packed int8 SH records 3*(sh_deg+1)^2 B, Covariance3D 12 B x M,
 * the 64-B quantisation block and the optional scalars.  No GPU needed. */
typedef struct ws_npz_cloud {
    uint32_t num_points;
    uint32_t sh_deg;
    const void* gaussians;
    size_t gaussians_bytes;
    const void* sh_coefs;
    size_t sh_coefs_bytes;
    const void* covars;
    size_t covars_bytes;
    ws_gaussian_quantization quantization;
    int32_t has_kernel_size;
    float kernel_size;
    int32_t has_mip_splatting;
    int32_t mip_splatting;
    int32_t has_background_color;
    float background_color[3];
} ws_npz_cloud;
int ws_npz_read(const char* path, ws_npz_cloud** out);
void ws_npz_free(ws_npz_cloud* pc);
/* NpzReader::read + GenericGaussianPointCloud::new_compressed (io/mod.rs:107-150) + PointCloud::new */
int ws_pointcloud_load_npz(ws_context* ctx, const char* path, ws_pointcloud** out);
/* io/mod.rs:45-61 GenericGaussianPointCloud::load: reader chosen by magic bytes ("ply" / "PK\3\4") */
int ws_pointcloud_load(ws_context* ctx, const char* path, ws_pointcloud** out);

/* ---- PointCloud: pointcloud.rs:99-222, 336-349 ------------------------------------------------ */
/* Positions are taken as they are: a Gaussian with a NaN coordinate fails no cull comparison, as in the reference, and yields a
 * visible slot (NaN axes and centre, a NaN depth key of either sign) that reaches no tile and leaves every other splat and the
 * image as they would be without it; +-inf coordinates are culled by the clip box.  bbox and center are the caller's too (the
 * fade-in is computed from them as declared, wherever the centre lies). */
int ws_pointcloud_create(ws_context* ctx, const ws_pointcloud_desc* desc, ws_pointcloud** out);
/* PlyReader::read (io/ply.rs:50-100, 164-196) + GenericGaussianPointCloud::new (io/mod.rs:63-105) + PointCloud::new
 * with the per-vertex conversion on the GPU: `rows` = n raw vertex rows of the INRIA layout (14 + 3*(sh_deg+1)^2 f32
 * each, host memory, native endianness); bbox / centroid / up are computed from them on the host; `meta` (may be
 * NULL) supplies the optional mip_splatting / kernel_size / background_color header values (the other fields of the
 * descriptor are ignored).  ws_pointcloud_load_ply takes this route. */
int ws_pointcloud_create_from_ply_rows(ws_context* ctx, const float* rows, uint32_t n, uint32_t sh_deg,
                                       const ws_pointcloud_desc* meta, ws_pointcloud** out);
/* The resident scene as loader blobs again (28-B Gaussians + 96-B SH records, or the 24-B compressed records):
 * accessor / parity tooling, the analogue of reading the PointCloud's buffers back (pointcloud.rs:201-222). */
int ws_pointcloud_download(const ws_pointcloud* pc, void* gaussians, size_t gaussians_bytes, void* sh_coefs, size_t sh_coefs_bytes);
void ws_pointcloud_destroy(ws_pointcloud* pc);
uint32_t ws_pointcloud_num_points(const ws_pointcloud* pc);
uint32_t ws_pointcloud_sh_deg(const ws_pointcloud* pc);
int ws_pointcloud_compressed(const ws_pointcloud* pc);
int ws_pointcloud_bbox(const ws_pointcloud* pc, ws_aabb* out);
int ws_pointcloud_center(const ws_pointcloud* pc, float out[3]);
int ws_pointcloud_up(const ws_pointcloud* pc, float out[3]);                   /* returns 1 if Some */
int ws_pointcloud_mip_splatting(const ws_pointcloud* pc, int32_t* out);        /* returns 1 if Some */
int ws_pointcloud_kernel_size(const ws_pointcloud* pc, float* out);            /* returns 1 if Some */
int ws_pointcloud_background_color(const ws_pointcloud* pc, float out[3]);     /* returns 1 if Some */

/* ---- GaussianRenderer: renderer.rs:33-123, 170-260, 281 --------------------------------------- */
/* GaussianRenderer::new(device, queue, color_format, sh_deg, compressed) */
int ws_renderer_create(ws_context* ctx, ws_color_format format, uint32_t sh_deg, int compressed, ws_renderer** out);
void ws_renderer_destroy(ws_renderer* r);
ws_color_format ws_renderer_color_format(const ws_renderer* r);
/* GaussianRenderer::prepare: reset counters -> preprocess (K1/K1c) -> depth radix sort -> tile binning.
 * (Re)allocates per-renderer scratch when pc.num_points or the viewport changes (renderer.rs:200-211). */
int ws_renderer_prepare(ws_renderer* r, const ws_pointcloud* pc, const ws_splatting_args* args, void* stream);
/* begin_render_pass(clear = background) + GaussianRenderer::render: composites the prepared frame into
 * d_rgba_out (device memory, viewport.y rows of row_pitch_bytes; texel = 4 x {u8 | f16 | f32} by format),
 * premultiplied RGBA over `background` (the clear colour, bin/render.rs:113-116). */
int ws_renderer_render(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba_out,
                       size_t row_pitch_bytes, void* stream);
/* ---- Auxiliary planes: where the image is (no counterpart in the reference) ------------------------------------------
 * All planes are f32, one value per pixel, rows of *_pitch bytes (at least 4 x viewport width, multiples of 4; 4-B aligned
 * pointers).  z_i is the view-space depth of splat i, (view * [x, y, z, 1]).z -- the f32 value the preprocess kernel computes,
 * positive in front of the camera.  w_i is the exact weight the FAST blend gives splat i at the pixel and T the
 * transmittance it ends with, both including the early termination at T < 2^-14:
 *   depth         expected depth sum(w_i z_i) / sum(w_i); 0 where nothing is drawn
 *   median_depth  z_i of the first splat, front to back, after which T <= 0.5; 0 where T never reaches 0.5
 *   alpha         coverage 1 - T, whatever the background; 0 where nothing is drawn
 * depth and median_depth need the frame's z plane: ws_renderer_enable_depth(r, 1) before prepare() (K1 then also writes
 * 4 B per visible splat).  Toggling it takes effect at the next prepare(). */
int ws_renderer_enable_depth(ws_renderer* r, int enable);
typedef struct ws_aux_targets {
    float* depth;              /* device pointers; any may be NULL */
    size_t depth_pitch;        /* bytes */
    float* median_depth;
    size_t median_depth_pitch;
    float* alpha;
    size_t alpha_pitch;
    uint32_t reserved[4];      /* must be zero */
} ws_aux_targets;
/* ws_renderer_render plus the auxiliary planes.  aux == NULL, or all three pointers NULL: exactly ws_renderer_render (same
 * launch, same bytes); the colour image is bit-identical to ws_renderer_render's in every case.  Errors: WS_ERR_STATE when
 * depth or median_depth is asked for but the prepared frame has no z plane; WS_ERR_INVALID for a pitch below 4 x width, a
 * pitch or pointer not 4-B aligned, or a non-zero reserved word; WS_ERR_UNSUPPORTED with any plane under
 * WS_BLEND_TARGET_PRECISION or WS_BLEND_FAST_EXACT_CUT (not built yet: a later change), capture mode or blend timing. */
int ws_renderer_render_aux(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba_out,
                           size_t row_pitch_bytes, const ws_aux_targets* aux, void* stream);
/* ---- Compositing over an existing target, behind an opaque depth buffer ------------------------------------------------
 * The reference draws into a pass the caller begins (renderer.rs:250-260) with PREMULTIPLIED_ALPHA_BLENDING (renderer.rs:63-67),
 * so a host may begin it with LoadOp::Load and put the splats over a sky, a grid or a mesh pass.  This is that path, plus the
 * exact mesh + splat composite: every splat behind the opaque surface is dropped, per pixel, during the blend.
 * Below, T and the weights w_i are the FAST blend's, early termination included (WS_BLEND_TARGET_PRECISION: that blend's, no
 * early termination).
 *   comp == NULL, or load == 0 with no occluder: exactly ws_renderer_render_aux (same launch, same bytes).
 *   load == 1: out = C + T * dst on all four channels, C = sum(w_i c_i) the splats' premultiplied colour and coverage, dst the
 *     texel the target held, decoded from its format: f32, f16, or unorm8 as k / 255 (f32 division).  This is what the
 *     reference's pipeline computes over a loaded pass, with the FAST mode's single rounding at the store; the result is
 *     rounded once, as by ws_renderer_render.  `background` is ignored.  (WS_BLEND_TARGET_PRECISION starts its destination
 *     from dst and rounds after every splat, as a wgpu pass with LoadOp::Load does.)
 *   occluder: splat i takes part at pixel p iff z_i < D(p) in f32, z_i the value of the frame's z plane
 *     (ws_renderer_download_depths): per splat, at its centre depth -- the granularity of the depth sort.  A pair that fails
 *     the test is skipped exactly like a pair outside the cut-off: no weight, T unchanged.
 *       WS_OCCLUDER_VIEW_Z     D = occluder[p].  +inf means "no geometry here"; NaN drops every splat (the comparison is false).
 *       WS_OCCLUDER_NDC_DEPTH  D = (n * f) / (f - d * (f - n)), d = occluder[p], n and f the prepared frame's znear and zfar
 *                              (-proj[3][2] / proj[2][2] and -proj[3][2] / (proj[2][2] - 1), what K1 derives from the
 *                              projection).  Evaluated in f32 in exactly this order -- n * f, f - n, d * (f - n), the
 *                              difference, then a correctly rounded division -- with no contraction into an FMA.  d >= 1 (a
 *                              cleared depth buffer) is +inf.
 *   Auxiliary planes follow the same weights: depth, median_depth and alpha describe the unoccluded splats only; alpha stays
 *     1 - T whatever the target held.
 * Every pixel of the target is read and written by exactly one thread of the frame's compositing launch, once: the target
 * may be the caller's colour attachment itself.  The occluder plane is read only.
 * Errors: WS_ERR_STATE when an occluder is given but the prepared frame has no z plane (ws_renderer_enable_depth before
 * prepare()); WS_ERR_INVALID for an occluder pitch below 4 x width, a pitch or pointer not 4-B aligned, load other than 0 / 1,
 * a non-zero reserved word or an unknown kind (and render_aux's errors for the planes); WS_ERR_UNSUPPORTED with load or an
 * occluder under WS_BLEND_FAST_EXACT_CUT, in capture mode or with blend timing (as the planes; the planes also need
 * WS_BLEND_FAST). */
typedef enum ws_occluder_kind {
    WS_OCCLUDER_VIEW_Z = 0,     /* f32 view-space depth, positive in front of the camera: the units of the depth planes */
    WS_OCCLUDER_NDC_DEPTH = 1   /* f32 [0, 1] depth-buffer value under the frame's own projection (camera.rs build_proj, wgpu) */
} ws_occluder_kind;
typedef struct ws_composite_desc {
    uint32_t load;              /* 0: clear to `background` first (= render / render_aux); 1: LoadOp::Load, over the target's texels */
    uint32_t occluder_kind;     /* ws_occluder_kind */
    const float* occluder;      /* device plane, one f32 per pixel; NULL = no depth test */
    size_t occluder_pitch;      /* bytes; >= 4 x width, multiple of 4; 4-B aligned pointer */
    uint32_t reserved[4];       /* must be zero */
} ws_composite_desc;
int ws_renderer_render_composite(ws_renderer* r, const ws_pointcloud* pc, const float background[4], void* d_rgba,
                                 size_t row_pitch_bytes, const ws_aux_targets* aux, const ws_composite_desc* comp,
                                 void* stream);
/* GaussianRenderer::num_visible_points (syncs) */
int ws_renderer_num_visible(ws_renderer* r, uint32_t* out);
int ws_renderer_frame_stats(ws_renderer* r, ws_frame_stats* out); /* syncs */
/* Error bits of EVERY frame this renderer drew since creation / the last reset (syncs; bit 4 = a compositing workgroup waited
 * ~1 s for a staged batch that never came -- k_blend2's bounded spin): bit 0 = the (tile, splat)
 * entry list overflowed its capacity (entries_needed = what the last frame would have needed), bits 1..3 = a
 * look-back spin timed out.  The reference has no counterpart: wgpu validates sizes up front and the ROPs cannot
 * overflow; here the binned entry list can, and a caller that enqueues frames back to back (bin/measure.rs:98-153)
 * checks once after its wait. */
int ws_renderer_errors(ws_renderer* r, uint32_t* bits, uint32_t* entries_needed, int reset);
/* GPUStopwatch::take_measurements for the last frame (syncs); needs ws_renderer_enable_timers(r,1) */
/* enable: 0 = off, 1 = the four stage labels, 2 = additionally one HIP event pair per kernel launch */
int ws_renderer_enable_timers(ws_renderer* r, int enable);
int ws_renderer_stage_times(ws_renderer* r, ws_stage_times* out);
/* per-launch GPU time of the last frame (prepare + render), launch order; *count = launches recorded. Syncs.
 * Each time is a HIP-event interval = dispatch latency of a dependent launch + the kernel; the entry
 * "_empty_launch" (after the preprocess kernel) is an empty kernel recorded the same way (subtract it to compare with rocprofv3 durations). */
int ws_renderer_kernel_times(ws_renderer* r, uint32_t capacity, ws_kernel_time* out, uint32_t* count);
/* How render() composites (src/renderer.rs:63-67 PREMULTIPLIED_ALPHA_BLENDING on the pass's target):
 *   WS_BLEND_FAST (default)      front to back with early termination, accumulators in f32, ONE rounding at the store;
 *   WS_BLEND_TARGET_PRECISION    the reference's fixed-function blend literally: back to front over the clear colour,
 *                                the destination rounded to the target's precision (f16 RNE / unorm8 RNE / f32) after
 *                                EVERY splat, no early termination -- what bin/render.rs:154 (Rgba16Float) and
 *                                bin/measure.rs:184 (Rgba8Unorm) write.  Several times slower; ws_render_views uses it.
 *   WS_BLEND_FAST_EXACT_CUT      WS_BLEND_FAST, but a fragment within a few ulp of the cut-off (gaussian.wgsl:61, a > 2 CUTOFF
 *                                discards: a step of 0.009 * alpha in its weight) is kept or discarded by the reference's own
 *                                expression, dot(screen_pos, screen_pos) from the un-prescaled inverse, re-derived from the Splat
 *                                record (rare: ~1e-5 of the fragments).  No cut-off boundary pixel is left between this mode and
 *                                the f32 reference image (max-abs 6.1e-5, the early-out bound, on the uncompressed workloads);
 *                                the band test costs the blend +5 ... +7 % (frames/s -3 %), so it is a mode, not the default.
 * Takes effect at the next render(). */
typedef enum ws_blend_mode { WS_BLEND_FAST = 0, WS_BLEND_TARGET_PRECISION = 1, WS_BLEND_FAST_EXACT_CUT = 2 } ws_blend_mode;
int ws_renderer_set_blend_mode(ws_renderer* r, int mode);
/* parity tooling: also record the original Gaussian index of every store slot (costs 4 B per visible splat) */
int ws_renderer_enable_capture(ws_renderer* r, int enable);
/* Capacity of the (tile, splat) entry list; 0 = automatic: max(8 M, 4 per Gaussian per Mpixel), twice what the BASELINE
 * scenes need.  A frame that needs more sets error bit 0 and leaves its demand in a word that survives the per-frame reset;
 * once ws_renderer_errors (or ws_view_batch_errors) has read it, the next prepare() with the automatic capacity allocates
 * 1.25 x that demand.  An overflowed frame keeps the first `capacity` entries in draw order (far to near; within a splat rows
 * top to bottom, columns left to right): its tile lists are those of exactly these entries.  Takes effect at the next prepare. */
int ws_renderer_set_tile_entry_capacity(ws_renderer* r, uint64_t entries);
/* parity read-back of the prepared frame (the reference's test tooling reads buffers back the same way,
 * gpu_rs.rs:900-941 download_buffer): splats = V x 20 B in store order, keys/src_index = V u32 in store
 * order (src_index = original Gaussian index of each slot), sorted = V u32 store indices in draw order
 * (far -> near).  Any pointer may be NULL.  capacity = number of elements each array can hold. Syncs.
 * src_index needs a frame whose K1 kept it: capture mode, or ws_renderer_enable_contrib before prepare(). */
int ws_renderer_download_frame(ws_renderer* r, uint32_t capacity, void* splats, uint32_t* keys,
                               uint32_t* src_index, uint32_t* sorted, uint32_t* num_visible);
/* The prepared frame's z plane: V view-space depths in store order (the order of ws_renderer_download_frame's splats; z may be
 * NULL to read num_visible only).  WS_ERR_STATE when depth was off at prepare().  Syncs. */
int ws_renderer_download_depths(ws_renderer* r, uint32_t capacity, float* z, uint32_t* num_visible);
/* The binning tile the LAST prepared frame used: the context's tile (ws_context_tile_size) or, when the frame's splats span
 * several tiles, 2 x 2 blocks of it -- decided per frame on the device from the tile counts K1 sums for both sizes (a pure
 * function of the frame; WS_BIN_SHIFT=0 / 1 forces it off / on; frames in capture mode always use the context's tile).
 * Four compositing workgroups then share one binned list: half the (tile, splat) entries to emit and sort.  Syncs. */
int ws_renderer_binning_tile(ws_renderer* r, uint32_t* width, uint32_t* height);
/* Digit passes the depth sort of the LAST prepared frame executed, and (digit_bits, may be NULL) their width.  The reference
 * always runs four 8-bit passes (gpu_rs.rs:865-884).  Here the sort's first histogram kernel -- which reads every key anyway --
 * leaves the frame's key range on the device; the passes behind it take their digits from (key - base), and the last of the
 * four enqueued passes leaves at once when it would run over a constant digit (the identity): 3 passes on a frame whose keys
 * span less than 2^24 (8-bit digits: a camera outside the scene) or 2^27 (9-bit digits).  The compressed shader's keys
 * (preprocess_compressed.wgsl:325) are NOT confined to 24 bits: clip z is below znear for the nearest splats.  The digit
 * width is chosen per frame on the host from the key range the renderer's PREVIOUS frame posted (8 bits when it was below
 * 2^24, else 9; ws_context_config::depth_digit_bits forces it); either width gives the reference's stable order.  Syncs. */
int ws_renderer_depth_sort_passes(ws_renderer* r, uint32_t* passes);
int ws_renderer_depth_sort_digit_bits(ws_renderer* r, uint32_t* digit_bits); /* of the last prepared frame; no sync */
/* Analysis of FRAMES IN FLIGHT (no counterpart in the reference; rocprofv3's kernel trace serialises the hardware queues, so what
 * runs beside what has to be measured on the device): K1 and the compositing kernel of the next `frames` frames of this renderer
 * leave {first workgroup start, last workgroup end} on the device's 100-MHz clock -- stamps[frame][4] = K1 start, K1 end, blend
 * start, blend end; one clock shared by all renderers of the device.  frames = 0 switches it off.  download syncs. */
int ws_renderer_enable_frame_trace(ws_renderer* r, uint32_t frames);
int ws_renderer_download_frame_trace(ws_renderer* r, uint32_t capacity, uint64_t* stamps, uint32_t* count);
/* The compositing tile in pixels (one workgroup of the blend): 32x32 by default (four 16x16 tiles -- 4x4 wave quadrants
 * of 8x8 pixels -- sharing one binned list), 32x16 or 16x16 with WS_TILE_SHAPE=4x2|2x2 at context creation (tuning; 2x2 is
 * the literal one-workgroup-per-16x16-tile form).  Lists are built per BINNING tile: this tile, or 2 x 2 of them when the
 * frame decides so (ws_renderer_binning_tile). */
int ws_context_tile_size(const ws_context* ctx, uint32_t* width, uint32_t* height);
/* test hook, host only (no device work): the compositing pass's staging step for ONE (tile, splat) entry --
 * splat = the five 32-bit words of a 20-B Splat record (pointcloud.rs:352-358), tile origin in pixels ->
 * rec[10] = {i00, i01, c0, i10, i11, c1, alpha, r, g, b} (tile-local affine form of gaussian.wgsl:59-61 in the
 * exp2 domain) and the mask of 8x8-pixel quadrants (bit qy * (tile_w / 8) + qx) the kept ellipse may reach. */
int ws_debug_stage_splat(const uint32_t splat[5], float viewport_w, float viewport_h, float tile_x0, float tile_y0,
                         uint32_t tile_w, uint32_t tile_h, float rec[10], uint32_t* quadrant_mask);
/* test hook, host only: the binning footprint of ONE splat (words 0..2 of its 20-B record: v1, v2, pos) -- the ids
 * (ty * ceil(viewport_w / tile_w) + tx) of the binning tiles its kept ellipse a <= 2*CUTOFF (gaussian.wgsl:40-64) can
 * reach, in the order the binning stage emits them; *count = their number (what K1 stores per splat), of which at most
 * `capacity` are written.  tile_w / tile_h: 16 or 32. */
int ws_debug_footprint(const uint32_t splat[3], float viewport_w, float viewport_h, uint32_t tile_w, uint32_t tile_h,
                       uint32_t capacity, uint32_t* tiles, uint32_t* count);
/* test hooks, host only: (1) the packed tile rectangle a splat carries through the depth sort (x0 | y0 << 8 | (w - 1) << 16 |
 * (h - 1) << 24 in compositing tiles, 0xFFFFFFFF = lists no tile): the number of tiles it lists at the compositing tile and
 * at 2 x 2 of them, and the same rectangle in units of 2 x 2 tiles -- the arithmetic K1, k_bin_prefix and k_bin_emit share;
 * (2) the frame's binning decision from K1's per-slot sums of those two counts (request: 0 = never coarse, 1 = decide,
 * 2 = always; nslots <= 16): *shift = 0 (lists per compositing tile) or 1 (per 2 x 2 of them). */
int ws_debug_packed_rect(uint32_t rect, uint32_t* tiles, uint32_t* tiles_coarse, uint32_t* rect_coarse);
int ws_debug_binning_decision(uint32_t request, const uint32_t* sums, const uint32_t* sums_coarse, uint32_t nslots,
                              uint32_t* shift);
/* host twin of the depth sort's range decision (ws_internal.h depth_range_decide; CPU unit test, not on any render path): from the
 * frame's smallest and largest depth key and the radix (256 | 512) -> the base the passes behind the first subtract, whether the
 * fourth pass is the identity (skip), and the span class the next frame's digit width is chosen by (0 unknown, 1 = < 2^24, 2 = not) */
int ws_debug_depth_range(uint32_t key_min, uint32_t key_max, int have_keys, uint32_t digits, uint32_t* base, uint32_t* skip,
                         uint32_t* span_class);
/* host twin of the whole fold (CPU unit test): keys[0, count) in sort tiles of tile_n keys, each tile reported by the rule the
 * depth sort's first histogram kernels share (ws_internal.h depth_tile_reports) into slot t & 15, then depth_range_decide ->
 * the same (base, skip, span_class) as ws_debug_depth_range gives from the keys' true min and max. */
int ws_debug_depth_fold(const uint32_t* keys, uint32_t count, uint32_t tile_n, uint32_t digits, uint32_t* base, uint32_t* skip,
                        uint32_t* span_class);
/* what the device decided in the last ws_sorter_sort_depth of this sorter (syncs on that call's stream): the base of passes
 * 1..3, whether the fourth pass was skipped, the span class.  WS_ERR_STATE when that call did not fold its key range (the
 * context's depth_skip_top is 0, the fat-tile form ran, or the sorter's last sort was not a ws_sorter_sort_depth). */
int ws_sorter_depth_range(ws_sorter* s, uint32_t* base, uint32_t* skip, uint32_t* span_class);
/* tuning / analysis read-back: per tile LIST (one per binning tile, ws_renderer_binning_tile; row-major over
 * ceil(viewport / binning tile)), the length of the depth-ordered splat list and (capture mode, where the binning tile is
 * the compositing tile) how deep into it the compositing pass read: the position, counted from the near end, of the deepest
 * entry any of the tile's waves composited before its pixels were saturated.  Syncs. */
int ws_renderer_download_tile_stats(ws_renderer* r, uint32_t capacity, uint32_t* list_len, uint32_t* consumed,
                                    uint32_t* num_tiles);
/* analysis read-back (capture mode): walked[t * 17 + w] = staged records wave w of tile t composited (w < waves
 * per tile, 16 at the default tile), walked[t * 17 + 16] = sum over the tile's batches of the most any of its waves
 * composited in that batch -- the lock-step cost of the per-batch barriers.  Syncs. */
int ws_renderer_download_wave_stats(ws_renderer* r, uint32_t tile_capacity, uint32_t* walked);
/* analysis / parity read-back of the compositing schedule: up to 4096 tiles (1080p class) the compositing workgroups of a
 * renderer that draws one frame at a time (not a slot of a view batch with several slots, and its context's last prepare()
 * calls all on one stream) run longest list first (one small kernel behind the tile-id sort orders them; the image does not depend on the order).
 * order4[4 * b + 0..3] = (tx | ty << 16, begin, end, 0) for workgroup b: the blend tile it composites and that tile's entry
 * range; 0xFFFFFFFF in word 0 = no tile.  *num_blocks = 0 when the last prepared frame was not ordered (4K-class tile
 * counts, non-default tile shapes, WS_BLEND_ORDER=0).  Syncs. */
int ws_renderer_download_blend_order(ws_renderer* r, uint32_t capacity_blocks, uint32_t* order4, uint32_t* num_blocks);
/* analysis: the next render() launches the time-stamped build of the compositing kernel (production form: 32x32 tiles,
 * rgba32float target, the frame's own binning) and every wave of every tile leaves 16 words: cycles (shader clock) spent in
 * [0] the tile-range load, [1] the first batch's dependent gather chain, [2] later batches' gather waits, [3] decode,
 * [4] the staging barrier, [5] compaction, [6] the walk, [7] the end-of-batch vote, [8] the pixel store; [9] batches,
 * [10] records walked, [11] / [12] shader-clock stamps at start / end, [13] / [14] the 100-MHz clock at start / end,
 * [15] XCC id << 28 | HW_ID.  The counterpart of the reference's GPUStopwatch (utils.rs:26-134) below kernel granularity.
 * times[(t * 16 + w) * 16 + k] for blend tile t (row-major), wave w.  Syncs. */
int ws_renderer_enable_blend_timing(ws_renderer* r, int enable);
int ws_renderer_download_blend_timing(ws_renderer* r, uint32_t tile_capacity, uint32_t* times, uint32_t* num_tiles);
/* parity read-back of the binning result: binning tile t's depth-ordered (far -> near) splat list is
 * entries[begin[t] .. end[t]) (store indices, as `sorted` of ws_renderer_download_frame); t is row-major over
 * ceil(viewport / binning tile) (ws_renderer_binning_tile; the tile count comes from ws_renderer_download_tile_stats).
 * Any pointer may be NULL; *num_entries = D.  Syncs. */
int ws_renderer_download_tile_lists(ws_renderer* r, uint32_t tile_capacity, uint32_t* begin, uint32_t* end,
                                    uint32_t entry_capacity, uint32_t* entries, uint32_t* num_entries);

/* ---- Scene: scene.rs:13-24, 113-194 (host only) ----------------------------------------------------- */
#define WS_SPLIT_ALL (-1)
#define WS_SPLIT_TRAIN 0 /* scene.rs:63-67 Split::Train */
#define WS_SPLIT_TEST 1  /* Split::Test: every 8th camera of the file (scene.rs:143-151) */
typedef struct ws_scene ws_scene; /* scene.rs:113-118 Scene */
/* scene.rs:13-24 SceneCamera; rotation = the 3 rows of cameras.json's 3x3 (camera-to-world) */
typedef struct ws_scene_camera {
    uint32_t id;
    char img_name[128];
    uint32_t width, height;
    float position[3];
    float rotation[9];
    float fx, fy;
    int32_t split;
} ws_scene_camera;
int ws_scene_load_json(const char* path, ws_scene** out);                        /* Scene::from_json */
int ws_scene_from_json_text(const char* text, size_t len, ws_scene** out);
void ws_scene_destroy(ws_scene* s);
uint32_t ws_scene_num_cameras(const ws_scene* s);
float ws_scene_extend(const ws_scene* s);                                        /* max camera-to-camera distance */
/* Scene::cameras(split), sorted by id; returns the number of matching cameras, fills at most `capacity` */
uint32_t ws_scene_cameras(const ws_scene* s, int split, uint32_t capacity, ws_scene_camera* out);
int ws_scene_get_camera(const ws_scene* s, uint32_t id, ws_scene_camera* out);   /* Scene::camera; 1 if Some */
int ws_scene_nearest_camera(const ws_scene* s, const float pos[3], int split, uint32_t* id); /* 1 if Some */

/* ---- offline front-ends: bin/render.rs, bin/measure.rs, renderer.rs:417-583 Display ------------------- */
/* bin/render.rs:187-246 download_texture: device image (format of the renderer) -> host RGBA8, each channel
 * clamp(v, 0, 1) * 255 TRUNCATED (`as u8`); a NaN channel stores 0 (Rust's saturating cast), +-inf clamp to 0 / 255; unorm8
 * images are copied. out = width*height*4 bytes. Syncs. */
int ws_download_texture_rgba8(ws_context* ctx, const void* d_image, ws_color_format format, uint32_t width,
                              uint32_t height, size_t row_pitch_bytes, uint8_t* out, void* stream);
/* `image` crate save (bin/render.rs:127): RGBA8 PNG */
int ws_png_write_rgba8(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba, size_t row_stride_bytes);
/* bin/render.rs:33-128 render_views: every camera of `split` (sorted by id) at its own resolution capped to 1600 px
 * wide (height rescaled with truncation), Rgba16Float target cleared to TRANSPARENT, fit_near_far, walltime 100 s,
 * max_sh_deg = pc.sh_deg  ->  <out_dir>/<train|test>/<index:05>.png.  *rendered = images written. */
int ws_render_views(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const char* out_dir,
                    uint32_t* rendered);
/* bin/measure.rs:27-154 render_views: 2048x2048 Rgba8Unorm target, one warm-up frame of camera 0, then num_samples
 * (reference: 10) frames of every TRAIN camera back to back, one sync; *fps = 1 / (elapsed / (cameras*num_samples))
 * with the clock started BEFORE the warm-up frame, as the reference does.  frames_in_flight > 1 (not in the
 * reference) gives every in-flight frame its own renderer scratch, target and HIP stream. */
int ws_measure(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, uint32_t num_samples,
               uint32_t frames_in_flight, float* fps);
/* ---- Per-Gaussian contributions over frames, and pruned point clouds (no counterpart in the reference) ----------------------
 * What each Gaussian of the resident scene did to the frames added to an accumulator.  For a prepared frame and a pixel p of
 * the viewport, p's tile list is walked near to far.  A pair (splat i, p) is kept iff a' <= the cut-off on the tile-local
 * affine form -- the FAST blend's rule, whatever the renderer's blend mode, background, target, occluder or planes.  Its
 * weight is w = b * T, b = min(0.99, 2^-a' * alpha_i) in f32, T the running f32 transmittance (1 at the start, T <- T - w).
 * As in the FAST blend an 8x8-px quadrant may stop once all of its pixels have T < 2^-14: every pair left out weighs less
 * than 2^-14, and together they weigh at most the pixel's remaining T.  Per source Gaussian j (its index in the point cloud):
 *   sum_q32[j]    (u64) sum over kept pairs of (uint64_t)(w * 2^32); sum_q32 / WS_CONTRIB_SUM_SCALE = sum of weights
 *   max_weight[j] (f32) the largest w of any pair
 * over every frame added since creation / the last reset.  Both are integer reductions (the max on the bits of a non-negative
 * float): bitwise reproducible for the same frames and context configuration, and accumulators of disjoint camera subsets
 * (ranks) add exactly (ws_contrib_add).  The tile-local arithmetic depends on the tile origin: contexts of different tile
 * shapes need not agree to the bit.
 * ws_renderer_enable_contrib(r, 1) before prepare(): K1 keeps the source index of every visible splat (4 B each); nothing else
 * of the frame changes -- every image and plane is bit-identical -- but, like capture mode, such a renderer does not replay a
 * captured frame graph.  ws_renderer_accumulate_contrib enqueues on `stream` behind the prepared frame (render() is not
 * needed) and makes no blend launch.
 * Errors: WS_ERR_INVALID for null handles, an accumulator and a point cloud of different sizes, capacity or n below
 * num_points, indices not strictly ascending or not below num_points, n == 0; WS_ERR_STATE when the frame is not prepared for
 * `pc` or was prepared with contributions off; WS_ERR_UNSUPPORTED in a context with debug_cut. */
typedef struct ws_contrib ws_contrib;   /* per-Gaussian accumulators for clouds of num_points Gaussians (device memory, zeroed) */
#define WS_CONTRIB_SUM_SCALE 4294967296.0 /* sum_q32 / scale = sum of weights */
int  ws_contrib_create(ws_context* ctx, uint32_t num_points, ws_contrib** out);
void ws_contrib_destroy(ws_contrib* c);
int  ws_contrib_reset(ws_contrib* c, void* stream);
uint32_t ws_contrib_num_points(const ws_contrib* c);
uint32_t ws_contrib_frames(const ws_contrib* c);              /* frames added since creation / reset (host counter) */
int  ws_renderer_enable_contrib(ws_renderer* r, int enable);  /* before prepare(): K1 keeps source indices (4 B per visible splat) */
int  ws_renderer_accumulate_contrib(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, void* stream); /* enqueues; after prepare(), render() not needed */
int  ws_contrib_download(ws_contrib* c, uint32_t capacity, uint64_t* sum_q32, float* max_weight);          /* either may be NULL; syncs */
int  ws_contrib_add(ws_contrib* c, const uint64_t* sum_q32, const float* max_weight, uint32_t n);          /* host arrays of another accumulator / rank: exact merge */
/* The Gaussians indices[0..n) of `src` (strictly ascending) as a point cloud of its own, gathered on the device: the 16-B
 * chunks of every plane, or the 24-B compressed records with the SH / covariance codebooks and the quantisation block copied
 * whole.  The relative order is kept (K1's store order and the stable sort's ties are the parent's); bbox, centre, up, the
 * mip / kernel-size / background metadata and sh_deg are inherited verbatim, so fit_near_far, the settings uniform and the
 * depth keys of the surviving splats stay bit-identical.  The subset owns its memory: `src` may be destroyed first. */
int  ws_pointcloud_create_subset(ws_context* ctx, const ws_pointcloud* src, const uint32_t* indices, uint32_t n, ws_pointcloud** out);
/* Every camera of `split` (sorted by id) added to `c`, set up exactly as ws_render_views does (1600-px cap, fit_near_far,
 * walltime 100 s, max_sh_deg = pc.sh_deg): one renderer, one stream, one sync at the end, no target and no blend launch.
 * *frames = cameras added.  WS_ERR_OVERFLOW when a frame overflowed its tile-entry list (read once, after the sync): the
 * accumulator is then incomplete.  (Every ws_scene_* driver and ws_render_views walk their cameras with one function and size
 * their frames by one rule, csrc/scene_frames.h; a camera with an empty image is WS_ERR_INVALID before the first frame.) */
int  ws_scene_accumulate_contrib(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, ws_contrib* c, uint32_t* frames);
/* ---- Attributing a pixel plane to Gaussians: weighted contribution sums (no counterpart in the reference) ---------------------
 * (Declared behind "Image metrics" below, whose types they use; this is the normative text.)
 * ws_renderer_accumulate_weighted is ws_renderer_accumulate_contrib with every weight multiplied by a per-pixel value E(p) of a
 * caller-supplied f32 plane over the prepared frame's viewport: for every Gaussian j, the sum over its kept (pixel, splat)
 * pairs of w * E(p).  E == 1 gives the contribution sum; E an error map gives blame (sum / plain sum = the mean error under the
 * Gaussian); E a 0/1 mask gives a visibility-weighted selection.  To the bit:
 *   the kept pairs, b, w = b * T, T <- T - w, the quadrant's stop at T < 2^-14 and everything else that decides which pairs are
 *     walked are EXACTLY those of ws_renderer_accumulate_contrib: the plane never influences them;
 *   E(p) = min(max(fma(scale, plane[p], bias), 0), 1) in f32 (one fused multiply-add), NaN -> 0; read once per pixel; nothing
 *     past a row's width-th value is read (rows may be padded with anything);
 *   v = w * E, one rounded f32 multiply;
 *   sum_q32[j] += (uint64_t)(v * 2^32) (truncation);  max_weight[j] = max(max_weight[j], v) over pairs whose q32 is not 0.
 * The results land in an ordinary ws_contrib -- integer reductions, bitwise reproducible, mergeable with ws_contrib_add -- and
 * the call counts as a frame of it.  For two planes with E_A + E_B == 1 at every pixel where each is 0 or 1 (a mask and its
 * complement) the two sums add up to the plain sum exactly.  An 8x8-px quadrant whose 64 values of E are all 0 is not walked
 * (it can add nothing), which is what makes a small mask cheap; no result depends on it.
 * scale / bias exist so that a plane can be used as it is produced: ws_metrics_add's SSIM map through scale -0.5, bias 0.5 is
 * DSSIM = (1 - ssim) / 2 in [0, 1].
 * Errors: state and size errors as ws_renderer_accumulate_contrib; WS_ERR_INVALID for a null view or d_values, a row pitch
 * below 4 * width or not a multiple of 4, a pointer not 4-B aligned, a non-finite scale or bias.
 * ws_image_error_plane: a per-pixel error plane of two resident images of one size, one thread per pixel (enqueues only).
 * Both images give their PIXEL VALUE exactly as "Image metrics" defines it (decode, over_background, clamp, and
 * WS_METRICS_QUANTIZE_U8 in `flags`); per colour channel d = x - y, e = d * d (WS_ERROR_SQ) or |d| (WS_ERROR_ABS);
 * plane[p] = ((e_r + e_g) + e_b) / 3.0f, every operation a separately rounded f32 one.  The SQ plane's mean is the pair's mse.
 * Errors: those of ws_metrics_add for the views, sizes and flags; WS_ERR_INVALID for a null plane, a plane pitch below
 * 4 * width or not a multiple of 4, a misaligned plane pointer, an unknown kind (WS_ERROR_DSSIM included: it has no kernel).
 * ws_scene_accumulate_error: every camera of `split` (sorted by id) blamed on the Gaussians of `pc`.  Exactly one of ref_pc /
 * gt_dir; cameras, frame sizes, targets, blend mode, background and PNG handling are exactly those of ws_scene_evaluate (one
 * walk serves every scene driver).  Per camera: prepare with contributions enabled and render `pc` (image a); image b is the
 * render of `ref_pc` (by a second renderer, as in ws_scene_evaluate) or the PNG; the error plane is ws_image_error_plane's,
 * or for WS_ERROR_DSSIM the SSIM map of a private one-slot ws_metrics through scale -0.5, bias 0.5; the weighted sum is added
 * to `err` and, if `weight` is not NULL, the plain contribution sum of the same prepared frame to `weight`.  One stream, one
 * sync at the end (gt_dir: the upload of every PNG waits for the frame before it, as in ws_scene_evaluate).  *frames =
 * cameras added.  WS_ERR_OVERFLOW when a frame overflowed its tile-entry list (read once, after the sync): the accumulators
 * are then incomplete -- there is no second run, an accumulator cannot be rolled back (ws_scene_accumulate_contrib's rule).
 * WS_ERR_INVALID for null handles, accumulators of another size than `pc`, an unknown kind, split or flag bit, both or neither
 * of ref_pc / gt_dir; WS_ERR_IO naming the file for a PNG that cannot be opened. */
/* ---- Image metrics: PSNR and SSIM between two resident images (no counterpart in the reference) ------------------------------
 * The two figures every 3DGS evaluation reports, as the INRIA / c3dgs metrics.py defines them, computed on the device between
 * two images of one size, per image pair.  The definition is bit-level up to the sums:
 * PIXEL VALUE of an image view (pointer, ws_color_format, row pitch) at (x, y), per colour channel ch:
 *   (r, g, b, a) decoded as ws_display_composite decodes: f32 as stored, f16 -> f32, unorm8 as (float)k / 255.0f;
 *   over_background != 0:  k = 1 - a;  t = background[ch] * k;  v = c_ch + t   -- three separately rounded f32 operations,
 *                          no fused multiply-add (the premultiplied texel over an opaque background);
 *   over_background == 0:  v = c_ch, alpha is ignored;
 *   v = min(max(v, 0), 1), NaN -> 0;
 *   WS_METRICS_QUANTIZE_U8:  q = (uint8_t)(v * 255.0f) (truncation, ws_download_texture_rgba8's rule), v = (float)q / 255.0f:
 *                          the metric of the PNG ws_render_views would have written.
 * MSE / PSNR: d = x - y and e = d * d in f32; mse = sum(e) / (3 W H) over the three colour channels, the sum taken in f64;
 *   psnr = -10 log10(mse) in double on the host, +inf when mse == 0.  With WS_METRICS_QUANTIZE_U8 the record also carries
 *   sse_u8 = sum (qx - qy)^2, an exact integer (at most 65025 * 3 W H), and mse = sse_u8 / (255^2 * 3 W H) in double.
 * SSIM (the 3DGS `ssim`): per colour channel, an 11-tap window g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in
 *   double and rounded to f32 -- g[0..5] = 0x1.0d956cp-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c4p-3,
 *   0x1.10656p-2, g[10 - k] = g[k] -- the 2-D window their outer product; ZERO padding of 5 pixels (a tap outside the image
 *   adds 0 to every moment); moments mu_x, mu_y, E[x^2], E[y^2], E[xy]; s_x = E[x^2] - mu_x^2, s_y likewise, s_xy = E[xy] -
 *   mu_x mu_y; C1 = 0.01^2, C2 = 0.03^2;
 *     ssim_map = ((2 mu_x mu_y + C1) (2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1) (s_x + s_y + C2)),
 *   ssim = its mean over 3 W H.  The moments and the map are evaluated in f64 on the f32 pixel values.  d_ssim_map (optional):
 *   an f32 W x H plane of (map_r + map_g + map_b) / 3, rounded once -- the error heat map.
 * Reduction: fixed-order sums per workgroup, one partial record each, summed in index order by a second kernel; no float
 * atomics: the same pair gives the same bits, whatever else the accumulator holds.
 * An accumulator holds the records of up to max_images comparisons, in ws_metrics_add order.  ws_metrics_add only ENQUEUES on
 * `stream` (the images must stay valid and unchanged until that work is done); ws_metrics_download syncs and finalises mse,
 * psnr and ssim on the host.  ONE ACCUMULATOR IS USED FROM ONE STREAM AT A TIME (its partial-record slab is shared by its adds
 * and grown at add): sync before moving it to another stream.
 * Image pointers and pitches must be multiples of the texel size (4 / 8 / 16 B); the map's of 4.  Rows may be padded with
 * anything: nothing past a row's last texel is read.
 * Errors: WS_ERR_INVALID for null handles (refused before anything touches a device), zero sizes, a pitch below the row or
 * misaligned, an unknown format or flag bit, capacity < count; WS_ERR_OVERFLOW when the accumulator is full (its records stay). */
typedef struct ws_image_view {
    const void* d_pixels;       /* device memory */
    ws_color_format format;
    size_t row_pitch_bytes;
    int32_t over_background;    /* 0: the colour channels as stored; 1: premultiplied over background[] */
    float background[3];
} ws_image_view;
typedef struct ws_image_metrics {
    double mse, psnr, ssim;
    uint64_t sse_u8;            /* WS_METRICS_QUANTIZE_U8 only, else 0 */
    uint32_t width, height, flags, reserved;
} ws_image_metrics;
typedef struct ws_metrics ws_metrics;   /* per-image records of up to max_images comparisons (device memory) */
#define WS_METRICS_QUANTIZE_U8 1u
int  ws_metrics_create(ws_context* ctx, uint32_t max_images, ws_metrics** out);
void ws_metrics_destroy(ws_metrics* m);
int  ws_metrics_reset(ws_metrics* m, void* stream);
uint32_t ws_metrics_count(const ws_metrics* m);               /* images added since creation / reset (host counter) */
int  ws_metrics_add(ws_metrics* m, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, uint32_t flags,
                    float* d_ssim_map /* may be NULL */, size_t map_pitch_bytes, void* stream);                  /* enqueues only */
int  ws_metrics_download(ws_metrics* m, uint32_t capacity, ws_image_metrics* out, uint32_t* count);            /* syncs */
/* An 8-bit PNG decoded to RGBA8 on the host: greyscale, grey + alpha, RGB or RGBA, non-interlaced, all five filter types; grey
 * is replicated, a missing alpha is 255.  *rgba is width * height * 4 bytes, released with ws_host_free.  Chunk CRCs and sizes
 * are checked: a damaged file is WS_ERR_IO; 16-bit, palette and interlaced files are WS_ERR_UNSUPPORTED. */
int  ws_png_read_rgba8(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgba);
void ws_host_free(void* p);
/* Every camera of `split` (WS_SPLIT_TRAIN, WS_SPLIT_TEST or WS_SPLIT_ALL; sorted by id) adds one record to `m`; *frames =
 * cameras added.  Exactly one of ref_pc / gt_dir:
 *   ref_pc (the prune check): each camera set up exactly as ws_render_views sets it up (1600-px cap, fit_near_far, walltime
 *     100 s, Rgba16Float targets cleared to transparent, the context's render-views blend mode), rendered once from `pc`
 *     (image a) and once from `ref_pc` (image b); both are compared over the background colour of `pc`, or black when it has
 *     none.  One stream, one sync at the end, no image read-back; if a frame overflowed its tile-entry list the entry lists
 *     are grown and the whole split runs again (at most twice), else WS_ERR_OVERFLOW.
 *   gt_dir (ground truth): image b is <gt_dir>/<img_name>, ".png" appended unless the name ends in it (any case), read with
 *     ws_png_read_rgba8 and taken as opaque unorm8.  There is no resampler: the frame is rendered at the PNG's own size, with
 *     the field of view of the camera's own fx, fy, width, height.  |png_w * cam_h - png_h * cam_w| > max(cam_w, cam_h) is an
 *     aspect mismatch: WS_ERR_INVALID, naming the file; a file that cannot be opened is WS_ERR_IO, naming it.  JPEG is out of
 *     scope.
 * flags: WS_METRICS_QUANTIZE_U8 or 0.  On an error `m` keeps the records it had before the call. */
int  ws_scene_evaluate(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                       const char* gt_dir, uint32_t flags, ws_metrics* m, uint32_t* frames);
/* "Attributing a pixel plane to Gaussians" (the text is above "Image metrics") */
typedef struct ws_plane_view {
    const float* d_values;      /* device memory: one f32 per viewport pixel */
    size_t row_pitch_bytes;
    float scale, bias;          /* E = clamp(scale * value + bias, 0, 1) */
} ws_plane_view;
int  ws_renderer_accumulate_weighted(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, const ws_plane_view* plane, void* stream); /* enqueues; counts as a frame of c */
#define WS_ERROR_SQ  0
#define WS_ERROR_ABS 1
int  ws_image_error_plane(ws_context* ctx, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, int kind,
                          uint32_t flags, float* d_plane, size_t plane_pitch_bytes, void* stream);                  /* enqueues only */
#define WS_ERROR_DSSIM 2   /* scene driver only: ws_metrics_add's map through scale -0.5, bias 0.5 */
int  ws_scene_accumulate_error(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                               const char* gt_dir, int kind, uint32_t flags, ws_contrib* err, ws_contrib* weight /* may be NULL */,
                               uint32_t* frames);
/* ---- Rendering per-Gaussian values to pixel planes, and the winner-id plane (no counterpart in the reference) ------------------
 * The operator the two attribution passes above are the transpose of.  For a prepared frame and a caller's f32 values f[j][c]
 * over the Gaussians of the point cloud (c < channels <= 4), per viewport pixel p
 *   plane[c](p) = sum over the kept pairs (p, i), near to far, of w_i(p) * f[src(i)][c]
 *   winner(p)   = src(i) of the kept pair with the largest w_i(p), 0xFFFFFFFF when no pair has w > 0
 * with the pairs, the weights w and src(i) -- the index in the point cloud of splat i -- EXACTLY those of "Per-Gaussian
 * contributions" above: whatever ws_renderer_accumulate_contrib sums for a frame in a context, this call draws.  So a blame
 * score, a contribution sum, a keep / drop mask or a label per Gaussian becomes an image, and winner answers "which Gaussian is
 * under this pixel".  To the bit:
 *   the kept pairs, b, w = b * T, T <- T - w, the quadrant's stop at T < 2^-14 and everything else that decides which pairs are
 *     walked are those of ws_renderer_accumulate_contrib in the same context; the values never influence them;
 *   per pixel and channel acc = 0, and per kept pair in near-to-far order acc = fma(w, f[src][c], acc) in f32 (one fused
 *     multiply-add); a pair that is not kept multiplies nothing, so a non-finite f[j] reaches only pixels Gaussian j reaches;
 *   winner: best_w = 0, best = 0xFFFFFFFF, and per kept pair  if (w > best_w) { best_w = w; best = src; }  -- strict, so of
 *     equal weights the nearest wins and a weight of 0 never does;
 *   every pixel of the viewport of every plane asked for is written, 0.0f / 0xFFFFFFFF where nothing is listed; nothing past a
 *     row's width-th value is written, nothing is read from the planes.
 * Consequences that hold bitwise: for f one-hot at j (1.0f at j, 0.0f elsewhere) the plane holds j's weights themselves, so
 * sum over p of (uint64_t)(plane(p) * 2^32) == sum_q32[j] and the largest value whose q32 is not 0 == max_weight[j] of
 * ws_renderer_accumulate_contrib on the same frame; channels are independent of each other and of the stride; f scaled by a
 * power of two scales the plane by it.  No normalisation: a channel of ones (= 1 - T, ws_renderer_render_aux's alpha up to
 * rounding) is the normaliser.
 * The call enqueues on `stream` behind the prepared frame (render() is not needed), makes no blend launch and changes no pixel
 * of any target.  `values` may be NULL when only winner is asked for.
 * Errors: WS_ERR_INVALID for null handles or targets, no output at all, channels of 0 or above 4, a plane that is not NULL at
 * c >= channels, a stride below 4 * channels or a pitch below 4 * width or either not a multiple of 4, a pointer not 4-B
 * aligned, num_points other than the point cloud's, a reserved word that is not 0 (all refused before anything touches a
 * device); WS_ERR_STATE when the frame is not prepared for `pc` or was prepared with contributions off; WS_ERR_UNSUPPORTED in
 * a context with debug_cut. */
typedef struct ws_values_view {
    const float* d_values;      /* device; value c of Gaussian j at (char*)d_values + j*stride_bytes + 4*c */
    size_t stride_bytes;        /* >= 4*channels, multiple of 4; 4-B aligned pointer */
    uint32_t num_points;        /* must equal the point cloud's */
    uint32_t channels;          /* 1..4 */
} ws_values_view;
typedef struct ws_value_targets {
    float* plane[4]; size_t pitch[4];     /* f32 per pixel; plane[c] may be NULL (not written); c >= channels must be NULL */
    uint32_t* winner; size_t winner_pitch;/* u32 per pixel or NULL */
    uint32_t reserved[4];                 /* zero */
} ws_value_targets;
int  ws_renderer_render_values(ws_renderer* r, const ws_pointcloud* pc, const ws_values_view* values /* may be NULL: winner only */,
                               const ws_value_targets* out, void* stream);                                        /* enqueues only */
/* ---- Removal effect: what deleting each Gaussian alone would do to the frames (no counterpart in the reference) ---------------
 * The contribution sum says how much a Gaussian drew, blame how much of a given error map lies under it; both are proxies for
 * the question a pruner asks.  This call answers it without a second image: per Gaussian j, the change of the frame itself if j
 * alone were deleted.  Call F the image the FAST blend's pairs produce over `background`.  With splat i taken out, every weight
 * behind it at pixel p grows by 1 / (1 - b_i) and everything in front stays; the pixel moves by
 *   D_i(p) = r_i * S_i(p) - w_i * c_i,   r_i = w_i / T_after_i = b_i / (1 - b_i),   S_i(p) = F(p) - P_i(p)
 * where P_i is the colour accumulated near to far through i, itself included: S_i is what lies behind i, background included,
 * and D_i = w_i * (B_i - c_i), the splat's weight times the difference between the normalised colour behind it and its own.
 * The form is exact, not first order, as long as no stop at T < 2^-14 intervenes.
 * Preconditions as for ws_renderer_accumulate_contrib: a prepared frame, ws_renderer_enable_contrib(r, 1) before prepare().
 * The call enqueues two launches on `stream` behind the prepared frame, makes no blend launch and changes no target.
 * PAIRS AND WEIGHTS.  The pairs walked, b, w = b * T, T <- T - w, the quadrant's stop and the batch loop's stop are exactly those
 * of "Per-Gaussian contributions" in the same context.  No argument of this call influences them.
 * PASS 1, THE BASE IMAGE, for every viewport pixel, empty tiles included.  acc_ch = 0; per kept pair, near to far,
 *   acc_ch = fma(w, c_ch, acc_ch)      one fused multiply-add; c_ch the f16 colour of the Splat record taken to f32;
 * at the end F_ch = fma(T_end, background_ch, acc_ch) and base(p) = (F_r, F_g, F_b, T_end) as one float4; (background, 1)
 * where nothing is listed.  With d_base it is written there -- the FAST image in f32 over that background, useful by itself;
 * nothing past a row's width-th float4 is written -- otherwise to renderer-owned scratch, grown on demand.
 * PASS 2, PER WALKED PAIR.  P_ch = 0 and a copy of T of its own (1; 0 outside the viewport), kept with the walk's arithmetic:
 *   Tb = T;  T = Tb - w                (w == 0 for a pair outside the cut-off)
 *   kept:  P_ch = fma(w, c_ch, P_ch)   the sequence of pass 1: P equals pass 1's acc at the last walked pair
 *   the pair COUNTS iff it is kept, w > 0 and Tb >= 2^-14: a pair at an already saturated pixel scores 0 whether or not its
 *     wave was still walking, and so does every pair at a pixel outside the viewport;
 *   r    = w / T                       IEEE division (T > 0: b <= 0.99)
 *   s_ch = F_ch - P_ch                 one rounded subtraction
 *   t_ch = w * c_ch                    one rounded multiply
 *   d_ch = fma(r, s_ch, -t_ch)         one fused multiply-add
 *   e_ch = d_ch * d_ch (WS_ERROR_SQ) or |d_ch| (WS_ERROR_ABS);  m = ((e_r + e_g) + e_b) / 3, each operation rounded by itself
 *   v    = min(scale * m, 0x1.fffffep-1f), NaN -> 0: one rounded multiply; the cap sits below 1 so that v * 2^32 fits 32 bits
 *   with a weight plane  v = v * E(p), one rounded multiply; E is formed exactly as ws_renderer_accumulate_weighted forms it
 *     (the same ws_plane_view: scale and bias in one fma, clamp to [0, 1], NaN -> 0, read once per pixel, nothing past a row's
 *     width-th value read).  A quadrant whose 64 values of E are all 0 is idle in pass 2; pass 1 is never idle.
 * ACCUMULATION.  sum_q32[j] += (uint64_t)(v * 2^32), truncating; max_weight[j] = max(max_weight[j], v) over pairs whose q32 is
 * not 0; both into an ordinary ws_contrib through the source index, and the call counts as a frame of it.  Integer reductions
 * as in ws_renderer_accumulate_contrib: bitwise reproducible, mergeable with ws_contrib_add, exact across ranks.  The pairs add
 * exactly: a 0/1 mask and its complement sum to the unweighted result bit for bit, and a plane with E == 1 everywhere equals
 * weight == NULL bit for bit.
 * THE STOPS.  In a frame where no stop occurs, sum[j] / scale with WS_ERROR_SQ is the sum over p of mean_ch (F_without_j - F)^2
 * up to f32 rounding: the squared error the frame would gain if j were deleted alone.  Where quadrants saturate, F is the FAST
 * blend's own image, which ignores what lies behind the stop: a deletion that would un-saturate a pixel is under-reported by at
 * most r * 2^-14 * colour per pair.
 * Out of scope: a per-Gaussian image of D, and the joint effect of deleting several Gaussians (it is not additive; the additive
 * first-order score is the opacity sum of "Gradients of an image loss" below).
 * Errors: state and size errors as ws_renderer_accumulate_contrib; WS_ERR_INVALID for null params, an unknown kind
 * (WS_ERROR_DSSIM included), a scale that is not finite and above 0, a non-finite background, a weight view with a null
 * d_values, a non-finite scale or bias, a pointer or pitch not a multiple of 4 or a pitch below 4 * width, a d_base or
 * base_pitch_bytes that is not a multiple of 16 or a pitch below 16 * width, a reserved word that is not 0.  Everything that can
 * be judged from the descriptor alone is refused before a handle is looked at.
 * ws_scene_accumulate_removal: every camera of `split` (sorted by id), set up exactly as ws_scene_accumulate_contrib sets it up
 * (the same walk over the cameras), over the cloud's own background colour, or black when it has none; the effect is added to
 * `effect` and, if `weight` is not NULL, the plain contribution sums of the same prepared frames to `weight`.  One renderer, one
 * stream, one sync at the end; *frames = cameras added; WS_ERR_OVERFLOW under ws_scene_accumulate_contrib's rule. */
typedef struct ws_removal_params {
    float background[3];            /* the frames are judged over this colour */
    int32_t kind;                   /* WS_ERROR_SQ | WS_ERROR_ABS */
    float scale;                    /* finite, > 0 */
    const ws_plane_view* weight;    /* may be NULL: E = 1 */
    float* d_base; size_t base_pitch_bytes;   /* may be NULL; float4 per pixel, 16-B aligned pointer and pitch >= 16 * width, multiple of 16 */
    uint32_t reserved[4];           /* zero */
} ws_removal_params;
int  ws_renderer_accumulate_removal(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, const ws_removal_params* p, void* stream); /* enqueues; counts as a frame of c */
int  ws_scene_accumulate_removal(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, int kind, float scale,
                                 ws_contrib* effect, ws_contrib* weight /* may be NULL: the plain contribution sums of the same frames */, uint32_t* frames);
/* ---- Gradients of an image loss: dL/d(colour) and dL/d(ln opacity) per Gaussian (no counterpart in the reference) --------------
 * What a refit of the colours and opacities of a (pruned) cloud needs.  The prepared frame is LINEAR in each splat's colour and
 * AFFINE in each splat's per-pixel opacity b_i(p): with F, T_end, w, r, D, P of "Removal effect",
 *   dF(p) / dc_i = w_i(p),     b_i * dF(p) / db_i = -D_i(p),     b_i * dT_end(p) / db_i = -r_i * T_end(p)
 * (taking b_i out moves the pixel by D_i = r_i S_i - w_i c_i, and F is affine in b_i, so D_i = -b_i dF/db_i; T_end carries the
 * factor 1 - b_i, and b_i / (1 - b_i) = r_i).  The caller supplies a plane g of one float4 per viewport pixel,
 *   g(p) = (dL/dF_r, dL/dF_g, dL/dF_b, dL/dT_end),   F and T_end those of "Removal effect", pass 1, over `background`,
 * and per source Gaussian j the call adds four sums over the pairs (p, i) with src(i) = j:
 *   colour[j][ch] += sum_p w_i(p) * G_ch(p)          ch = r, g, b: the loss's derivative with respect to an offset added to the
 *                                                    Gaussian's colour BEFORE K1's clamp at 0 (preprocess.wgsl:258): a pair whose
 *                                                    staged c_ch is exactly 0 adds nothing to channel ch
 *   opacity[j]    += -sum_p (G_r D_r + G_g D_g + G_b D_b + G_T r T_end(p))
 *                                                    the derivative with respect to ln of a common factor on every b_i(p) of the
 *                                                    Gaussian, dL/d ln(alpha); pairs whose b sits on the 0.99 clamp add nothing
 * Preconditions as for ws_renderer_accumulate_removal: a prepared frame, ws_renderer_enable_contrib(r, 1) before prepare().  The
 * call enqueues two launches on `stream` behind the prepared frame, makes no blend launch and changes no target.
 * PAIRS AND WEIGHTS.  The pairs walked, b, w = b * T, T <- T - w, the quadrant's stop and the batch loop's stop are exactly those
 * of "Per-Gaussian contributions" in the same context.  No argument of this call influences them.
 * THE PLANE.  G_k(p) = min(max(scale * g_k(p), -1), 1) in f32: one rounded multiply, NaN -> 0, read once per pixel as one 16-byte
 * load; nothing past a row's width-th float4 is read; scale is finite and > 0.  A quadrant whose 64 x 4 values of G are all 0 is
 * idle in pass 2; pass 1 is never idle.
 * PASS 1.  Removal's base image, unchanged (the same kernel): base(p) = (F_r, F_g, F_b, T_end), to d_base or to the renderer's
 * scratch, which the two calls share.
 * PASS 2, PER WALKED PAIR.  Tb, T, P_ch as "Removal effect" pass 2 keeps them: the same operations in the same order.  Then
 *   colour, per ch:  v_ch = w * G_ch, one rounded multiply; counted iff the pair is kept, w > 0 and c_ch > 0; |v_ch| < 1 (b <= 0.99)
 *   opacity:  counted iff the pair is kept, w > 0, Tb >= 2^-14 (removal's rule) and the pair is NOT CLAMPED; it is clamped iff
 *     w == 0x1.fae148p-1f * Tb (one rounded f32 multiply): the only way min(0.99, ...) shows in b * T
 *     r, s_ch, t_ch, d_ch exactly removal's
 *     a = G_r * d_r (rounded);  a = fma(G_g, d_g, a);  a = fma(G_b, d_b, a);  u = r * T_end (rounded);  a = fma(G_T, u, a)
 *     v_o = -min(max(opacity_scale * a, -0x1.fffffep-1f), 0x1.fffffep-1f), NaN -> 0; opacity_scale finite and > 0 (|d| can reach
 *     r * colour with r up to 99); the cap is removal's and silent, as there
 * every step a separately rounded f32 operation except the fused ones named.
 * ACCUMULATION.  q = (int64_t)(v * 2^32): the product is exact, |q| < 2^32, the conversion truncates TOWARD ZERO.  Four int64
 * sums per Gaussian, added through the source index; integer sums commute, so the result depends on the order of nothing:
 * bitwise reproducible, mergeable with ws_grad_add, exact across ranks.  sum / (2^32 * scale) is the colour gradient,
 * sum / (2^32 * scale * opacity_scale) the opacity gradient.  Bit for bit: (a) g and -g give exactly negated sums; (b) a plane
 * restricted to a 0/1 mask and to its complement add up to the whole; (c) with g = (E, 0, 0, 0), E in [0, 1], scale 1,
 * colour[j][r] equals sum_q32[j] of ws_renderer_accumulate_weighted with that E through scale 1, bias 0, for every Gaussian whose
 * red is above 0 in the frame -- with E == 1 everywhere, ws_renderer_accumulate_contrib's sum.
 * THE STOPS.  As "Removal effect": F ignores what lies behind a stop, so a pair's opacity term is under-reported by at most
 * r * 2^-14 * colour * |G|.
 * Elsewhere: the higher SH coefficients are "SH gradients" below, position and covariance "Geometry gradients" behind it, the
 * optimiser "Refitting colour and opacity", the writer "Saving a point cloud".
 * Errors: as ws_renderer_accumulate_removal, judged from the descriptor before a handle is looked at; in addition
 * WS_ERR_INVALID for a null d_grad, a gradient pointer or pitch that is not a multiple of 16, a pitch below 16 * width, a scale
 * or opacity_scale that is not finite and above 0.
 * ws_grad: four int64 sums per Gaussian in device memory, zeroed at creation and by ws_grad_reset; ws_grad_download syncs and
 * copies [num_points][4] (colour r, g, b; ln-opacity); ws_grad_add adds another accumulator's (or rank's) downloaded sums, exactly.
 * ws_image_error_gradient: kernel beside ws_image_error_plane's, one thread per pixel (enqueues only).  Both pixel values are as
 * "Image metrics" defines them, WS_METRICS_QUANTIZE_U8 is refused; per colour channel d = x - y, g = (2 * d) / 3.0f (WS_ERROR_SQ:
 * one rounded multiply, IEEE division) or copysign(1 / 3.0f, d), 0 at d == 0 (WS_ERROR_ABS); g = 0 where a's value before the
 * clamp lay outside [0, 1] or was NaN; the fourth component is 0.  So sum g * dx is the first-order change of the sum of
 * ws_image_error_plane's plane.  Image a may be the base plane itself: rgba32float, over_background = 0 (the alpha slot holds
 * T_end and is ignored).  d_grad: float4 per pixel, pointer and pitch multiples of 16, pitch >= 16 * width.
 * ws_scene_accumulate_gradient: cameras, image b and PNG handling exactly those of ws_scene_accumulate_error (the same walk
 * over the cameras); per camera: prepare, the base image over the cloud's background (black if none), ws_image_error_gradient(base, b),
 * accumulate.  One stream, one sync at the end; *frames = cameras added; WS_ERR_OVERFLOW under ws_scene_accumulate_contrib's rule. */
typedef struct ws_grad ws_grad;                 /* four int64 sums per Gaussian, device memory, zeroed */
#define WS_GRAD_CHANNELS 4                      /* colour r, g, b; ln-opacity */
#define WS_GRAD_SUM_SCALE 4294967296.0
int  ws_grad_create(ws_context* ctx, uint32_t num_points, ws_grad** out);
void ws_grad_destroy(ws_grad* g);
int  ws_grad_reset(ws_grad* g, void* stream);
uint32_t ws_grad_num_points(const ws_grad* g);
uint32_t ws_grad_frames(const ws_grad* g);
int  ws_grad_download(ws_grad* g, uint32_t capacity, int64_t* q32 /* [capacity][4] */);   /* syncs */
int  ws_grad_add(ws_grad* g, const int64_t* q32, uint32_t n);                             /* exact merge of another rank's */
typedef struct ws_gradient_params {
    float background[3]; float scale; float opacity_scale; uint32_t reserved0;   /* scales finite, > 0; reserved0 zero */
    const float* d_grad; size_t grad_pitch_bytes;      /* float4 per pixel, 16-B aligned pointer and pitch >= 16 * width, multiple of 16 */
    float* d_base; size_t base_pitch_bytes;            /* may be NULL, as ws_removal_params */
    uint32_t reserved[4];                              /* zero */
} ws_gradient_params;
int  ws_renderer_accumulate_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_grad* g, const ws_gradient_params* p, void* stream); /* enqueues; counts as a frame of g */
int  ws_image_error_gradient(ws_context* ctx, const ws_image_view* a, const ws_image_view* b, uint32_t width, uint32_t height, int kind,
                             uint32_t flags, float* d_grad, size_t grad_pitch_bytes, void* stream);
int  ws_scene_accumulate_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                  const char* gt_dir, int kind, float scale, float opacity_scale, ws_grad* grad, uint32_t* frames);
/* ---- SH gradients: dL/d(sh[k][ch]) per Gaussian and coefficient, and dL/d(ln opacity) (no counterpart in the reference) -----------
 * K1's colour is max(0, 0.5 + sum_k basis_k(dir) * sh[k][ch]) with dir the unit vector from the camera to the Gaussian, so
 *   dL/d sh[k][ch] = basis_k(dir) * dL/d colour[ch]
 * and dir depends on the frame: the product has to be taken per frame, before frames are summed -- a ws_grad summed over frames
 * cannot give it.  A ws_shgrad holds 3 * ncoef + 1 int64 sums per Gaussian, ncoef = (sh_deg + 1)^2: sh[j][k][ch] and opacity[j],
 * in device memory, zeroed at creation and by ws_shgrad_reset, and a per-frame scratch of four int64 per Gaussian laid out as a
 * ws_grad.  DEVICE LAYOUT: one plane per element, [3 * ncoef + 1][num_points] (element 3 k + ch, the opacity's last), so that a
 * wave's accesses are contiguous in the Gaussian index; ws_shgrad_download transposes to q_sh[capacity][ncoef][3] and
 * q_opacity[capacity] (either may be NULL; syncs), ws_shgrad_add takes the same two arrays (either may be NULL) and is the exact
 * merge of another accumulator's or rank's sums.
 * ws_renderer_accumulate_sh_gradient: preconditions, descriptor and descriptor checks exactly those of
 * ws_renderer_accumulate_gradient; in addition WS_ERR_INVALID for a ws_shgrad of another size or one whose sh_deg is not the
 * cloud's, WS_ERR_UNSUPPORTED for a compressed cloud.  It enqueues three launches: k_removal_base, unchanged; k_gradient,
 * unchanged, into the accumulator's scratch; k_sh_spread, one thread per Gaussian j, no atomics (a Gaussian belongs to one thread;
 * frames are ordered by the stream):
 *   q_r, q_g, q_b, q_o = the four scratch sums of j.  All four 0 (culled or unseen, the common case): nothing else of j is read
 *   or written.  Otherwise the scratch row is zeroed again (the next frame starts clean without a memset) and
 *     opacity[j] += q_o;   sh[j][0][ch] += q_ch     the plain colour sum: the factor C0 stays in the refit step, as it is there
 *     sh[j][k][ch] += llrint((double)q_ch * (double)basis_k)    1 <= k < (min(max_sh_deg of the prepared frame, sh_deg) + 1)^2
 *   int64 -> double, the product and double -> int64 each round to nearest even; a q_ch of 0 and a basis that is not finite add
 *   nothing; coefficients above the frame's degree are not touched.
 * THE DIRECTION, TO THE BIT.  x, y, z the three f32 of plane 0, cam = view_inv[12..14] of the prepared frame's ws_camera_uniform,
 * d = xyz - cam, dl = sqrtf((dx * dx + dy * dy) + dz * dz), dir = d / dl, every operation a separately rounded IEEE f32 operation.
 * That is K1's default arithmetic, NOT the fast rsq path a library built with WS_K1_STRICT=0 takes.  dl == 0 and a non-finite
 * position give no finite basis: such a Gaussian gets its opacity and DC sums only.
 * THE BASIS.  bas[1..15] by the expressions of K1's SH evaluation (preprocess.wgsl:124-154) in its order, with (x, y, z) = dir:
 *   -C1 y, C1 z, C1 x | C2_0 xy, C2_1 yz, C2_2 (2 zz - xx - yy), C2_3 xz, C2_4 (xx - yy) | C3_0 y (3 xx - yy), C3_1 xy z,
 *   C3_2 y (4 zz - xx - yy), C3_3 z (2 zz - 3 xx - 3 yy), C3_4 x (4 zz - xx - yy), C3_5 z (xx - yy), C3_6 x (xx - 3 yy)
 * each product and difference evaluated left to right in f32.  K1 SUBTRACTS the term of coefficient 3: its effective basis is
 * -bas[3].  Every basis is bounded by 1 on unit directions, so no sum overflows that a ws_grad's would not.
 * THE CLAMP at 0 is honoured already: k_gradient counts no pair whose staged c_ch is 0.
 * Bit for bit: (a) q_sh[:, 0, :] and q_opacity equal the ws_grad of ws_renderer_accumulate_gradient with the same arguments;
 * (b) two frames added equal the sum of the two single-frame downloads; (c) g and -g negate every sum; (d) the result does not
 * depend on the launch geometry.
 * ws_sh_spread_rows (host only, no device needed): the per-Gaussian code of k_sh_spread from the same text, over n rows --
 * q4[n][4] one frame's ws_grad-layout sums, xyz[n][3], cam[3]; ADDS to q_sh[n][ncoef][3] and q_opacity[n] (either may be NULL)
 * with active_deg in the place of the prepared frame's max_sh_deg.
 * ws_scene_accumulate_sh_gradient: ws_scene_accumulate_gradient's walk over the cameras with this per-frame call.
 * The optimiser is ws_refit_step_sh ("Refitting colour and opacity" below); gradients with respect to position and covariance are
 * "Geometry gradients" below.  Out of scope: compressed clouds; a float or compacted accumulator. */
typedef struct ws_shgrad ws_shgrad;             /* 3 (sh_deg + 1)^2 + 1 int64 sums per Gaussian, device memory, zeroed */
int  ws_shgrad_create(ws_context* ctx, uint32_t num_points, uint32_t sh_deg, ws_shgrad** out);
void ws_shgrad_destroy(ws_shgrad* g);
int  ws_shgrad_reset(ws_shgrad* g, void* stream);
uint32_t ws_shgrad_num_points(const ws_shgrad* g);
uint32_t ws_shgrad_sh_deg(const ws_shgrad* g);
uint32_t ws_shgrad_frames(const ws_shgrad* g);
int  ws_shgrad_download(ws_shgrad* g, uint32_t capacity, int64_t* q_sh /* [capacity][ncoef][3] */, int64_t* q_opacity /* [capacity] */);   /* syncs */
int  ws_shgrad_add(ws_shgrad* g, const int64_t* q_sh, const int64_t* q_opacity, uint32_t n);   /* exact merge of another rank's */
int  ws_renderer_accumulate_sh_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_shgrad* g, const ws_gradient_params* p, void* stream); /* enqueues; counts as a frame of g */
int  ws_sh_spread_rows(const int64_t* q4, const float* xyz, const float* cam, uint32_t n, uint32_t sh_deg, uint32_t active_deg,
                       int64_t* q_sh, int64_t* q_opacity);
int  ws_scene_accumulate_sh_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                     const char* gt_dir, int kind, float scale, float opacity_scale, ws_shgrad* grad, uint32_t* frames);
/* ---- Geometry gradients: dL/d(position) and dL/d(covariance) per Gaussian (no counterpart in the reference) ----------------------
 * The part of a 3DGS parameter set "Gradients of an image loss" and "SH gradients" leave out, and the densification statistic of
 * the INRIA trainer.  The blend evaluates b = min(0.99, alpha * 2^(-a')), a' = p0^2 + p1^2, p = I' (x - mu), with I' the 2 x 2 map
 * and mu the pixel centre the blend decodes from the 20-B Splat record: I'^T I' = (log2 e / 2) Sigma^-1, Sigma = (v1 v1^T + v2
 * v2^T) / 2 in px^2; a pair is kept iff a' <= CUT_A2 (about 6.8), so |p|^2 <= CUT_A2 on every kept pair.
 * With kappa = G_r d_r + G_g d_g + G_b d_b + G_T r T_end of "Gradients of an image loss" (its a, before opacity_scale):
 * b dL/db = -kappa and db/da' = -ln2 b off the clamp, so dL/da' = ln2 kappa per pair.  Perturb mu -> mu + dmu and I' -> (1 + E) I':
 * da' = 2 p^T (E p - I' dmu); the antisymmetric part of E turns the unit disc into itself and drops out.  Hence with
 *   m_k  = sum_p kappa p_k   (k = 0, 1)        S_kl = sum_p kappa p_k p_l   (00, 01, 11)
 * five sums per splat, bounded because |p| is:
 *   dL/dmu    = sum_p ln2 kappa (-2 I'^T p)                          = -2 ln2 I'^T m                (px^-1, x right, y down)
 *   dL/dSigma = sum_p ln2 kappa (-(log2 e / 2) Sigma^-1 d d^T Sigma^-1) = -2 (ln2)^2 I'^T S I'      (symmetric 2 x 2, px^-2)
 * the second with d = x - mu and Sigma^-1 d = (2 / log2 e) I'^T p.
 * ws_renderer_accumulate_geometry_gradient: preconditions and descriptor checks exactly those of ws_renderer_accumulate_gradient
 * (geometry_scale in the place of opacity_scale: finite, > 0), WS_ERR_INVALID for a ws_geomgrad of another size, WS_ERR_UNSUPPORTED
 * for a compressed cloud.  Three launches on `stream`, no blend launch, no target changed; counts as a frame of g.
 * STAGE A, k_removal_base (unchanged) and k_geometry: the pairs, weights and stops of "Per-Gaussian contributions"; per walked pair
 * Tb, T, P_ch, r, d_ch, u and kappa exactly as "Gradients of an image loss" forms them (one copy of the code), counted under its
 * opacity rule: kept, w > 0, Tb >= 2^-14, not on the 0.99 clamp.  With p0, p1 the walk's own values, every multiply rounded by itself:
 *   t = geometry_scale * kappa;  v = (t * p0, t * p1, (t * p0) * p0, (t * p0) * p1, (t * p1) * p1)
 * each NaN -> 0 and capped silently at +-0x1.fffffep-1f, into five int64 sums per Gaussian under the ACCUMULATION rule of
 * "Gradients of an image loss" (q = (int64_t)(v * 2^32) toward zero; integer sums commute), in the accumulator's scratch.  Bit for
 * bit: g and -g give negated sums; a 0/1 mask of the plane and its complement add up to the whole; the launch geometry and
 * repetition do not show.
 * STAGE B, k_geom_spread: one thread per store slot i of the prepared frame (slots at or beyond the visible count return), no
 * atomics.  j = src_index[i]; the five scratch sums of j all 0: nothing else is read or written; else they are zeroed again (the
 * next frame needs no memset) and, ALL IN F64 with + - x / sqrt and comparisons only, none contracted:
 *   1. I' from the record's four halves by the blend's decode expressions; m, S = sums / (2^32 geometry_scale); dmu and D = dL/dSigma
 *      as above.  K1 forms Sigma with y up (its Jacobian's second row is negated), so D_K = diag(1, -1) D diag(1, -1).
 *   2. from the prepared frame's ws_camera_uniform and ws_settings_uniform, the cloud's f32 position and six f16 covariance halves,
 *      as K1 states them: cs = view (xyz, 1); clip = proj cs; w; jac(cs) = [fx / z, 0, -fx x / z^2; 0, -fy / z, fy y / z^2]; T = jac
 *      view3x3; scaling^2 = (gaussian_scaling scale_mod)^2; V = scaling^2 sym(cov); lambda2_raw of T V T^T + kernel_size I.
 *   3. position.  Through the centre mu_px = ((clip_x / w / 2 + 1/2) W, (1/2 - clip_y / w / 2) H); through the Jacobian,
 *      dL/dT = 2 D_K T V, on through jac's four non-zero entries to cs; both to the world by view^T.
 *   4. covariance.  scaling^2 T^T D_K T as six numbers (xx xy xz yy yz zz): the derivatives with respect to the six STORED
 *      elements, so an off-diagonal is twice the symmetric matrix's entry.
 *   5. the statistic.  n = sqrt(gx^2 + gy^2) of the NDC gradient (W/2 dmu_x, -H/2 dmu_y) -- the INRIA trainer's
 *      viewspace_point_tensor.grad -- is added to screen_norm[j], and 1 to seen[j].
 * LEFT OUT.  A splat whose lambda2_raw < 0.1 has its record's minor axis on K1's clamp: it adds nothing to the covariance sums and
 * nothing through the Jacobian; its centre path still counts.  The dependence of the colour on the view direction, of the
 * mip-splatting opacity factor on Sigma and of the fade-in scale_mod on the position are not differentiated.  The record's f16
 * rounding is treated as the identity.  Compressed clouds are refused (WS_ERR_UNSUPPORTED), as ws_refit refuses them.  No
 * optimiser step moves positions or covariances.
 * THE SUMS.  Ten f64 per Gaussian (position 3, covariance 6, screen_norm 1) and one uint64 count, one plane per element on the
 * device.  They are f64, not q32, because their range is unbounded: a covariance gradient scales with 1 / extent^2.  Each Gaussian
 * belongs to one thread per frame and the stream orders the frames: the result is reproducible for a given frame order, and it is
 * in units of the clamped plane G (divide by scale).  Merges across ranks are exact only for seen; ws_geomgrad_add adds in the
 * order given.  ws_geomgrad_download: any of the four arrays may be NULL; syncs.
 * ws_geom_spread_rows (host only, no device needed): stage B's per-Gaussian code from the same text, over n rows -- q5[n][5] one
 * frame's scratch sums, rec[n][4] the record's halves 0..3 as f16 bits, xyz[n][3], cov[n][6] f16 bits; rows whose five sums are
 * all 0 are skipped; ADDS to the four arrays (any may be NULL). */
typedef struct ws_geomgrad ws_geomgrad;         /* ten f64 sums and one uint64 count per Gaussian, device memory, zeroed */
typedef struct ws_geometry_params {
    float background[3]; float scale; float geometry_scale; uint32_t reserved0;   /* scales finite, > 0; reserved0 zero */
    const float* d_grad; size_t grad_pitch_bytes;      /* as ws_gradient_params */
    float* d_base; size_t base_pitch_bytes;            /* may be NULL, as ws_removal_params */
    uint32_t reserved[4];                              /* zero */
} ws_geometry_params;
int  ws_geomgrad_create(ws_context* ctx, uint32_t num_points, ws_geomgrad** out);
void ws_geomgrad_destroy(ws_geomgrad* g);
int  ws_geomgrad_reset(ws_geomgrad* g, void* stream);
uint32_t ws_geomgrad_num_points(const ws_geomgrad* g);
uint32_t ws_geomgrad_frames(const ws_geomgrad* g);
int  ws_geomgrad_download(ws_geomgrad* g, uint32_t capacity, double* position /* [capacity][3] */, double* covariance /* [capacity][6] */,
                          double* screen_norm /* [capacity] */, uint64_t* seen /* [capacity] */);   /* syncs */
int  ws_geomgrad_add(ws_geomgrad* g, const double* position, const double* covariance, const double* screen_norm, const uint64_t* seen,
                     uint32_t n);
int  ws_renderer_accumulate_geometry_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_geomgrad* g, const ws_geometry_params* p,
                                              void* stream); /* enqueues; counts as a frame of g */
int  ws_geom_spread_rows(const int64_t* q5, const uint16_t* rec, const float* xyz, const uint16_t* cov, const ws_camera_uniform* cam,
                         const ws_settings_uniform* settings, float geometry_scale, uint32_t n, double* position, double* covariance,
                         double* screen_norm, uint64_t* seen);
/* ws_scene_accumulate_gradient's walk over the cameras with this per-frame call (geometry_scale where that has opacity_scale) */
int  ws_scene_accumulate_geometry_gradient(ws_context* ctx, const ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc,
                                           const char* gt_dir, int kind, float scale, float geometry_scale, ws_geomgrad* grad, uint32_t* frames);
/* test hook: the scratch of a ws_geomgrad, [capacity][5] int64 (m0, m1, S00, S01, S11); syncs.  Zero between the calls. */
int  ws_debug_geomgrad_scratch(ws_geomgrad* g, uint32_t capacity, int64_t* q5);
/* test hooks: stage A alone (k_removal_base + k_geometry) into g's scratch, adding no frame; and the scratch zeroed again, which a
 * caller of the first owes the next ws_renderer_accumulate_geometry_gradient (stage B would have done it). */
int  ws_debug_geometry_stage_a(ws_renderer* r, const ws_pointcloud* pc, ws_geomgrad* g, const ws_geometry_params* p, void* stream);
int  ws_debug_geomgrad_clear_scratch(ws_geomgrad* g, void* stream);
/* ---- Refitting colour and opacity: Adam steps on the resident planes, in place (no counterpart in the reference) -----------------
 * What "Gradients of an image loss" is for: its sums say in which direction every colour and opacity of a (pruned) cloud should
 * move; a ws_refit moves them.  It belongs to ONE uncompressed point cloud and holds, per Gaussian, f32 masters of four
 * parameters and the two Adam moments of each, in device memory.  The parameters are indexed like WS_GRAD_CHANNELS:
 *   x[0..2]  the DC SH coefficients: the first [f16;3] of the 96-B SH record (the first 6 bytes of plane 2's chunk)
 *   x[3]     the opacity: the f16 behind x, y, z in the 28-B record (plane 0), the post-sigmoid value the loaders store
 * ws_refit_create runs a small kernel that widens those four halves to the f32 masters and sets m = v = 0; steps = 0 and the
 * running powers p1 = beta1^steps, p2 = beta2^steps are host doubles, 1.0 at creation.  Compressed clouds are refused with
 * WS_ERR_UNSUPPORTED: their codebooks are shared between Gaussians.
 * GRADIENTS TO PARAMETERS.  K1 computes colour = max(0, 0.5 + C0 * dc + the view-dependent rest), C0 = 0.28209479177387814, and a
 * ws_grad's colour sums are derivatives with respect to an offset before that clamp: dL/d dc = C0 * dL/d colour.  Its opacity
 * sum is dL/d ln(opacity), which a constant factor on the opacity (mip-splatting's) does not change: dL/d opacity = sum / opacity.
 * colour_unit and opacity_unit say what ONE unit of a sum is worth as dL/d colour and as dL/d ln opacity: for sums of B frames
 * through `scale` and `opacity_scale`, the mean over the frames has colour_unit = 1 / (2^32 * scale * B) and opacity_unit =
 * 1 / (2^32 * scale * opacity_scale * B).
 * THE STEP, TO THE BIT.  Once per call, on the host: p1 <- p1 * (double)beta1, p2 <- p2 * (double)beta2; bc1 = (float)(1.0 - p1),
 * bc2 = (float)(1.0 - p2); omb1 = 1.0f - beta1, omb2 = 1.0f - beta2 in f32; u_c = colour_unit * C0, u_o = opacity_unit in double.
 * One thread per Gaussian j; for each channel k of a group whose rate is not 0, with x, m, v the stored f32 values and q the sum:
 *   g  = (float)((double)q[j][k] * u)         u = u_c for k < 3, u_o for k = 3; int64 -> double and double -> float round to
 *                                             nearest even
 *   k = 3 only:  g = (x == 0) ? 0 : g / x     x the opacity master before the step
 *   m' = (beta1 * m) + (omb1 * g)
 *   v' = (beta2 * v) + (omb2 * (g * g))
 *   s  = (m' / bc1) / (sqrtf(v' / bc2) + eps)
 *   x' = x - (lr * s)                         lr = lr_colour for k < 3, lr_opacity for k = 3
 *   k < 3:  x' below -65504 becomes -65504, above 65504 becomes 65504     k = 3:  below opacity_min -> opacity_min, above 1 -> 1
 * every operation a separately rounded IEEE f32 operation, no contraction, division and square root correctly rounded.  x', m',
 * v' are stored, and f16(x'), round to nearest even, into the four halves of the cloud's planes.  NO OTHER BYTE OF THE RESIDENT
 * CLOUD CHANGES: not x, y, z, not the two bytes of padding beside the opacity, not the SH halves behind the DC triple.  A rate of
 * 0 freezes its group: its masters, moments and stored halves are not written.  Consequences that hold to the bit: (a) a Gaussian
 * with q = 0 and m = v = 0 keeps its masters and its stored halves, provided opacity_min is not above its opacity; (b) the result
 * does not depend on the launch geometry.
 * THE EDGES OF THE STEP, pinned like the rest (tests/refit_edges.py; profiles/refit/edges.json).  Denormals are honoured in every
 * operation above -- operands and results, the division and the square root included -- and in both conversions: a subnormal
 * half widens to its exact f32 master, and f16(x') rounds to nearest even onto subnormal halves (2^-25 stores as 0, 3 * 2^-25 as
 * 0x0002).  Nothing is flushed: a first moment that decays under zero sums ends at +-4 * 2^-149 (4 * 0.9 rounds back to 4), not
 * at 0.  A NaN passes both clamps (x' < lo and x' > hi are false) and is stored as a NaN half, its sign and payload the
 * hardware's; a master of +-inf (an infinite half widened, or an x' that overflowed) is clamped like any other value: +-65504,
 * opacity_min or 1.  A NaN half that a step only passes through keeps its bits, a signalling one too.  A master of -0 with sum 0
 * stays -0.  Beyond the f32 range of g * g there are TWO OVERFLOW REGIMES, both permanent:
 *   g * g = inf with g finite (|g| >= 2^64):  v' = inf, s = m^ / inf = 0, x' = x.  v stays inf under every later sum (beta2 * inf):
 *                                             the parameter never moves again.
 *   g = +-inf (|q * u| >= 2^128, or the opacity's g / x):  m' = +-inf, s = inf / inf = NaN: the master and its stored half are
 *                                             NaN from this step on.
 * Neither can occur while |q * u| < 2^63 for the colour and rest sums and |q * u / x| < 2^63 for the opacity, x its master (then
 * g * g < 2^126 and every later intermediate is finite).  The descriptor checks do not enforce this bound: units are only required
 * to be finite and positive, and an opacity master may lie far below the f16 range (opacity_min = 0 allows it: the master 2^-40
 * stores as the half 0 and divides a sum by 2^-40).  Keeping the sums inside the bound is the caller's business.
 * ORDER.  ws_refit_step only ENQUEUES on `stream`, behind the accumulations that filled `g` on it.  Frames prepared later on that
 * stream see the new values (K1 reads the planes at every prepare()); frames of the cloud in flight on OTHER streams, prepared
 * or being prepared, are the caller's business -- the step does not wait for them.  ws_refit_download syncs.
 * Errors: WS_ERR_INVALID for null params, a rate that is negative or not finite, a beta outside [0, 1), an eps that is not finite
 * and above 0, an opacity_min outside [0, 1], a unit that is not finite and above 0, non-zero reserved words -- all judged from the
 * descriptor before a handle is looked at; then for null handles, a `pc` other than the one the object was created for, a ws_grad
 * of another size; ws_refit_download: a capacity below the number of points.
 * ws_scene_refit: per epoch, the cameras of `split` in split order through the per-frame sequence of
 * ws_scene_accumulate_gradient (the same set-up; scale = 1, the caller's opacity_scale, image b the render of `ref_pc` or the
 * PNGs of `gt_dir`) into a ws_grad of the driver's own.  A batch ends after every views_per_step frames (0 = the whole split) and
 * at the end of the epoch if one is partly filled; after a batch of B frames the driver enqueues ws_refit_step with colour_unit =
 * 1 / (2^32 * B), opacity_unit = 1 / (2^32 * opacity_scale * B), computed in double (the two fields of `params` are ignored),
 * then ws_grad_reset.  Argument checks as ws_scene_accumulate_gradient, the params' as ws_refit_step; ref_pc == pc is refused.
 * One stream, one sync and one look at the error bits per epoch; WS_ERR_OVERFLOW under ws_scene_accumulate_contrib's rule, after
 * the steps of that epoch have been taken.  *steps = the steps taken.  Known costs: the reference cloud is rendered again every
 * epoch, and the PNGs are read again every epoch.
 * THE REST COEFFICIENTS (the sums of "SH gradients").  ws_refit_enable_sh allocates f32 masters and two moments for the
 * 3 * (ncoef - 1) rest elements of the cloud, one plane per element, and enqueues a small kernel that widens the stored halves and
 * sets m = v = 0.  WS_ERR_INVALID once ws_refit_steps() > 0 (the bias-correction powers are shared); a second call is a no-op;
 * sh_deg = 0 enables nothing and succeeds.  ws_refit_step_sh enqueues ONE kernel, one thread per (Gaussian, 16-B piece of the SH
 * record):
 *   DC and opacity: THE STEP above, word for word, fed with q_sh[:, 0, :] and q_opacity of the ws_shgrad.
 *   a rest element e = 3 * coef + ch, coef >= 1: the same step with g = (float)((double)q_sh[j][coef][ch] * colour_unit) -- no C0:
 *   the basis is in the sum already --, lr = lr_sh, the clamp at +-65504, and f16(x') stored to half e of the SH record.
 * steps, p1 and p2 are the object's own, shared with ws_refit_step: the two calls may be mixed.  A frozen group keeps the bits it
 * read and its masters and moments are not written; so do the halves past 3 * ncoef of the record.  No byte of the cloud changes
 * outside the opacity half and the first 3 * ncoef SH halves.  With lr_sh = 0 a ws_refit_step_sh leaves the same masters, moments
 * and cloud bytes as ws_refit_step with a ws_grad holding the same four sums.  ws_refit_download_sh: [capacity][ncoef - 1][3] f32
 * each, any may be NULL; syncs.  Errors: the descriptor's as ws_refit_step's plus an lr_sh that is negative or not finite, judged
 * before a handle is looked at; then WS_ERR_INVALID for null handles, a `pc` other than the object's, a step or download before
 * ws_refit_enable_sh, a ws_shgrad of another size or degree.
 * ws_scene_refit_sh: ws_scene_refit with ws_renderer_accumulate_sh_gradient as the per-frame call, a ws_shgrad of the driver's
 * own and ws_refit_step_sh; it calls ws_refit_enable_sh itself if it has not been called.  Units as in ws_scene_refit.
 * Out of scope: position and covariance; learning-rate schedules; raising a cloud's SH degree.  A refitted cloud is kept
 * with ws_pointcloud_save_ply ("Saving a point cloud" below). */
typedef struct ws_refit ws_refit;               /* f32 masters and Adam moments of one uncompressed cloud, device memory */
typedef struct ws_refit_params {
    float lr_colour, lr_opacity;     /* finite, >= 0; 0 freezes the group: its masters, moments and stored halves are not touched */
    float beta1, beta2, eps;         /* betas in [0, 1), eps finite and > 0 */
    float opacity_min;               /* in [0, 1]: lower clamp of the opacity master */
    double colour_unit, opacity_unit;/* what ONE unit of a ws_grad sum is worth as dL/d colour and as dL/d ln opacity: finite, > 0 */
    uint32_t reserved[4];            /* zero */
} ws_refit_params;
int  ws_refit_create(ws_context* ctx, const ws_pointcloud* pc, ws_refit** out);
void ws_refit_destroy(ws_refit* refit);
uint32_t ws_refit_num_points(const ws_refit* refit);
uint32_t ws_refit_steps(const ws_refit* refit);
int  ws_refit_step(ws_refit* refit, ws_pointcloud* pc, const ws_grad* g, const ws_refit_params* params, void* stream);   /* enqueues only */
int  ws_refit_download(ws_refit* refit, uint32_t capacity, float* master, float* m, float* v);   /* [capacity][4] each, any may be NULL; syncs */
int  ws_scene_refit(ws_context* ctx, ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc, const char* gt_dir,
                    int kind, float opacity_scale, ws_refit* refit, const ws_refit_params* params, uint32_t epochs, uint32_t views_per_step,
                    uint32_t* steps);
typedef struct ws_refit_sh_params {
    ws_refit_params base;            /* as ws_refit_step; colour_unit is also what one unit of a rest sum is worth */
    float lr_sh;                     /* finite, >= 0; 0 freezes the rest coefficients */
    uint32_t reserved[3];            /* zero */
} ws_refit_sh_params;
int  ws_refit_enable_sh(ws_refit* refit, const ws_pointcloud* pc, void* stream);   /* enqueues only */
int  ws_refit_step_sh(ws_refit* refit, ws_pointcloud* pc, const ws_shgrad* g, const ws_refit_sh_params* params, void* stream);   /* enqueues only */
int  ws_refit_download_sh(ws_refit* refit, uint32_t capacity, float* master, float* m, float* v);   /* [capacity][ncoef - 1][3] each, any may be NULL; syncs */
int  ws_scene_refit_sh(ws_context* ctx, ws_pointcloud* pc, const ws_scene* scene, int split, const ws_pointcloud* ref_pc, const char* gt_dir,
                       int kind, float opacity_scale, ws_refit* refit, const ws_refit_sh_params* params, uint32_t epochs, uint32_t views_per_step,
                       uint32_t* steps);
/* ---- Saving a point cloud: the resident planes back to an INRIA 3DGS .ply (no counterpart in the reference) -------------------------
 * The last step of prune -> refit -> evaluate: a resident, uncompressed cloud written as the file this library, the reference
 * viewer and every other 3DGS tool read.  The resident scene holds the covariance (six f16 halves) and the opacity after the
 * sigmoid; the file stores three log-scales, a quaternion and an opacity logit: saving inverts the load kernel, one thread per
 * Gaussian (k_ply_encode, ply_encode.hip), with a host twin of the same operations (ws_ply_rows_encode, no GPU needed).
 * THE ROW, TO THE BIT: 14 + 3 (sh_deg + 1)^2 f32 in the file's order, x y z | nx ny nz | f_dc[3] | f_rest[3][C-1] | opacity |
 * scale[3] | rot[4], with C = (sh_deg + 1)^2.
 *   x y z     the f32 bits as they are.                  nx ny nz   +0.
 *   f_dc, f_rest   the f16 halves widened to f32 (exact; a NaN half gives a NaN), transposed back from the resident
 *             coefficient-major [16][3] to the file's channel-major [3][C-1].  Coefficients above the cloud's degree are not written.
 *   opacity   with o the half widened to f64: (float)log(o / (1 - o)) for 0 < o < 1; -20 for o <= 0 (-0 included) and +20 for
 *             o >= 1 -- finite, and sigmoid(-+20) rounds to the halves 0 and 1 under both decoders; a NaN half gives NaN.  THE ONE
 *             LOSSY CASE: a half above 1 is written as 1.
 *   scale, rot   the six halves c00 c01 c02 c11 c12 c22 widened to f64; a cyclic Jacobi eigen-solve in f64: pairs in the order
 *             (0,1), (0,2), (1,2), at most 16 sweeps, ended when the three off-diagonal entries are exactly 0.  A rotation is
 *             skipped when its off-diagonal entry is 0; the entry is set to 0 without a rotation when 100 times its magnitude, added
 *             to the magnitude of either diagonal entry, changes neither; otherwise t = a_pq / h when 100 |a_pq| added to |h| does
 *             not change |h| (h = a_qq - a_pp), else t = sign(theta) / (|theta| + sqrt(1 + theta^2)), theta = 0.5 h / a_pq; c =
 *             1 / sqrt(1 + t^2), s = t c, tau = s / (1 + c); a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and every other pair (x, y)
 *             the rotation touches becomes (x - s (y + x tau), y + s (x - y tau)).  Only + - x / sqrt: host and device agree to the bit.
 *             THE ORDER: eigenvalue k is entry k of the diagonal the sweeps end with, eigenvector k column k of the accumulated
 *             rotations; nothing is sorted.  A product of plane rotations is a proper rotation (det = +1), and a covariance that is
 *             diagonal already keeps R = I and comes back exactly (sorting would turn it by 90 degrees, which f32 quaternion
 *             components cannot express exactly).  The quaternion
 *             is taken from R by the largest pivot among trace, R00, R11, R22 (Shepperd; the first of equals), normalised in f64,
 *             negated as a whole when its scalar part is negative (a scalar part of -0 is written +0), and each component rounded once
 *             to f32: rot_0 >= 0 is the scalar part.  scale_k = (float)(0.5 * log(l_k)) for l_k > 0; l_k <= 0 gives -20, whose exp
 *             squared is 0 in f16.
 *             A covariance with a half that is not finite gets the identity quaternion (1, 0, 0, 0) and its scales from the
 *             diagonal by the same rule, a diagonal half of +inf taken as 65504 and one that is NaN or -inf as 0: finite and
 *             deterministic; nothing traps or loops on it.
 * The two log() calls are the only operations that are not IEEE operations: everything else is identical between kernel and host
 * twin, and the four log columns are within one f32 ulp of each other.
 * WHAT COMES BACK.  Loading what was saved gives the positions, the SH halves and the opacity halves (o > 1 -> 1; NaN as a class)
 * bit for bit.  An f16-rounded covariance is often INDEFINITE, which the file cannot express: a negative eigenvalue is written as
 * a zero extent, and every element of the reloaded covariance C' obeys |C' - C| <= sum |l_neg| + ulp16(max(|C|, |C'|)): the
 * clamp moves an element by at most sum |l_neg|, the re-rounding and the f32 decode by under one f16 ulp.  Where
 * l_min > 2^-10 l_max the six halves come back identical but for about one row in 10^4.  A cloud saved twice is stable; a cloud
 * loaded and saved is not byte-equal to its source (only the covariance is resident, not the file's scales and quaternion).
 * ws_pointcloud_encode_ply_rows: the rows of `pc` into host memory, num_points x row length f32 (rows_bytes at least that).  The
 * kernel and the copy run on a private stream and are waited for; the rows are staged in ONE device buffer of that size, released
 * at the return.  Work on other streams that writes the cloud (ws_refit_step) must have been waited for.
 * ws_pointcloud_encode_ply_rows_device: the same kernel into DEVICE memory of the caller's, only ENQUEUED on `stream` -- for rows
 * that stay on the device, and what scripts/ply_encode_cost.py times.  ws_pointcloud_decode_ply_rows_device is its inverse: k_ply_decode
 * of num_points device rows of the cloud's degree INTO the cloud's planes, enqueued on `stream`; bbox, centre and the comments'
 * values stay as they are (the caller's business, as for ws_pointcloud_create).  Same refusals; rows_bytes is checked, the pointer is trusted.
 * ws_pointcloud_save_ply: the rows, then ws_ply_write with the cloud's mip / kernel_size / background_color.  `path` is opened
 * only after the rows exist.
 * ws_ply_write (host only): `ply`, `format binary_little_endian 1.0`, the comments `mip=true|false`, `kernel_size=%.9g`,
 * `background_color=%.9g,%.9g,%.9g` exactly when `meta` (may be NULL; its other fields are ignored) has them -- nine digits give
 * every f32 back --, `element vertex N`, the property list above as `property float NAME`, `end_header`, the rows.  n == 0 writes a
 * valid empty file.  On an I/O error the partial file is removed: WS_ERR_IO.
 * Errors: WS_ERR_UNSUPPORTED for a compressed cloud (its codebooks are shared between Gaussians) and sh_deg > 3; WS_ERR_INVALID for
 * null arguments and a rows_bytes that is too small.
 * Out of scope: .npz / compressed output; big-endian or ASCII output; keeping the source file's scales and quaternion; expressing
 * an indefinite covariance exactly. */
int ws_ply_rows_encode(const void* gaussians /* 28 B x n */, const void* sh /* 96 B x n */, uint32_t n, uint32_t sh_deg, float* rows_out);
int ws_pointcloud_encode_ply_rows(const ws_pointcloud* pc, float* rows, size_t rows_bytes);   /* syncs */
int ws_pointcloud_save_ply(const ws_pointcloud* pc, const char* path);                        /* syncs */
int ws_pointcloud_encode_ply_rows_device(const ws_pointcloud* pc, float* d_rows, size_t rows_bytes, void* stream);        /* enqueues only */
int ws_pointcloud_decode_ply_rows_device(ws_pointcloud* pc, const float* d_rows, size_t rows_bytes, void* stream);        /* enqueues only */
int ws_ply_write(const char* path, const float* rows, uint32_t n, uint32_t sh_deg, const ws_pointcloud_desc* meta);
/* ---- view batches (BASELINE configs 4 / 5: many independent views of one resident scene) ----------------
 * The reference renders one view at a time on one queue (lib.rs:422-431, bin/measure.rs:98-146).  A view batch keeps
 * `frames_in_flight` frames going at once: frame i of the batch's life runs on renderer + HIP stream i mod
 * frames_in_flight (private scratch each; the point cloud is shared).  ws_view_batch_render only ENQUEUES; the caller
 * observes completion with ws_view_batch_sync.  The host's RUN-AHEAD is bounded: a slot's host side stays at most 5 frames
 * (WS_BATCH_QUEUE_DEPTH; 0 = unbounded) ahead of the device, so a call with more views than slots x 5 returns when all but
 * the last of them have reached the device -- the caller's thread SLEEPS meanwhile (it polls a word the compositing kernel
 * posts to pinned memory; no runtime call, no spinning: a rank costs 0.5-0.7 host cores instead of 1.9).  On an error in the
 * middle of a call the one-thread path stops at the failing frame; with submission threads (below) the other slots still
 * enqueue THEIR frames of the call, and the frame-to-slot position advances by num_views.  For point clouds of at most 512 Ki Gaussians -- where the GPU needs less time
 * per frame than one host thread needs to enqueue it -- every slot's frames are enqueued by a worker thread of the batch (the
 * order on each stream is unchanged; the call returns when everything is enqueued; WS_BATCH_THREADS=0 / 1 forces it off / on).
 * d_targets[i] receives view i (device memory, format of the batch);
 * targets may repeat with period frames_in_flight (a ring), since a slot's frames are ordered on its stream. */
typedef struct ws_view_batch ws_view_batch;
int ws_view_batch_create(ws_context* ctx, ws_color_format format, uint32_t sh_deg, int compressed,
                         uint32_t frames_in_flight, ws_view_batch** out);
void ws_view_batch_destroy(ws_view_batch* b);
uint32_t ws_view_batch_frames_in_flight(const ws_view_batch* b);
int ws_view_batch_render(ws_view_batch* b, const ws_pointcloud* pc, const ws_splatting_args* views, uint32_t num_views,
                         void* const* d_targets, size_t row_pitch_bytes, const float background[4]);
int ws_view_batch_sync(ws_view_batch* b);
int ws_view_batch_errors(ws_view_batch* b, uint32_t* bits, int reset); /* OR of ws_renderer_errors over the slots (syncs) */
ws_renderer* ws_view_batch_renderer(ws_view_batch* b, uint32_t slot); /* the renderer of a slot (stats, timers) */
/* times ws_view_batch_render had to sleep because a slot's host side was queue_depth frames ahead of the device (statistics).
 * A slot whose progress word does not move for 10 s (lost launch, device fault) makes ws_view_batch_render return
 * WS_ERR_STATE once; its later frames are enqueued without the bound. */
uint32_t ws_view_batch_host_waits(const ws_view_batch* b);

/* Display::render (renderer.rs:548-582) + display.wgsl:37-55: the splat image (premultiplied RGBA, renderer
 * format) composited with PREMULTIPLIED_ALPHA_BLENDING over a surface cleared to `background`, written as 8-bit
 * unorm in the surface's channel order (lib.rs:184-243 picks the surface format and strips the sRGB suffix).
 * Per channel: out = c + background * (1 - a) in f32 (the multiply-add may be fused), clamped to [0, 1], * 255, rounded half
 * to even.  A NaN result (a NaN texel, inf - inf, 0 * inf) stores 0; +-inf clamp to 0 / 255.  Rows beyond `width` texels (the
 * pitch's padding) are neither read into a pixel nor written. */
typedef enum ws_surface_format { WS_SURFACE_RGBA8_UNORM = 0, WS_SURFACE_BGRA8_UNORM = 1 } ws_surface_format;
int ws_display_composite(ws_context* ctx, const void* d_src, ws_color_format src_format, size_t src_pitch_bytes,
                         uint32_t width, uint32_t height, const float background[4], ws_surface_format dst_format,
                         void* d_dst, size_t dst_pitch_bytes, void* stream);

/* ---- GPURSSorter: gpu_rs.rs:65-175, 720-727, 865-884 ------------------------------------------ */
/* GPURSSorter::new + create_sort_stuff(device, max_n): scratch for sorting up to max_n pairs */
int ws_sorter_create(ws_context* ctx, uint32_t max_n, ws_sorter** out);
void ws_sorter_destroy(ws_sorter* s);
/* record_sort (d_count == NULL, sorts n pairs) / record_sort_indirect (count read from device memory,
 * clamped to n): ascending, stable, in place in d_keys / d_payload (gpu_rs.rs:865-884). */
int ws_sorter_sort(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, const uint32_t* d_count, uint32_t n,
                   void* stream);
/* The same contract (record_sort / record_sort_indirect) through the kernels a frame's depth sort runs: the generic sorter
 * at the context's digit width (8 or 9 bits) and 9-bit tile size, with the frame's key-range fold unless the context's
 * depth_skip_top is 0 -- passes 1..3 sort key - base, and the fourth pass is skipped when the keys span less than three
 * digits above the base (ws_sorter_depth_range reads the decision back) -- or, in a context created with
 * WS_DEPTH_SORT=onesweep | coop, the fat-tile one-sweep; d_aux (may be NULL) is a 4-byte companion that travels with the
 * payload.  In place: after three passes a copy kernel brings [0, count) back; nothing past count is touched.
 * d_keys must be 16-byte aligned (both entry points: the histogram kernels read the keys four at a time);
 * WS_ERR_INVALID otherwise. */
int ws_sorter_sort_depth(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, uint32_t* d_aux, const uint32_t* d_count,
                         uint32_t n, void* stream);
/* GPURSSorter::test_sort (gpu_rs.rs:295-331): 8192 reversed f32 keys must come out ascending. 1 = pass */
int ws_sort_selftest(ws_context* ctx, int* passed);

#ifdef __cplusplus
}
#endif
#endif /* WEBSPLAT_H */
