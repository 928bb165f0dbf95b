// api_pointcloud.cpp -- ws_pointcloud (PointCloud, pointcloud.rs:72-222): creation from the loader's blobs, from PLY rows and as a
// subset of another cloud, download, saving as a PLY, and the getters.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "api_state.h"
#include "contrib.h"
#include "ply_encode.h"

using namespace ws;

// A failure of an owner's alloc() / create() under the name an entry point gives its uploads ("ws_pointcloud_create: upload: out
// of memory"): hip_fail's "what: why"
static int alloc_as(int rc, const char* what) {
    if (rc) {
        std::string why = ws_last_error();
        set_error(why.replace(0, why.rfind(": "), what));
    }
    return rc;
}

extern "C" {

// ---- PointCloud --------------------------------------------------------------------------------------
// what a descriptor says about how its scene wants to be drawn
static void set_render_hints(PointCloudMeta* pc, const ws_pointcloud_desc* d) {
    pc->has_mip = d->has_mip_splatting != 0;
    pc->mip = d->mip_splatting != 0;
    pc->has_kernel_size = d->has_kernel_size != 0;
    pc->kernel_size = d->kernel_size;
    pc->has_background = d->has_background_color != 0;
    std::memcpy(pc->background, d->background_color, sizeof pc->background);
}
int ws_pointcloud_create(ws_context* ctx, const ws_pointcloud_desc* d, ws_pointcloud** out) {
    if (!ctx || !d || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create: null argument");
    *out = nullptr;
    if (d->sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create: sh_deg > 3");
    const uint32_t n = d->num_points;
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create: empty point cloud");
    if (n >= (1u << 30)) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create: more than 2^30-1 points");
    if (!d->gaussians || !d->sh_coefs) return fail(WS_ERR_INVALID, "ws_pointcloud_create: missing buffers");
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create: host allocation failed");
    pc->ctx = ctx;
    pc->num_points = n;
    pc->sh_deg = d->sh_deg;
    pc->compressed = d->compressed != 0;
    pc->bbox = d->bbox;
    std::memcpy(pc->center, d->center, sizeof pc->center);
    pc->has_up = d->has_up != 0;
    std::memcpy(pc->up, d->up, sizeof pc->up);
    set_render_hints(pc.get(), d);
    if (!pc->compressed) {
        if (d->gaussians_bytes != (size_t)n * 28 || d->sh_coefs_bytes != (size_t)n * 96)
            return fail(WS_ERR_INVALID, "ws_pointcloud_create: expected 28 B Gaussians and 96 B SH records");
        // re-lay the loader's AoS records as eight planes of 16-B chunks (ws_internal.h)
        std::vector<uint32_t> staging;
        try {
            staging.resize((size_t)n * PC_PLANES * 4);
        } catch (...) {
            return fail(WS_ERR_OOM, "ws_pointcloud_create: host staging allocation failed");
        }
        const uint8_t* g = static_cast<const uint8_t*>(d->gaussians);
        const uint8_t* s = static_cast<const uint8_t*>(d->sh_coefs);
        uint32_t* st = staging.data();
        const ws::OmpQuietWorkers omp_quiet;  // (ws_internal.h: the region's workers sleep at once instead of spinning 200 ms)
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)n; ++i) {
            const uint8_t* gi = g + (size_t)i * 28;
            uint32_t* p0 = st + ((size_t)0 * n + i) * 4;
            std::memcpy(p0, gi, 16);  // x, y, z, opacity f16 | pad
            uint32_t* p1 = st + ((size_t)1 * n + i) * 4;
            std::memcpy(p1, gi + 16, 12);  // cov f16 x 6
            p1[3] = 0u;
            const uint8_t* si = s + (size_t)i * 96;
            for (int q = 0; q < 6; ++q) std::memcpy(st + ((size_t)(2 + q) * n + i) * 4, si + q * 16, 16);
        }
        WS_TRY(alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), "ws_pointcloud_create: upload"));
        const hipError_t e = hipMemcpy(pc->planes.get(), st, pc->planes.bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "ws_pointcloud_create: upload");
    } else {
        const uint32_t ncoef = (d->sh_deg + 1) * (d->sh_deg + 1);
        if (d->gaussians_bytes != (size_t)n * 24 || !d->covars || !d->quantization || (d->covars_bytes % 12) != 0 ||
            (d->sh_coefs_bytes % (3 * ncoef)) != 0)
            return fail(WS_ERR_INVALID, "ws_pointcloud_create: compressed layout mismatch (24 B splats, 12 B covars, "
                                        "3*(deg+1)^2 B SH records, quantization block)");
        // the kernel indexes covars / SH records with the per-Gaussian indices: validate them on the host,
        // where WebGPU would have clamped out-of-bounds reads
        const uint8_t* g = static_cast<const uint8_t*>(d->gaussians);
        const uint32_t n_cov = (uint32_t)(d->covars_bytes / 12), n_sh = (uint32_t)(d->sh_coefs_bytes / (3 * ncoef));
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t gi, si;
            std::memcpy(&gi, g + (size_t)i * 24 + 16, 4);
            std::memcpy(&si, g + (size_t)i * 24 + 20, 4);
            if (gi >= n_cov || si >= n_sh) return fail(WS_ERR_INVALID, "ws_pointcloud_create: geometry_idx / sh_idx out of range");
        }
        pc->quant = *d->quantization;
        // (the index check above has seen n_cov >= 1: no codebook is empty)
        const char* what = "ws_pointcloud_create: upload (compressed)";
        WS_TRY(alloc_as(pc->gaussians_c.alloc(d->gaussians_bytes), what));
        WS_TRY(alloc_as(pc->sh_bytes.alloc(d->sh_coefs_bytes + 16), what));
        WS_TRY(alloc_as(pc->covars.alloc(d->covars_bytes), what));
        hipError_t e = hipMemcpy(pc->gaussians_c.get(), d->gaussians, d->gaussians_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(pc->sh_bytes.get(), d->sh_coefs, d->sh_coefs_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(pc->covars.get(), d->covars, d->covars_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, what);
    }
    *out = pc.release();
    return WS_OK;
}

// PlyReader::read + PointCloud::new with the per-vertex conversion (io/ply.rs:50-100) done by a kernel: the rows go
// to the device as they sit in the file, k_ply_decode writes the resident planes directly (ply_decode.hip).
int ws_pointcloud_create_from_ply_rows(ws_context* ctx, const float* rows, uint32_t n, uint32_t sh_deg,
                                       const ws_pointcloud_desc* meta, ws_pointcloud** out) {
    if (!ctx || !rows || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create_from_ply_rows: null argument");
    *out = nullptr;
    if (sh_deg > 3) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create_from_ply_rows: sh_deg > 3");
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create_from_ply_rows: empty point cloud");
    if (n >= (1u << 30)) return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_create_from_ply_rows: more than 2^30-1 points");
    const uint32_t row_len = 14u + 3u * (sh_deg + 1u) * (sh_deg + 1u);
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create_from_ply_rows: host allocation failed");
    pc->ctx = ctx;
    pc->num_points = n;
    pc->sh_deg = sh_deg;
    pc->compressed = false;
    ws_aabb zero;  // Aabb::zeroed(), io/mod.rs:74: the positions are the first three floats of every row
    std::memset(&zero, 0, sizeof zero);
    int32_t has_up = 0;
    int rc = ws_pointcloud_stats(rows, n, row_len * (uint32_t)sizeof(float), &zero, &pc->bbox, pc->center, &has_up, pc->up);
    pc->has_up = has_up != 0;
    if (meta) set_render_hints(pc.get(), meta);
    // Upload and decode run on a PRIVATE stream and are waited for with hipStreamSynchronize: no legacy-NULL-stream work
    // (it would serialise against every renderer and break replays of a captured frame graph) and no
    // device-wide synchronisation of other renderers' frames.
    if (rc) return rc;
    DeviceBuf<float> d_rows;  // (let go at the return, behind the stream sync)
    Stream own;               // (declared behind d_rows: destroyed in front of it)
    const char* what = "ws_pointcloud_create_from_ply_rows: upload";
    hipError_t e = hipSuccess;
    rc = alloc_as(own.create(), what);
    const hipStream_t ls = own.get();
    if (rc == WS_OK) rc = alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), what);
    if (rc == WS_OK) rc = alloc_as(d_rows.alloc((size_t)n * row_len), what);
    if (rc == WS_OK && (e = hipMemcpyAsync(d_rows.get(), rows, d_rows.bytes(), hipMemcpyHostToDevice, ls)) != hipSuccess) rc = hip_fail(e, what);
    if (rc == WS_OK) rc = launch_ply_decode(d_rows.get(), n, sh_deg, pc->planes.get(), ls);
    if (rc == WS_OK) {
        e = hipStreamSynchronize(ls);
        if (e != hipSuccess) rc = hip_fail(e, "ws_pointcloud_create_from_ply_rows: decode");
    } else if (ls) {
        (void)hipStreamSynchronize(ls);
    }
    if (rc) return rc;
    *out = pc.release();
    return WS_OK;
}

// The scene blobs as the loader would have produced them (parity tooling / accessors): uncompressed clouds are
// re-assembled from the resident planes into 28-B Gaussians + 96-B SH records, compressed blobs are copied back as is.
int ws_pointcloud_download(const ws_pointcloud* pc, void* gaussians, size_t gaussians_bytes, void* sh_coefs, size_t sh_bytes) {
    if (!pc || !gaussians || !sh_coefs) return fail(WS_ERR_INVALID, "ws_pointcloud_download: null argument");
    const size_t n = pc->num_points;
    if (pc->compressed) {
        if (gaussians_bytes < n * 24) return fail(WS_ERR_INVALID, "ws_pointcloud_download: gaussians buffer too small");
        WS_HIP(hipMemcpy(gaussians, pc->gaussians_c.get(), n * 24, hipMemcpyDeviceToHost));
        return WS_OK;  // (the packed SH / covariance codebooks are what the caller uploaded; not re-exported)
    }
    if (gaussians_bytes < n * 28 || sh_bytes < n * 96) return fail(WS_ERR_INVALID, "ws_pointcloud_download: buffers too small");
    std::vector<uint32_t> st;
    try {
        st.resize(n * PC_PLANES * 4);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_pointcloud_download: host allocation failed");
    }
    WS_HIP(hipMemcpy(st.data(), pc->planes.get(), st.size() * 4, hipMemcpyDeviceToHost));
    uint8_t* g = static_cast<uint8_t*>(gaussians);
    uint8_t* s = static_cast<uint8_t*>(sh_coefs);
    const ws::OmpQuietWorkers omp_quiet;  // (ws_internal.h: the region's workers sleep at once instead of spinning 200 ms)
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        std::memcpy(g + (size_t)i * 28, st.data() + ((size_t)0 * n + i) * 4, 16);
        std::memcpy(g + (size_t)i * 28 + 16, st.data() + ((size_t)1 * n + i) * 4, 12);
        for (int q = 0; q < 6; ++q) std::memcpy(s + (size_t)i * 96 + q * 16, st.data() + ((size_t)(2 + q) * n + i) * 4, 16);
    }
    return WS_OK;
}

// Saving (websplat.h "Saving a point cloud"): k_ply_encode writes the rows into one DeviceBuf, which is copied to the host and
// let go at the return.  Kernel and copy run on a private stream and are waited for, as ws_pointcloud_create_from_ply_rows does.
static int ply_rows_device_check(const ws_pointcloud* pc, const void* d_rows, size_t rows_bytes, const char* who, size_t* need) {
    if (!pc) return fail(WS_ERR_INVALID, std::string(who) + ": null argument");
    if (pc->compressed)
        return fail(WS_ERR_UNSUPPORTED, std::string(who) + ": a compressed cloud has no PLY rows (its codebooks are shared between Gaussians)");
    const uint32_t row_len = 14u + 3u * (pc->sh_deg + 1u) * (pc->sh_deg + 1u);
    *need = (size_t)pc->num_points * row_len * sizeof(float);
    if (!d_rows && *need) return fail(WS_ERR_INVALID, std::string(who) + ": null argument");
    if (rows_bytes < *need) return fail(WS_ERR_INVALID, std::string(who) + ": rows buffer too small");
    return WS_OK;
}

int ws_pointcloud_encode_ply_rows_device(const ws_pointcloud* pc, float* d_rows, size_t rows_bytes, void* stream) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, d_rows, rows_bytes, "ws_pointcloud_encode_ply_rows_device", &need));
    return launch_ply_encode(pc->planes.get(), pc->num_points, pc->sh_deg, d_rows, static_cast<hipStream_t>(stream));
}

int ws_pointcloud_decode_ply_rows_device(ws_pointcloud* pc, const float* d_rows, size_t rows_bytes, void* stream) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, d_rows, rows_bytes, "ws_pointcloud_decode_ply_rows_device", &need));
    return launch_ply_decode(d_rows, pc->num_points, pc->sh_deg, pc->planes.get(), static_cast<hipStream_t>(stream));
}

int ws_pointcloud_encode_ply_rows(const ws_pointcloud* pc, float* rows, size_t rows_bytes) {
    size_t need = 0;
    WS_TRY(ply_rows_device_check(pc, rows, rows_bytes, "ws_pointcloud_encode_ply_rows", &need));
    const uint32_t n = pc->num_points;
    if (n == 0) return WS_OK;
    DeviceBuf<float> d_rows;  // (let go at the return, behind the stream sync)
    Stream own;               // (declared behind d_rows: destroyed in front of it)
    const char* what = "ws_pointcloud_encode_ply_rows: encode";
    hipError_t e = hipSuccess;
    int rc = alloc_as(own.create(), what);
    const hipStream_t ls = own.get();
    if (rc == WS_OK) rc = alloc_as(d_rows.alloc(need / sizeof(float)), what);
    if (rc == WS_OK) rc = launch_ply_encode(pc->planes.get(), n, pc->sh_deg, d_rows.get(), ls);
    if (rc == WS_OK && (e = hipMemcpyAsync(rows, d_rows.get(), need, hipMemcpyDeviceToHost, ls)) != hipSuccess) rc = hip_fail(e, what);
    if (ls) {
        e = hipStreamSynchronize(ls);
        if (rc == WS_OK && e != hipSuccess) rc = hip_fail(e, what);
    }
    return rc;
}

int ws_pointcloud_save_ply(const ws_pointcloud* pc, const char* path) {
    if (!pc || !path) return fail(WS_ERR_INVALID, "ws_pointcloud_save_ply: null argument");
    if (pc->compressed)
        return fail(WS_ERR_UNSUPPORTED, "ws_pointcloud_save_ply: a compressed cloud cannot be saved as a PLY (its codebooks are shared between Gaussians)");
    const uint32_t row_len = 14u + 3u * (pc->sh_deg + 1u) * (pc->sh_deg + 1u);
    std::vector<float> rows;
    try {
        rows.resize((size_t)pc->num_points * row_len);
    } catch (...) {
        return fail(WS_ERR_OOM, "ws_pointcloud_save_ply: host allocation failed");
    }
    WS_TRY(ws_pointcloud_encode_ply_rows(pc, rows.data(), rows.size() * sizeof(float)));
    ws_pointcloud_desc meta;  // the file is opened only now, with the rows in hand
    std::memset(&meta, 0, sizeof meta);
    meta.has_mip_splatting = pc->has_mip;
    meta.mip_splatting = pc->mip;
    meta.has_kernel_size = pc->has_kernel_size;
    meta.kernel_size = pc->kernel_size;
    meta.has_background_color = pc->has_background;
    std::memcpy(meta.background_color, pc->background, sizeof meta.background_color);
    return ws_ply_write(path, rows.data(), pc->num_points, pc->sh_deg, &meta);
}

int ws_pointcloud_create_subset(ws_context* ctx, const ws_pointcloud* src, const uint32_t* indices, uint32_t n, ws_pointcloud** out) {
    if (!ctx || !src || !indices || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: null argument");
    *out = nullptr;
    if (n == 0) return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: empty subset");
    for (uint32_t i = 0; i < n; ++i)
        if (indices[i] >= src->num_points || (i && indices[i] <= indices[i - 1]))
            return fail(WS_ERR_INVALID, "ws_pointcloud_create_subset: indices must be strictly ascending and below the number of points");
    std::unique_ptr<ws_pointcloud> pc(new (std::nothrow) ws_pointcloud());
    if (!pc) return fail(WS_ERR_OOM, "ws_pointcloud_create_subset: host allocation failed");
    static_cast<PointCloudMeta&>(*pc) = *src;  // bbox, centre, up, metadata, sh_deg, quantisation: verbatim
    pc->ctx = ctx;
    pc->num_points = n;
    // upload, gather and the codebook copies run on a private stream and are waited for (as ws_pointcloud_create_from_ply_rows)
    DeviceBuf<uint32_t> d_idx;  // (let go at the return, behind the stream sync)
    Stream own;               // (declared behind d_idx: destroyed in front of it)
    const char* what = "ws_pointcloud_create_subset: allocation / copy";
    int rc = d_idx.alloc(n);
    hipError_t e = hipSuccess;
    if (rc == WS_OK) rc = alloc_as(own.create(), what);
    const hipStream_t ls = own.get();
    if (rc == WS_OK && e == hipSuccess) e = hipMemcpyAsync(d_idx.get(), indices, (size_t)n * 4, hipMemcpyHostToDevice, ls);
    if (rc == WS_OK && e == hipSuccess) {
        if (!src->compressed) {
            rc = alloc_as(pc->planes.alloc((size_t)n * PC_PLANES), what);
            if (rc == WS_OK)
                rc = launch_pc_gather(reinterpret_cast<const uint32_t*>(src->planes.get()), reinterpret_cast<uint32_t*>(pc->planes.get()), d_idx.get(),
                                      src->num_points, n, PC_PLANES, 4, ls);
        } else {
            rc = alloc_as(pc->gaussians_c.alloc((size_t)n * 24), what);
            if (rc == WS_OK) rc = alloc_as(pc->sh_bytes.alloc(src->sh_bytes.count()), what);
            if (rc == WS_OK) rc = alloc_as(pc->covars.alloc(src->covars.count()), what);
            if (rc == WS_OK) e = hipMemcpyAsync(pc->sh_bytes.get(), src->sh_bytes.get(), src->sh_bytes.bytes(), hipMemcpyDeviceToDevice, ls);
            if (rc == WS_OK && e == hipSuccess) e = hipMemcpyAsync(pc->covars.get(), src->covars.get(), src->covars.bytes(), hipMemcpyDeviceToDevice, ls);
            if (rc == WS_OK && e == hipSuccess)
                rc = launch_pc_gather(reinterpret_cast<const uint32_t*>(src->gaussians_c.get()), reinterpret_cast<uint32_t*>(pc->gaussians_c.get()), d_idx.get(),
                                      src->num_points, n, 1, 6, ls);
        }
    }
    if (e != hipSuccess && rc == WS_OK) rc = hip_fail(e, what);
    if (ls) {
        const hipError_t se = hipStreamSynchronize(ls);
        if (se != hipSuccess && rc == WS_OK) rc = hip_fail(se, "ws_pointcloud_create_subset: gather");
    }
    if (rc) return rc;
    *out = pc.release();
    return WS_OK;
}

void ws_pointcloud_destroy(ws_pointcloud* pc) { delete pc; }

uint32_t ws_pointcloud_num_points(const ws_pointcloud* pc) { return pc ? pc->num_points : 0; }
uint32_t ws_pointcloud_sh_deg(const ws_pointcloud* pc) { return pc ? pc->sh_deg : 0; }
int ws_pointcloud_compressed(const ws_pointcloud* pc) { return pc && pc->compressed ? 1 : 0; }
int ws_pointcloud_bbox(const ws_pointcloud* pc, ws_aabb* out) {
    if (!pc || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_bbox: null argument");
    *out = pc->bbox;
    return WS_OK;
}
int ws_pointcloud_center(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !out) return fail(WS_ERR_INVALID, "ws_pointcloud_center: null argument");
    std::memcpy(out, pc->center, 12);
    return WS_OK;
}
int ws_pointcloud_up(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !pc->has_up) return 0;
    if (out) std::memcpy(out, pc->up, 12);
    return 1;
}
int ws_pointcloud_mip_splatting(const ws_pointcloud* pc, int32_t* out) {
    if (!pc || !pc->has_mip) return 0;
    if (out) *out = pc->mip ? 1 : 0;
    return 1;
}
int ws_pointcloud_kernel_size(const ws_pointcloud* pc, float* out) {
    if (!pc || !pc->has_kernel_size) return 0;
    if (out) *out = pc->kernel_size;
    return 1;
}
int ws_pointcloud_background_color(const ws_pointcloud* pc, float out[3]) {
    if (!pc || !pc->has_background) return 0;
    if (out) std::memcpy(out, pc->background, 12);
    return 1;
}

}  // extern "C"
