// api_attrib.cpp -- the C ABI's passes over a prepared frame's blend weights and the per-Gaussian accumulators they add to
// (include/websplat.h): contributions, values, removal effect, gradients, SH gradients, geometry gradients.  They read the
// renderer's prepared frame (api_state.h) and never make one; the four accumulators are one store (gaussian_sums.h).  The three
// gradient accumulators share one pass (ws_internal_gradient_passes: a target, named steps, one descriptor) and, with removal,
// one set of descriptor checks; the handles with per-Gaussian rows share one transpose.
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>

#include "api_state.h"
#include "contrib.h"
#include "gaussian_sums.h"
#include "geometry.h"
#include "geometry_spread.h"
#include "gradient.h"
#include "sh_gradient.h"
#include "values.h"
using namespace ws;

// ---- the store (gaussian_sums.h) -------------------------------------------------------------------------------------------------
int GaussianSums::reset(GaussianSums* s, const char* who, hipStream_t stream) {
    if (!s) return fail(WS_ERR_INVALID, std::string(who) + ": null accumulator");
    WS_HIP(hipMemsetAsync(s->sums.get(), 0, s->sums.bytes(), stream));
    s->frames = 0;
    s->last_stream = stream;
    return WS_OK;
}

int GaussianSums::download_words(GaussianSums* s, const char* who, uint32_t capacity, bool wanted, void* dst) {
    if (!s) return fail(WS_ERR_INVALID, std::string(who) + ": null accumulator");
    if (wanted && capacity < s->num_points) return fail(WS_ERR_INVALID, std::string(who) + ": capacity smaller than the number of points");
    WS_HIP(hipStreamSynchronize(s->last_stream));
    return dst ? copy_d2h(dst, s->sums.get(), s->sums.bytes(), s->last_stream) : WS_OK;
}

int GaussianSums::merge_words(GaussianSums* s, const char* who_c, uint32_t n, const void* host_words, const Merge& merge) {
    const std::string who(who_c);
    if (!s) return fail(WS_ERR_INVALID, who + ": null accumulator");
    if (n < s->num_points) return fail(WS_ERR_INVALID, who + ": fewer values than the accumulator has points");
    if (!host_words && !merge) return WS_OK;
    DeviceBuf<unsigned long long> d_words;  // (let go at the return, behind the stream sync)
    hipStream_t stream = s->last_stream;
    int rc = host_words ? d_words.alloc(s->sums.count()) : WS_OK;
    if (rc == WS_OK && host_words) {
        const hipError_t e = hipMemcpyAsync(d_words.get(), host_words, s->sums.bytes(), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) rc = hip_fail(e, (who + ": upload").c_str());
    }
    if (rc == WS_OK) rc = merge ? merge(d_words.get(), stream) : launch_grad_merge(s->sums.get(), d_words.get(), s->sums.count(), stream);
    if (hipStreamSynchronize(stream) != hipSuccess && rc == WS_OK) rc = fail(WS_ERR_HIP, who + ": stream sync failed");
    return rc;
}

// How all three are created: `init` allocates what the handle has and resets it on the NULL stream; the device sync waits for that.
// unsupported: what the entry point's own arguments ask for that the library has not, or nullptr
template <typename H, typename Init>
static int create_sums(const char* who_c, ws_context* ctx, uint32_t num_points, H** out, Init&& init, const char* unsupported = nullptr) {
    const std::string who(who_c);
    if (!ctx || !out) return fail(WS_ERR_INVALID, who + ": null argument");
    *out = nullptr;
    if (num_points == 0) return fail(WS_ERR_INVALID, who + ": no points");
    if (unsupported) return fail(WS_ERR_UNSUPPORTED, who + ": " + unsupported);
    std::unique_ptr<H, SyncedDelete> h(new (std::nothrow) H());
    if (!h) return fail(WS_ERR_OOM, who + ": host allocation failed");
    h->ctx = ctx;
    h->num_points = num_points;
    WS_TRY(init(h.get()));
    if (hipDeviceSynchronize() != hipSuccess) return fail(WS_ERR_HIP, who + ": device sync failed");
    *out = h.release();
    return WS_OK;
}

// ---- a pass over the prepared frame ------------------------------------------------------------------------------------------------
// What a launch over the prepared frame's weights (k_contrib, k_values, k_removal_base, k_removal) reads of the renderer
static FrameLists frame_lists(const ws_renderer* r) {
    FrameLists f;
    f.splats = r->scratch.splats.get();
    f.entry_vals = r->frame.arrays.entries;
    f.tile_ranges = r->scratch.tile_ranges();
    f.src_index = r->scratch.src_index.get();
    f.width = r->vw;
    f.height = r->vh;
    f.tiles_x = r->plan.tiles_x;
    f.tiles_y = r->plan.tiles_y;
    f.qw = r->ctx->tile_qw;
    f.qh = r->ctx->tile_qh;
    f.counters = r->scratch.counters();
    f.sticky = r->sticky.get();
    f.demand_mailbox = r->mailbox.dev();
    return f;
}

// ... and whether the renderer holds such a frame for `pc`.  points_match: the caller's own per-Gaussian array fits the cloud.
static int check_weights_frame(const ws_renderer* r, const ws_pointcloud* pc, const std::string& who, bool points_match,
                               const char* points_text) {
    if (r->ctx->debug_cut) return fail(WS_ERR_UNSUPPORTED, who + ": the context stops its frames early (debug_cut)");
    if (!points_match) return fail(WS_ERR_INVALID, who + ": " + points_text);
    if (!r->frame.prepared || r->frame.pc != pc) return fail(WS_ERR_STATE, who + ": prepare() was not called for this point cloud");
    if (!r->frame.contrib) return fail(WS_ERR_STATE, who + ": needs ws_renderer_enable_contrib before prepare()");
    return WS_OK;
}

// A caller's plane of 4-B values (`what`: "plane" | "winner"; nullptr: nothing to judge).  r == nullptr: by itself, pointer and
// pitch; else against r's prepared frame, the pitch.  who: the text's prefix.
static int check_plane(const ws_renderer* r, const std::string& who, const char* what, const void* ptr, size_t pitch) {
    if (ptr && !r && (pitch % 4 != 0 || reinterpret_cast<uintptr_t>(ptr) % 4 != 0))
        return fail(WS_ERR_INVALID, who + ": " + what + " pointer and row pitch must be multiples of 4");
    if (ptr && r && pitch < (size_t)r->vw * 4) return fail(WS_ERR_INVALID, who + ": " + what + " row pitch below 4 x the viewport's width");
    return WS_OK;
}
static int check_plane_view(const ws_renderer* r, const std::string& who, const ws_plane_view* v) {
    if (!v) return WS_OK;
    if (!r && (!std::isfinite(v->scale) || !std::isfinite(v->bias))) return fail(WS_ERR_INVALID, who + ": scale and bias must be finite");
    return check_plane(r, who, "plane", v->d_values, v->row_pitch_bytes);
}

// The bracket of a launch over the prepared frame: the timers' begin before it; behind it, with its status, the mark and the
// streams to wait for.  acc: the accumulator the launch added a frame to, or nullptr
static KernelMarks* launch_begin(ws_renderer* r, hipStream_t stream) {
    KernelMarks* km = r->marks.active ? &r->marks : nullptr;
    if (km) km->begin(stream, false);
    return km;
}
static int launch_done(int rc, ws_renderer* r, GaussianSums* acc, hipStream_t stream, KernelMarks* km, const char* mark) {
    if (rc) return rc;
    km_mark(km, mark);
    if (acc) acc->launched(stream);
    r->last_stream = stream;
    return WS_OK;
}

// Removal's launch parameters, for ws_renderer_accumulate_removal and for the gradient pass, whose first step is removal's pass 1.
// The base plane (F, T_end) is the caller's, or the renderer's scratch, grown on demand.
static int removal_params(ws_renderer* r, const float background[3], float* d_base, size_t pitch, float scale, int kind, const Accum& acc,
                          RemovalParams* rp) {
    if (!d_base && !r->scratch.removal_base.get()) {  // (one viewport per scratch: the plane is freed with it)
        WS_HIP(hipDeviceSynchronize());
        WS_TRY(r->scratch.removal_base.alloc(r->scratch.layout.removal_base));
    }
    rp->frame = frame_lists(r);
    rp->base = d_base ? reinterpret_cast<float4*>(d_base) : r->scratch.removal_base.get();
    rp->base_pitch = d_base ? pitch : (size_t)r->vw * 16;
    for (int i = 0; i < 3; ++i) rp->background[i] = background[i];
    rp->scale = scale;
    rp->kind = kind;
    rp->acc = acc;
    return WS_OK;
}

// The accumulator as the kernels' argument: the plain sums (plane == nullptr) or the weighted ones
static Accum accum_arg(const ws_contrib* c, const ws_plane_view* plane) {
    if (!plane) return {c->sums.get(), c->max_bits.get(), nullptr, 0, 1.0f, 0.0f};
    return {c->sums.get(), c->max_bits.get(), plane->d_values, plane->row_pitch_bytes, plane->scale, plane->bias};
}

// One attribution launch over the prepared frame: the plain sums (plane == nullptr) or the weighted ones
static int accumulate_frame(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, const ws_plane_view* plane, void* stream_v,
                            const char* who_c) {
    const std::string who(who_c);
    int rc = check_weights_frame(r, pc, who, c->num_points == pc->num_points, "the accumulator was created for another number of points");
    if (rc == WS_OK) rc = check_plane_view(r, who, plane);
    if (rc) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const ContribParams cp{frame_lists(r), accum_arg(c, plane)};
    KernelMarks* km = launch_begin(r, stream);
    return launch_done(launch_contrib(cp, stream), r, c, stream, km, plane ? "k_contrib_weighted" : "k_contrib");
}

static_assert(WS_GRAD_CHANNELS == GRAD_CHANNELS, "the ABI's channel count is the kernel's");

// What ws_renderer_accumulate_removal and the gradient pass refuse in the same words.  Each entry point calls them in its own
// order: the descriptor alone, then the handles, then the descriptor against the frame.
static int check_scale(const std::string& who, const char* name, float v) {
    return std::isfinite(v) && v > 0.0f ? (int)WS_OK : fail(WS_ERR_INVALID, who + ": " + name + " must be finite and above 0");
}
static int check_background(const std::string& who, const float bg[3]) {
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(bg[i])) return fail(WS_ERR_INVALID, who + ": background must be finite");
    return WS_OK;
}
// A caller's plane of float4, d_<name> with <name>_pitch_bytes (nullptr: nothing to judge).  r == nullptr: by itself, pointer and
// pitch; else against r's prepared frame, the pitch.
static int check_plane16(const ws_renderer* r, const std::string& who, const std::string& name, const void* ptr, size_t pitch) {
    if (ptr && !r && (pitch % 16 != 0 || reinterpret_cast<uintptr_t>(ptr) % 16 != 0))
        return fail(WS_ERR_INVALID, who + ": d_" + name + ": pointer and " + name + "_pitch_bytes must be multiples of 16");
    if (ptr && r && pitch < (size_t)r->vw * 16) return fail(WS_ERR_INVALID, who + ": d_" + name + ": " + name + "_pitch_bytes below 16 x the viewport's width");
    return WS_OK;
}

// The timers' label of a gradient pass, by the target's kind and the steps: the kernels that ran, joined by '+'.  String literals
// (KernelMarks::mark keeps the pointer), and scripts/*_cost.py select on them.  A ws_grad has no spread.
static const char* const GRAD_LABELS[3][GRAD_ALL + 1] = {
    {"", "k_removal_base", "k_gradient", "k_removal_base+k_gradient", "", "k_removal_base", "k_gradient", "k_removal_base+k_gradient"},
    {"", "k_removal_base", "k_gradient", "k_removal_base+k_gradient", "k_sh_spread", "k_removal_base+k_sh_spread", "k_gradient+k_sh_spread",
     "k_removal_base+k_gradient+k_sh_spread"},
    {"", "k_removal_base", "k_geometry", "k_removal_base+k_geometry", "k_geom_spread", "k_removal_base+k_geom_spread", "k_geometry+k_geom_spread",
     "k_removal_base+k_geometry+k_geom_spread"}};

static const char* const GRAD_ENTRY[3] = {"ws_renderer_accumulate_gradient", "ws_renderer_accumulate_sh_gradient",
                                          "ws_renderer_accumulate_geometry_gradient"};

// One sequence for the three gradient accumulators (GradTarget, GradSteps, GradDesc: gaussian_sums.h).  The descriptor is judged by
// itself first, then the handles, then the descriptor against the frame; only then the launches: GRAD_BASE is removal's pass 1;
// GRAD_SUMS the walk, k_gradient into a ws_grad's sums or a ws_shgrad's scratch, k_geometry into a ws_geomgrad's scratch;
// GRAD_SPREAD the target's own kernel from its scratch into its sums (without it the sums stay in the scratch:
// ws_debug_geometry_stage_a).  who: the entry point, for messages; nullptr: the target's own ws_renderer_accumulate_* one.
int ws_internal_gradient_passes(const char* who_c, ws_renderer* r, const ws_pointcloud* pc, const GradTarget& t, const GradDesc& d, void* stream_v,
                                unsigned steps) {
    const std::string who(who_c ? who_c : GRAD_ENTRY[t.kind]);
    ws_shgrad* const sh = t.sh();
    ws_geomgrad* const geo = t.geo();
    WS_TRY(check_scale(who, "scale", d.scale));
    WS_TRY(check_scale(who, t.kind == GRAD_GEOMETRY ? "geometry_scale" : "opacity_scale", d.second_scale));
    WS_TRY(check_background(who, d.background));
    if (!d.d_grad) return fail(WS_ERR_INVALID, who + ": null d_grad");
    WS_TRY(check_plane16(nullptr, who, "grad", d.d_grad, d.grad_pitch_bytes));
    WS_TRY(check_plane16(nullptr, who, "base", d.d_base, d.base_pitch_bytes));
    if (!r || !pc || !t.acc) return fail(WS_ERR_INVALID, who + ": null argument");
    WS_TRY(check_weights_frame(r, pc, who, t.acc->num_points == pc->num_points, "the accumulator was created for another number of points"));
    if (sh && pc->compressed) return fail(WS_ERR_UNSUPPORTED, who + ": a compressed cloud has no SH gradients (its codebooks are shared between Gaussians)");
    if (geo && pc->compressed) return fail(WS_ERR_UNSUPPORTED, who + ": a compressed cloud has no geometry gradients (its covariances are a codebook shared between Gaussians)");
    if (sh && sh->sh_deg != pc->sh_deg) return fail(WS_ERR_INVALID, who + ": the accumulator was created for another SH degree");
    WS_TRY(check_plane16(r, who, "grad", d.d_grad, d.grad_pitch_bytes));
    WS_TRY(check_plane16(r, who, "base", d.d_base, d.base_pitch_bytes));
    RemovalParams rp;  // (pass 1 reads neither scale, kind nor accumulator)
    WS_TRY(removal_params(r, d.background, d.d_base, d.base_pitch_bytes, 1.0f, WS_ERROR_SQ, Accum{nullptr, nullptr, nullptr, 0, 1.0f, 0.0f}, &rp));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    KernelMarks* km = launch_begin(r, stream);
    int rc = (steps & GRAD_BASE) ? launch_removal_base(rp, stream) : WS_OK;
    // (the two walks' params: frame, base, base_pitch, grad, grad_pitch, scale, the second scale under its own name, sums)
    const float4* grad = reinterpret_cast<const float4*>(d.d_grad);
    if (rc == WS_OK && (steps & GRAD_SUMS) && !geo)
        rc = launch_gradient(GradientParams{rp.frame, rp.base, rp.base_pitch, grad, d.grad_pitch_bytes, d.scale, /*opacity_scale*/ d.second_scale,
                                            sh ? sh->scratch.get() : t.acc->sums.get()}, stream);
    if (rc == WS_OK && (steps & GRAD_SUMS) && geo)
        rc = launch_geometry(GeometryParams{rp.frame, rp.base, rp.base_pitch, grad, d.grad_pitch_bytes, d.scale, /*geometry_scale*/ d.second_scale,
                                            geo->scratch.get()}, stream);
    if (rc == WS_OK && (steps & GRAD_SPREAD) && sh) {
        ShSpreadParams sp;
        sp.planes = pc->planes.get();
        sp.scratch = sh->scratch.get();
        sp.sums = sh->sums.get();
        sp.n = sh->num_points;
        sp.ncoef = sh->ncoef;
        sp.nact = sh_active_coefs(r->frame.max_sh_deg, sh->sh_deg);
        for (int i = 0; i < 3; ++i) sp.cam[i] = r->frame.cam_pos[i];
        rc = launch_sh_spread(sp, stream);
    }
    if (rc == WS_OK && (steps & GRAD_SPREAD) && geo) {
        GeomSpreadParams sp{};
        sp.planes = pc->planes.get();
        sp.splats = rp.frame.splats;
        sp.src_index = rp.frame.src_index;
        sp.counters = rp.frame.counters;
        sp.scratch = geo->scratch.get();
        sp.sums = geo->sums.get();
        sp.n = geo->num_points;
        sp.frame.cam = r->frame.cam;
        sp.frame.rs = r->frame.settings;
        sp.frame.geometry_scale = d.second_scale;
        rc = launch_geom_spread(sp, stream);
    }
    // (the frame is counted by the step that completes it)
    const bool counted = steps & (t.kind == GRAD_COLOUR ? GRAD_SUMS : GRAD_SPREAD);
    return launch_done(rc, r, counted ? t.acc : nullptr, stream, km, GRAD_LABELS[t.kind][steps & GRAD_ALL]);
}

// An ABI descriptor under the pass's names, read through its own: P is ws_gradient_params with its opacity_scale, or
// ws_geometry_params with its geometry_scale.  What needs no more than the descriptor's own words is refused here, first.
template <typename P>
static int gradient_entry(const char* who, ws_renderer* r, const ws_pointcloud* pc, const GradTarget& t, const P* p, float P::*second_scale,
                          void* stream, unsigned steps) {
    if (!p) return fail(WS_ERR_INVALID, std::string(who) + ": null params");
    if (p->reserved0 | p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]) return fail(WS_ERR_INVALID, std::string(who) + ": reserved words must be zero");
    GradDesc d;
    for (int i = 0; i < 3; ++i) d.background[i] = p->background[i];
    d.scale = p->scale;
    d.second_scale = p->*second_scale;
    d.d_grad = p->d_grad;
    d.grad_pitch_bytes = p->grad_pitch_bytes;
    d.d_base = p->d_base;
    d.base_pitch_bytes = p->base_pitch_bytes;
    return ws_internal_gradient_passes(who, r, pc, t, d, stream, steps);
}

// The host's transposes under ws_shgrad and ws_geomgrad.  The device keeps one plane per element, [elements][n] 8-B words; the
// caller's arrays are rows per Gaussian.  A column: the caller's array of n rows of `width` words (nullptr: not given) and the
// first of the `width` planes they are.
struct RowColumn {
    const void* rows;
    size_t first, width;
};
using RowColumns = std::initializer_list<RowColumn>;
static bool any_rows(RowColumns cols) {
    for (const RowColumn& c : cols)
        if (c.rows) return true;
    return false;
}
// to_rows: planes -> the caller's arrays (which are then not const: ws_*_download); else the caller's arrays -> planes
static void transpose_rows(uint64_t* planes, size_t n, RowColumns cols, bool to_rows) {
    for (const RowColumn& c : cols) {
        char* rows = static_cast<char*>(const_cast<void*>(c.rows));
        for (size_t e = 0; rows && e < c.width; ++e)
            for (size_t i = 0; i < n; ++i) {
                char* row = rows + (i * c.width + e) * 8;  // (bytes: the rows are int64, double or uint64)
                uint64_t* word = planes + (c.first + e) * n + i;
                to_rows ? std::memcpy(row, word, 8) : std::memcpy(word, row, 8);
            }
    }
}
// Through one staging array of every word, sized by the accumulator, so it may be made before the store has judged the handle
// and the capacity.
static int download_rows(GaussianSums* g, const char* who, uint32_t capacity, RowColumns cols) {
    std::unique_ptr<uint64_t[]> st;
    if (g && any_rows(cols)) {
        st.reset(new (std::nothrow) uint64_t[g->sums.count()]);
        if (!st) return fail(WS_ERR_OOM, std::string(who) + ": host allocation failed");
    }
    WS_TRY(GaussianSums::download_words(g, who, capacity, st != nullptr, st.get()));
    if (st) transpose_rows(st.get(), g->num_points, cols, true);
    return WS_OK;
}
// merge: the handle's own, used when there is something to add (an empty one: the store's k_grad_merge)
static int add_rows(GaussianSums* g, const char* who, uint32_t n_rows, RowColumns cols, const GaussianSums::Merge& merge) {
    std::unique_ptr<uint64_t[]> st;
    if (g && n_rows >= g->num_points && any_rows(cols)) {  // (else the store refuses, or there is nothing to add)
        st.reset(new (std::nothrow) uint64_t[g->sums.count()]());  // (zeros where a pointer is NULL: 0, +0.0)
        if (!st) return fail(WS_ERR_OOM, std::string(who) + ": host allocation failed");
        transpose_rows(st.get(), g->num_points, cols, false);
    }
    return GaussianSums::merge_words(g, who, n_rows, st.get(), st ? merge : GaussianSums::Merge());
}

extern "C" {

// ---- ws_contrib: the store, and a plane of maxima that is its own
int ws_contrib_create(ws_context* ctx, uint32_t num_points, ws_contrib** out) {
    return create_sums("ws_contrib_create", ctx, num_points, out, [num_points](ws_contrib* c) {
        WS_TRY(c->sums.alloc(num_points));
        WS_TRY(c->max_bits.alloc(num_points));
        return ws_contrib_reset(c, nullptr);
    });
}

void ws_contrib_destroy(ws_contrib* c) { SyncedDelete()(c); }

int ws_contrib_reset(ws_contrib* c, void* stream_v) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    WS_TRY(GaussianSums::reset(c, "ws_contrib_reset", stream));
    WS_HIP(hipMemsetAsync(c->max_bits.get(), 0, c->max_bits.bytes(), stream));
    return WS_OK;
}

uint32_t ws_contrib_num_points(const ws_contrib* c) { return c ? c->num_points : 0u; }
uint32_t ws_contrib_frames(const ws_contrib* c) { return c ? c->frames : 0u; }

int ws_contrib_download(ws_contrib* c, uint32_t capacity, uint64_t* sum_q32, float* max_weight) {
    WS_TRY(GaussianSums::download_words(c, "ws_contrib_download", capacity, sum_q32 || max_weight, sum_q32));
    return max_weight ? copy_d2h(max_weight, c->max_bits.get(), c->max_bits.bytes(), c->last_stream) : WS_OK;
}

// (one launch merges both planes: the maxima are uploaded beside the sums and go through launch_contrib_merge with them)
int ws_contrib_add(ws_contrib* c, const uint64_t* sum_q32, const float* max_weight, uint32_t n) {
    DeviceBuf<uint32_t> d_max;  // (let go at the return, behind merge_words' stream sync)
    const GaussianSums::Merge both = [&](const unsigned long long* d_sum, hipStream_t stream) {
        if (max_weight) {
            WS_TRY(d_max.alloc(c->num_points));
            const hipError_t e = hipMemcpyAsync(d_max.get(), max_weight, d_max.bytes(), hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return hip_fail(e, "ws_contrib_add: upload");
        }
        return launch_contrib_merge(c->sums.get(), c->max_bits.get(), d_sum, d_max.get(), c->num_points, stream);
    };
    return GaussianSums::merge_words(c, "ws_contrib_add", n, sum_q32, sum_q32 || max_weight ? both : GaussianSums::Merge());
}

int ws_renderer_enable_contrib(ws_renderer* r, int enable) {
    if (!r) return fail(WS_ERR_INVALID, "ws_renderer_enable_contrib: null renderer");
    // Only K1's src_index pointer changes (a kernel argument the frame graph's update rewrites anyway); the binning tile and
    // the blend's form stay what they are, unlike capture.  Off: the frame at hand no longer answers accumulate_contrib.
    r->contrib = enable != 0;
    if (!r->contrib) r->frame.contrib = false;
    return WS_OK;
}

int ws_renderer_accumulate_contrib(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, void* stream_v) {
    if (!r || !pc || !c) return fail(WS_ERR_INVALID, "ws_renderer_accumulate_contrib: null argument");
    return accumulate_frame(r, pc, c, nullptr, stream_v, "ws_renderer_accumulate_contrib");
}

int ws_renderer_accumulate_weighted(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, const ws_plane_view* plane, void* stream_v) {
    if (!r || !pc || !c || !plane || !plane->d_values) return fail(WS_ERR_INVALID, "ws_renderer_accumulate_weighted: null argument");
    if (const int rc = check_plane_view(nullptr, "ws_renderer_accumulate_weighted", plane)) return rc;
    return accumulate_frame(r, pc, c, plane, stream_v, "ws_renderer_accumulate_weighted");
}

// The forward operator of the attribution pass: the caller's per-Gaussian values through the prepared frame's weights, to planes.
// The descriptors are judged by themselves first, then the handles, then the descriptors against the frame; only then a launch.
int ws_renderer_render_values(ws_renderer* r, const ws_pointcloud* pc, const ws_values_view* values, const ws_value_targets* out,
                              void* stream_v) {
    const std::string who("ws_renderer_render_values");
    if (!out) return fail(WS_ERR_INVALID, who + ": null targets");
    for (uint32_t w : out->reserved)
        if (w != 0) return fail(WS_ERR_INVALID, who + ": reserved words must be zero");
    const uint32_t channels = values ? values->channels : 0u;
    if (values) {
        if (!values->d_values) return fail(WS_ERR_INVALID, who + ": null d_values");
        if (channels == 0 || channels > 4) return fail(WS_ERR_INVALID, who + ": channels must be 1..4");
        if (values->stride_bytes < (size_t)4 * channels || values->stride_bytes % 4 != 0)
            return fail(WS_ERR_INVALID, who + ": values stride below 4 x channels or not a multiple of 4");
        if (reinterpret_cast<uintptr_t>(values->d_values) % 4 != 0) return fail(WS_ERR_INVALID, who + ": values pointer not 4-B aligned");
    }
    bool any = out->winner != nullptr;
    for (uint32_t c = 0; c < 4; ++c) {
        if (!out->plane[c]) continue;
        if (c >= channels) return fail(WS_ERR_INVALID, who + ": a plane at or above the number of channels");
        if (const int rc = check_plane(nullptr, who, "plane", out->plane[c], out->pitch[c])) return rc;
        any = true;
    }
    if (const int rc = check_plane(nullptr, who, "winner", out->winner, out->winner_pitch)) return rc;
    if (!any) return fail(WS_ERR_INVALID, who + ": no output plane");
    if (!r || !pc) return fail(WS_ERR_INVALID, who + ": null argument");
    const int state = check_weights_frame(r, pc, who, !values || values->num_points == pc->num_points, "the values were laid out for another number of points");
    if (state) return state;
    for (uint32_t c = 0; c < 4; ++c)
        if (const int rc = check_plane(r, who, "plane", out->plane[c], out->pitch[c])) return rc;
    if (const int rc = check_plane(r, who, "winner", out->winner, out->winner_pitch)) return rc;
    ValuesParams vp;
    vp.frame = frame_lists(r);
    vp.values = values ? values->d_values : nullptr;
    vp.stride = values ? values->stride_bytes : 0;
    vp.channels = channels;
    for (uint32_t c = 0; c < 4; ++c) {
        vp.plane[c] = out->plane[c];
        vp.pitch[c] = out->pitch[c];
    }
    vp.winner = out->winner;
    vp.winner_pitch = out->winner_pitch;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    KernelMarks* km = launch_begin(r, stream);
    return launch_done(launch_values(vp, stream), r, nullptr, stream, km, "k_values");
}

// What deleting each Gaussian alone would do to the prepared frame (websplat.h "Removal effect"; removal.h).  The descriptor is
// judged by itself first, then the handles, then the descriptor against the frame; only then the two launches.
int ws_renderer_accumulate_removal(ws_renderer* r, const ws_pointcloud* pc, ws_contrib* c, const ws_removal_params* p, void* stream_v) {
    const std::string who("ws_renderer_accumulate_removal");
    if (!p) return fail(WS_ERR_INVALID, who + ": null params");
    for (uint32_t w : p->reserved)
        if (w != 0) return fail(WS_ERR_INVALID, who + ": reserved words must be zero");
    if (p->kind == WS_ERROR_DSSIM) return fail(WS_ERR_INVALID, who + ": kind WS_ERROR_DSSIM has no removal effect (sq or abs)");
    if (p->kind != WS_ERROR_SQ && p->kind != WS_ERROR_ABS) return fail(WS_ERR_INVALID, who + ": unknown kind");
    WS_TRY(check_scale(who, "scale", p->scale));
    WS_TRY(check_background(who, p->background));
    if (p->weight && !p->weight->d_values) return fail(WS_ERR_INVALID, who + ": weight: null d_values");
    WS_TRY(check_plane_view(nullptr, who + ": weight", p->weight));
    WS_TRY(check_plane16(nullptr, who, "base", p->d_base, p->base_pitch_bytes));
    if (!r || !pc || !c) return fail(WS_ERR_INVALID, who + ": null argument");
    WS_TRY(check_weights_frame(r, pc, who, c->num_points == pc->num_points, "the accumulator was created for another number of points"));
    WS_TRY(check_plane_view(r, who + ": weight", p->weight));
    WS_TRY(check_plane16(r, who, "base", p->d_base, p->base_pitch_bytes));
    RemovalParams rp;
    WS_TRY(removal_params(r, p->background, p->d_base, p->base_pitch_bytes, p->scale, p->kind, accum_arg(c, p->weight), &rp));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    KernelMarks* km = launch_begin(r, stream);
    return launch_done(launch_removal(rp, stream), r, c, stream, km, "k_removal_base+k_removal");
}

// ---- ws_grad: the store as it is
int ws_grad_create(ws_context* ctx, uint32_t num_points, ws_grad** out) {
    return create_sums("ws_grad_create", ctx, num_points, out, [num_points](ws_grad* g) {
        WS_TRY(g->sums.alloc((size_t)num_points * GRAD_CHANNELS));
        return ws_grad_reset(g, nullptr);
    });
}

void ws_grad_destroy(ws_grad* g) { SyncedDelete()(g); }
int ws_grad_reset(ws_grad* g, void* stream) { return GaussianSums::reset(g, "ws_grad_reset", static_cast<hipStream_t>(stream)); }

uint32_t ws_grad_num_points(const ws_grad* g) { return g ? g->num_points : 0u; }
uint32_t ws_grad_frames(const ws_grad* g) { return g ? g->frames : 0u; }

int ws_grad_download(ws_grad* g, uint32_t capacity, int64_t* q32) {
    return GaussianSums::download_words(g, "ws_grad_download", capacity, q32 != nullptr, q32);
}

int ws_grad_add(ws_grad* g, const int64_t* q32, uint32_t n) { return GaussianSums::merge_words(g, "ws_grad_add", n, q32); }

int ws_renderer_accumulate_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_grad* g, const ws_gradient_params* p, void* stream) {
    return gradient_entry("ws_renderer_accumulate_gradient", r, pc, g, p, &ws_gradient_params::opacity_scale, stream, GRAD_ALL);
}

// ---- ws_shgrad: one plane of the store per element, a frame's scratch, and the host's transposes
int ws_shgrad_create(ws_context* ctx, uint32_t num_points, uint32_t sh_deg, ws_shgrad** out) {
    return create_sums("ws_shgrad_create", ctx, num_points, out, [num_points, sh_deg](ws_shgrad* g) {
        g->sh_deg = sh_deg;
        g->ncoef = (sh_deg + 1) * (sh_deg + 1);
        WS_TRY(g->sums.alloc(((size_t)3 * g->ncoef + 1) * num_points));
        WS_TRY(g->scratch.alloc((size_t)num_points * GRAD_CHANNELS));
        WS_HIP(hipMemsetAsync(g->scratch.get(), 0, g->scratch.bytes(), nullptr));
        return ws_shgrad_reset(g, nullptr);
    }, sh_deg > 3 ? "sh_deg > 3" : nullptr);
}

void ws_shgrad_destroy(ws_shgrad* g) { SyncedDelete()(g); }
// (the scratch is zero between the calls by k_sh_spread's own doing; a reset leaves it alone)
int ws_shgrad_reset(ws_shgrad* g, void* stream) { return GaussianSums::reset(g, "ws_shgrad_reset", static_cast<hipStream_t>(stream)); }

uint32_t ws_shgrad_num_points(const ws_shgrad* g) { return g ? g->num_points : 0u; }
uint32_t ws_shgrad_sh_deg(const ws_shgrad* g) { return g ? g->sh_deg : 0u; }
uint32_t ws_shgrad_frames(const ws_shgrad* g) { return g ? g->frames : 0u; }

// rows of 3 ncoef words per Gaussian, and the opacity's plane as it is
int ws_shgrad_download(ws_shgrad* g, uint32_t capacity, int64_t* q_sh, int64_t* q_opacity) {
    const size_t el = g ? (size_t)3 * g->ncoef : 0;
    return download_rows(g, "ws_shgrad_download", capacity, {{q_sh, 0, el}, {q_opacity, el, 1}});
}

int ws_shgrad_add(ws_shgrad* g, const int64_t* q_sh, const int64_t* q_opacity, uint32_t n_rows) {
    const size_t el = g ? (size_t)3 * g->ncoef : 0;
    return add_rows(g, "ws_shgrad_add", n_rows, {{q_sh, 0, el}, {q_opacity, el, 1}}, GaussianSums::Merge());
}

// ... and ws_renderer_accumulate_gradient's launches into the accumulator's scratch, then k_sh_spread
int ws_renderer_accumulate_sh_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_shgrad* g, const ws_gradient_params* p, void* stream) {
    return gradient_entry("ws_renderer_accumulate_sh_gradient", r, pc, g, p, &ws_gradient_params::opacity_scale, stream, GRAD_ALL);
}

// ---- ws_geomgrad: ten f64 planes and a count plane of the store, a frame's scratch, and the host's transposes
int ws_geomgrad_create(ws_context* ctx, uint32_t num_points, ws_geomgrad** out) {
    return create_sums("ws_geomgrad_create", ctx, num_points, out, [num_points](ws_geomgrad* g) {
        WS_TRY(g->sums.alloc((size_t)GEOM_ELEMENTS * num_points));
        WS_TRY(g->scratch.alloc((size_t)num_points * GEOM_SCRATCH));
        WS_HIP(hipMemsetAsync(g->scratch.get(), 0, g->scratch.bytes(), nullptr));
        return ws_geomgrad_reset(g, nullptr);
    });
}

void ws_geomgrad_destroy(ws_geomgrad* g) { SyncedDelete()(g); }
// (the scratch is zero between the calls by k_geom_spread's own doing; a reset leaves it alone.  All-zero words are 0.0 and 0.)
int ws_geomgrad_reset(ws_geomgrad* g, void* stream) { return GaussianSums::reset(g, "ws_geomgrad_reset", static_cast<hipStream_t>(stream)); }

uint32_t ws_geomgrad_num_points(const ws_geomgrad* g) { return g ? g->num_points : 0u; }
uint32_t ws_geomgrad_frames(const ws_geomgrad* g) { return g ? g->frames : 0u; }

// rows of 3 and of 6 f64 per Gaussian, then the two planes that are per Gaussian as they are
int ws_geomgrad_download(ws_geomgrad* g, uint32_t capacity, double* position, double* covariance, double* screen_norm, uint64_t* seen) {
    return download_rows(g, "ws_geomgrad_download", capacity, {{position, 0, 3}, {covariance, 3, 6}, {screen_norm, 9, 1}, {seen, 10, 1}});
}

int ws_geomgrad_add(ws_geomgrad* g, const double* position, const double* covariance, const double* screen_norm, const uint64_t* seen, uint32_t n_rows) {
    const GaussianSums::Merge merge = [g](const unsigned long long* d_words, hipStream_t stream) {
        return launch_geom_merge(g->sums.get(), d_words, g->num_points, stream);
    };
    return add_rows(g, "ws_geomgrad_add", n_rows, {{position, 0, 3}, {covariance, 3, 6}, {screen_norm, 9, 1}, {seen, 10, 1}}, merge);
}

int ws_renderer_accumulate_geometry_gradient(ws_renderer* r, const ws_pointcloud* pc, ws_geomgrad* g, const ws_geometry_params* p, void* stream) {
    return gradient_entry("ws_renderer_accumulate_geometry_gradient", r, pc, g, p, &ws_geometry_params::geometry_scale, stream, GRAD_ALL);
}

int ws_debug_geometry_stage_a(ws_renderer* r, const ws_pointcloud* pc, ws_geomgrad* g, const ws_geometry_params* p, void* stream) {
    WS_TRY(gradient_entry("ws_debug_geometry_stage_a", r, pc, g, p, &ws_geometry_params::geometry_scale, stream, GRAD_BASE | GRAD_SUMS));
    g->last_stream = static_cast<hipStream_t>(stream);  // (no frame added, but the scratch is read back behind this stream)
    return WS_OK;
}

int ws_debug_geomgrad_scratch(ws_geomgrad* g, uint32_t capacity, int64_t* q5) {
    if (!g || !q5) return fail(WS_ERR_INVALID, "ws_debug_geomgrad_scratch: null argument");
    if (capacity < g->num_points) return fail(WS_ERR_INVALID, "ws_debug_geomgrad_scratch: capacity smaller than the number of points");
    WS_HIP(hipStreamSynchronize(g->last_stream));
    return copy_d2h(q5, g->scratch.get(), g->scratch.bytes(), g->last_stream);
}

int ws_debug_geomgrad_clear_scratch(ws_geomgrad* g, void* stream) {
    if (!g) return fail(WS_ERR_INVALID, "ws_debug_geomgrad_clear_scratch: null accumulator");
    WS_HIP(hipMemsetAsync(g->scratch.get(), 0, g->scratch.bytes(), static_cast<hipStream_t>(stream)));
    g->last_stream = static_cast<hipStream_t>(stream);
    return WS_OK;
}

}  // extern "C"
