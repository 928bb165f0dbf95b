// api_refit.cpp -- the C ABI's refit of a resident cloud (include/websplat.h "Refitting colour and opacity", "SH gradients";
// refit.hip): Adam steps on the colours, the opacities and the rest coefficients from a ws_grad's or a
// ws_shgrad's sums (gaussian_sums.h).
#include <cmath>
#include <cstddef>
#include <memory>
#include <new>
#include <utility>

#include "api_state.h"
#include "gaussian_sums.h"
#include "refit.h"
using namespace ws;

struct ws_refit {
    ws_context* ctx = nullptr;
    const ws_pointcloud* pc = nullptr;   // the cloud the masters were widened from: the only one a step accepts
    const uint4* planes = nullptr;       // (and its planes: a later cloud at the same address is another cloud)
    uint32_t num_points = 0;
    DeviceBuf<float4> master, m, v;      // [num_points] each
    uint32_t steps = 0;
    double p1 = 1.0, p2 = 1.0;           // beta1^steps, beta2^steps
    hipStream_t last_stream = nullptr;
    // ws_refit_enable_sh: the rest coefficients, one plane per element ([3 (ncoef - 1)][num_points]); empty at degree 0
    uint32_t ncoef = 1;                  // (sh_deg + 1)^2 of the cloud
    bool sh_enabled = false;
    DeviceBuf<float> sh_master, sh_m, sh_v;
};
static_assert(sizeof(ws_refit_sh_params) == 72 && offsetof(ws_refit_sh_params, lr_sh) == 56 && offsetof(ws_refit_sh_params, reserved) == 60,
              "ws_refit_sh_params layout (websplat/_lib.py mirrors it)");
static_assert(sizeof(ws_refit_params) == 56 && offsetof(ws_refit_params, colour_unit) == 24 && offsetof(ws_refit_params, reserved) == 40,
              "ws_refit_params layout (websplat/_lib.py mirrors it)");

// Everything about a ws_refit_params that can be judged without a handle; units = false: the two unit fields are not looked at
// (ws_scene_refit computes them per batch).
int ws_internal_refit_check_params(const ws_refit_params* p, const std::string& who, bool units) {
    if (!p) return fail(WS_ERR_INVALID, who + ": null params");
    for (uint32_t w : p->reserved)
        if (w != 0) return fail(WS_ERR_INVALID, who + ": reserved words must be zero");
    if (!std::isfinite(p->lr_colour) || !(p->lr_colour >= 0.0f)) return fail(WS_ERR_INVALID, who + ": lr_colour must be finite and not below 0");
    if (!std::isfinite(p->lr_opacity) || !(p->lr_opacity >= 0.0f)) return fail(WS_ERR_INVALID, who + ": lr_opacity must be finite and not below 0");
    if (!(p->beta1 >= 0.0f && p->beta1 < 1.0f)) return fail(WS_ERR_INVALID, who + ": beta1 must lie in [0, 1)");
    if (!(p->beta2 >= 0.0f && p->beta2 < 1.0f)) return fail(WS_ERR_INVALID, who + ": beta2 must lie in [0, 1)");
    if (!std::isfinite(p->eps) || !(p->eps > 0.0f)) return fail(WS_ERR_INVALID, who + ": eps must be finite and above 0");
    if (!(p->opacity_min >= 0.0f && p->opacity_min <= 1.0f)) return fail(WS_ERR_INVALID, who + ": opacity_min must lie in [0, 1]");
    if (units && (!std::isfinite(p->colour_unit) || !(p->colour_unit > 0.0))) return fail(WS_ERR_INVALID, who + ": colour_unit must be finite and above 0");
    if (units && (!std::isfinite(p->opacity_unit) || !(p->opacity_unit > 0.0))) return fail(WS_ERR_INVALID, who + ": opacity_unit must be finite and above 0");
    return WS_OK;
}

int ws_internal_refit_check_sh_params(const ws_refit_sh_params* p, const std::string& who, bool units) {
    if (!p) return fail(WS_ERR_INVALID, who + ": null params");
    if (const int rc = ws_internal_refit_check_params(&p->base, who, units)) return rc;
    for (uint32_t w : p->reserved)
        if (w != 0) return fail(WS_ERR_INVALID, who + ": reserved words must be zero");
    if (!std::isfinite(p->lr_sh) || !(p->lr_sh >= 0.0f)) return fail(WS_ERR_INVALID, who + ": lr_sh must be finite and not below 0");
    return WS_OK;
}

// The host's share of a step, common to ws_refit_step and ws_refit_step_sh: p1, p2 are the powers AFTER this step (committed by
// the caller only when the launch went out); `sums` is the caller's.
static RefitParams refit_kernel_params(const ws_refit* rf, ws_pointcloud* pc, const ws_refit_params* p, double p1, double p2) {
    RefitParams kp;
    kp.planes = pc->planes.get();
    kp.sums = nullptr;
    kp.master = rf->master.get();
    kp.m = rf->m.get();
    kp.v = rf->v.get();
    kp.n = rf->num_points;
    kp.lr_colour = p->lr_colour;
    kp.lr_opacity = p->lr_opacity;
    kp.beta1 = p->beta1;
    kp.beta2 = p->beta2;
    kp.omb1 = 1.0f - p->beta1;
    kp.omb2 = 1.0f - p->beta2;
    kp.bc1 = (float)(1.0 - p1);
    kp.bc2 = (float)(1.0 - p2);
    kp.eps = p->eps;
    kp.opacity_min = p->opacity_min;
    kp.u_colour = p->colour_unit * REFIT_C0_F64;
    kp.u_opacity = p->opacity_unit;
    return kp;
}

extern "C" {

int ws_refit_create(ws_context* ctx, const ws_pointcloud* pc, ws_refit** out) {
    if (!ctx || !pc || !out) return fail(WS_ERR_INVALID, "ws_refit_create: null argument");
    *out = nullptr;
    if (pc->compressed)
        return fail(WS_ERR_UNSUPPORTED, "ws_refit_create: a compressed cloud cannot be refitted (its codebooks are shared between Gaussians)");
    std::unique_ptr<ws_refit, SyncedDelete> rf(new (std::nothrow) ws_refit());
    if (!rf) return fail(WS_ERR_OOM, "ws_refit_create: host allocation failed");
    rf->ctx = ctx;
    rf->pc = pc;
    rf->planes = pc->planes.get();
    rf->num_points = pc->num_points;
    rf->ncoef = (pc->sh_deg + 1) * (pc->sh_deg + 1);
    WS_TRY(rf->master.alloc(rf->num_points));
    WS_TRY(rf->m.alloc(rf->num_points));
    WS_TRY(rf->v.alloc(rf->num_points));
    WS_TRY(launch_refit_init(rf->planes, rf->num_points, rf->master.get(), rf->m.get(), rf->v.get(), nullptr));
    if (hipDeviceSynchronize() != hipSuccess) return fail(WS_ERR_HIP, "ws_refit_create: device sync failed");
    *out = rf.release();
    return WS_OK;
}

void ws_refit_destroy(ws_refit* rf) { SyncedDelete()(rf); }

uint32_t ws_refit_num_points(const ws_refit* rf) { return rf ? rf->num_points : 0u; }
uint32_t ws_refit_steps(const ws_refit* rf) { return rf ? rf->steps : 0u; }

// The descriptor is judged by itself first, then the handles; the host's share of the step (the running beta powers, the bias
// corrections, the units) is committed only when the launch went out.
int ws_refit_step(ws_refit* rf, ws_pointcloud* pc, const ws_grad* g, const ws_refit_params* p, void* stream_v) {
    const std::string who("ws_refit_step");
    if (const int rc = ws_internal_refit_check_params(p, who, true)) return rc;
    if (!rf || !pc || !g) return fail(WS_ERR_INVALID, who + ": null argument");
    if (pc != rf->pc || pc->planes.get() != rf->planes || pc->compressed || pc->num_points != rf->num_points)
        return fail(WS_ERR_INVALID, who + ": not the point cloud this object was created for");
    if (g->num_points != rf->num_points) return fail(WS_ERR_INVALID, who + ": the gradient accumulator was created for another number of points");
    const double p1 = rf->p1 * (double)p->beta1, p2 = rf->p2 * (double)p->beta2;
    RefitParams kp = refit_kernel_params(rf, pc, p, p1, p2);
    kp.sums = g->sums.get();
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (const int rc = launch_refit_step(kp, stream)) return rc;
    rf->p1 = p1;
    rf->p2 = p2;
    ++rf->steps;
    rf->last_stream = stream;
    return WS_OK;
}

// The rest coefficients join: masters and moments of their own, widened from the stored halves.  Refused once a step has been
// taken: the bias-correction powers are the object's, shared by every element.
int ws_refit_enable_sh(ws_refit* rf, const ws_pointcloud* pc, void* stream_v) {
    const std::string who("ws_refit_enable_sh");
    if (!rf || !pc) return fail(WS_ERR_INVALID, who + ": null argument");
    if (pc != rf->pc || pc->planes.get() != rf->planes || pc->compressed || pc->num_points != rf->num_points)
        return fail(WS_ERR_INVALID, who + ": not the point cloud this object was created for");
    if (rf->sh_enabled) return WS_OK;
    if (rf->steps > 0) return fail(WS_ERR_INVALID, who + ": steps have been taken already (the bias-correction powers are shared)");
    const size_t count = (size_t)3 * (rf->ncoef - 1) * rf->num_points;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (count) {
        DeviceBuf<float> master, m, v;
        WS_TRY(master.alloc(count));
        WS_TRY(m.alloc(count));
        WS_TRY(v.alloc(count));
        WS_TRY(launch_refit_init_sh(rf->planes, rf->num_points, rf->ncoef, master.get(), m.get(), v.get(), stream));
        rf->sh_master = std::move(master);
        rf->sh_m = std::move(m);
        rf->sh_v = std::move(v);
        rf->last_stream = stream;
    }
    rf->sh_enabled = true;
    return WS_OK;
}

int ws_refit_step_sh(ws_refit* rf, ws_pointcloud* pc, const ws_shgrad* g, const ws_refit_sh_params* p, void* stream_v) {
    const std::string who("ws_refit_step_sh");
    if (const int rc = ws_internal_refit_check_sh_params(p, who, true)) return rc;
    if (!rf || !pc || !g) return fail(WS_ERR_INVALID, who + ": null argument");
    if (pc != rf->pc || pc->planes.get() != rf->planes || pc->compressed || pc->num_points != rf->num_points)
        return fail(WS_ERR_INVALID, who + ": not the point cloud this object was created for");
    if (!rf->sh_enabled) return fail(WS_ERR_INVALID, who + ": ws_refit_enable_sh was not called");
    if (g->num_points != rf->num_points) return fail(WS_ERR_INVALID, who + ": the gradient accumulator was created for another number of points");
    if (g->ncoef != rf->ncoef) return fail(WS_ERR_INVALID, who + ": the gradient accumulator was created for another SH degree");
    const double p1 = rf->p1 * (double)p->base.beta1, p2 = rf->p2 * (double)p->base.beta2;
    RefitShParams kp;
    kp.base = refit_kernel_params(rf, pc, &p->base, p1, p2);
    kp.sh_sums = g->sums.get();
    kp.sh_master = rf->sh_master.get();
    kp.sh_m = rf->sh_m.get();
    kp.sh_v = rf->sh_v.get();
    kp.ncoef = rf->ncoef;
    kp.lr_sh = rf->ncoef > 1 ? p->lr_sh : 0.0f;
    kp.u_sh = p->base.colour_unit;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (const int rc = launch_refit_step_sh(kp, stream)) return rc;
    rf->p1 = p1;
    rf->p2 = p2;
    ++rf->steps;
    rf->last_stream = stream;
    return WS_OK;
}

int ws_refit_download_sh(ws_refit* rf, uint32_t capacity, float* master, float* m, float* v) {
    if (!rf) return fail(WS_ERR_INVALID, "ws_refit_download_sh: null object");
    if (!rf->sh_enabled) return fail(WS_ERR_INVALID, "ws_refit_download_sh: ws_refit_enable_sh was not called");
    if ((master || m || v) && capacity < rf->num_points) return fail(WS_ERR_INVALID, "ws_refit_download_sh: capacity smaller than the number of points");
    WS_HIP(hipStreamSynchronize(rf->last_stream));
    const size_t n = rf->num_points, el = (size_t)3 * (rf->ncoef - 1);
    if (el == 0 || (!master && !m && !v)) return WS_OK;
    std::unique_ptr<float[]> st(new (std::nothrow) float[el * n]);
    if (!st) return fail(WS_ERR_OOM, "ws_refit_download_sh: host allocation failed");
    const std::pair<float*, const float*> jobs[3] = {{master, rf->sh_master.get()}, {m, rf->sh_m.get()}, {v, rf->sh_v.get()}};
    for (const auto& job : jobs) {
        if (!job.first) continue;
        WS_TRY(copy_d2h(st.get(), job.second, el * n * sizeof(float), rf->last_stream));
        for (size_t e = 0; e < el; ++e)
            for (size_t i = 0; i < n; ++i) job.first[i * el + e] = st[e * n + i];
    }
    return WS_OK;
}

int ws_refit_download(ws_refit* rf, uint32_t capacity, float* master, float* m, float* v) {
    if (!rf) return fail(WS_ERR_INVALID, "ws_refit_download: null object");
    if ((master || m || v) && capacity < rf->num_points) return fail(WS_ERR_INVALID, "ws_refit_download: capacity smaller than the number of points");
    WS_HIP(hipStreamSynchronize(rf->last_stream));
    if (master) WS_TRY(copy_d2h(master, rf->master.get(), rf->master.bytes(), rf->last_stream));
    if (m) WS_TRY(copy_d2h(m, rf->m.get(), rf->m.bytes(), rf->last_stream));
    if (v) WS_TRY(copy_d2h(v, rf->v.get(), rf->v.bytes(), rf->last_stream));
    return WS_OK;
}

}  // extern "C"
