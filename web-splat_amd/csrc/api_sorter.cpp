// api_sorter.cpp -- ws_sorter (GPURSSorter + PointCloudSortStuff, gpu_rs.rs:23-175, 865-884): the stand-alone sorter, the
// renderer's depth sort as a call of its own, and the known-answer self-test.
#include <cstddef>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_state.h"

using namespace ws;

// small per-sort zero arena of a stand-alone sorter: tickets, error word, digit histograms, the depth sort's key-range fold
struct SorterZero {
    uint32_t tickets[4];
    uint32_t error;
    uint32_t _pad[3];
    uint32_t hist[4 * 512];                                  // (rows of 512: 9-bit digits; 8-bit digits use the first 256)
    uint32_t fat_barrier[9 * 16];                            // single-launch depth sort: barrier state
    FrameCounters counters;                                  // ws_sorter_sort_depth: the range report and decision (depth_range_decide)
};

struct ws_sorter {
    ws_context* ctx = nullptr;
    DeviceBuf<uint32_t> keys_alt, vals_alt, aux_alt, tile_sums;  // ping-pong partners [max_n + 4] and the count rows
    DeviceBuf<SorterZero> zero;
    DeviceBuf<uint64_t> fat_status;  // a context whose depth sort is the fat-tile one-sweep: its chunk-count rows
    SortScratch sc;        // what the launchers take: views of the buffers above
    FatSortScratch fat;
    uint32_t epoch = 0;
    bool folded = false;              // the last ws_sorter_sort_depth folded the key range (ws_sorter_depth_range)
    hipStream_t last_stream = nullptr;
};

extern "C" {

// ---- GPURSSorter ---------------------------------------------------------------------------------------
int ws_sorter_create(ws_context* ctx, uint32_t max_n, ws_sorter** out) {
    if (!ctx || !out) return fail(WS_ERR_INVALID, "ws_sorter_create: null argument");
    *out = nullptr;
    if (max_n == 0 || max_n >= (1u << 30)) return fail(WS_ERR_INVALID, "ws_sorter_create: max_n out of range");
    std::unique_ptr<ws_sorter, SyncedDelete> s(new (std::nothrow) ws_sorter());
    if (!s) return fail(WS_ERR_OOM, "ws_sorter_create: host allocation failed");
    s->ctx = ctx;
    const SortShape shape = sort_shape(max_n, 0, 512);  // (512 count rows: 9-bit digits)
    WS_TRY(s->keys_alt.alloc((size_t)max_n + 4));
    WS_TRY(s->vals_alt.alloc((size_t)max_n + 4));
    WS_TRY(s->tile_sums.alloc(shape.sum_words));
    WS_TRY(s->zero.alloc(1));
    WS_TRY(s->aux_alt.alloc((size_t)max_n + 4));
    if (hipDeviceSynchronize() != hipSuccess) return fail(WS_ERR_HIP, "ws_sorter_create: device sync failed");
    SorterZero* const zero = s->zero.get();
    s->sc = sort_view(shape, s->keys_alt.get(), s->vals_alt.get(), zero->hist, 512, s->tile_sums.get(), nullptr);
    if (ctx->depth_sort_mode == DS_ONESWEEP || ctx->depth_sort_mode == DS_COOP) {
        WS_TRY(s->fat_status.alloc(fat_sort_status_words()));
        if (hipMemset(s->fat_status.get(), 0, s->fat_status.bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return fail(WS_ERR_HIP, "ws_sorter_create: look-back word initialisation failed");
        FatSortScratch& fs = s->fat;
        fs.cap = max_n, fs.status = s->fat_status.get(), fs.grid_request = ctx->dsort_fat_grid;
        fs.keys_alt = s->keys_alt.get(), fs.vals_alt = s->vals_alt.get(), fs.aux_alt = s->aux_alt.get();
        fs.hist = zero->hist, fs.tickets = zero->tickets, fs.barrier = zero->fat_barrier, fs.error = &zero->error;
    }
    *out = s.release();
    return WS_OK;
}

void ws_sorter_destroy(ws_sorter* s) { SyncedDelete()(s); }

int ws_sorter_sort(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, const uint32_t* d_count, uint32_t n,
                   void* stream_v) {
    if (!s || !d_keys || !d_payload) return fail(WS_ERR_INVALID, "ws_sorter_sort: null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    s->folded = false;  // (the memset below clears what a ws_sorter_sort_depth decided)
    WS_HIP(hipMemsetAsync(s->zero.get(), 0, sizeof(SorterZero), stream));
    SortJob job;
    job.keys = d_keys, job.vals = d_payload, job.d_count = d_count, job.n = n;
    SortResult res;
    WS_TRY(launch_sort_pairs(s->sc, job, stream, nullptr, &res));
    if (res.keys != d_keys) return fail(WS_ERR_STATE, "ws_sorter_sort: internal ping-pong parity error");
    return WS_OK;
}

// The renderer's depth sort as a stand-alone call: the same result as ws_sorter_sort (stable ascending on the full
// 32-bit keys) by the kernels a frame's depth sort runs -- the generic sorter with a companion value, or, in a context
// created with WS_DEPTH_SORT=onesweep | coop and for inputs within its capacity, the fat-tile one-sweep (sort.hip);
// `d_aux` (may be null) is a 4-byte companion value that travels with the payload.  Four passes: keys, payload and
// companion are sorted in place.
int ws_sorter_sort_depth(ws_sorter* s, uint32_t* d_keys, uint32_t* d_payload, uint32_t* d_aux, const uint32_t* d_count,
                         uint32_t n, void* stream_v) {
    if (!s || !d_keys || !d_payload) return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: null argument");
    if (n > s->sc.cap) return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: n exceeds the sorter's capacity");
    // the histogram kernels read the keys 16 bytes at a time: the same alignment ws_sorter_sort asks for
    if ((reinterpret_cast<uintptr_t>(d_keys) & 15u) != 0)
        return fail(WS_ERR_INVALID, "ws_sorter_sort_depth: keys must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (++s->epoch == 0) {  // epoch-tagged count rows of the fat-tile form: re-zeroed on wrap-around
        if (s->fat_status.get()) WS_HIP(hipMemsetAsync(s->fat_status.get(), 0, s->fat_status.bytes(), stream));
        s->epoch = 1;
    }
    s->folded = false;
    s->last_stream = stream;
    WS_HIP(hipMemsetAsync(s->zero.get(), 0, sizeof(SorterZero), stream));
    const bool fat = n != 0 && s->fat.status && fat_sort_grid(n, s->ctx->num_cus, s->fat.grid_request) != 0u;
    // the frame's form (ws_renderer_prepare): the first histogram kernel reports the key range, the column scan behind it decides
    // the base of passes 1..3 and whether the fourth pass runs (depth_range_decide)
    FrameCounters* skip_top = (s->ctx->depth_skip_top && !fat) ? &s->zero.get()->counters : nullptr;
    s->folded = skip_top != nullptr;
    if (n == 0) return WS_OK;
    SortResult res;
    if (fat)
        return launch_depth_sort_fat(s->fat, d_keys, d_payload, d_aux, d_count, n, false, s->ctx->depth_sort_mode == DS_COOP,
                                     s->epoch, s->ctx->num_cus, stream, nullptr, &res);
    SortJob job;
    job.kind = SORT_DEPTH;
    job.keys = d_keys, job.vals = d_payload, job.d_count = d_count, job.n = n;
    job.digit_bits = depth_sort_digit_bits(s->ctx->depth_digit_bits, false, 0u, 0);  // (no previous frame, no graph: forced, or the default)
    job.aux = d_aux, job.aux_alt = d_aux ? s->aux_alt.get() : nullptr;
    job.skip_top = skip_top;
    job.kpt9 = s->ctx->depth_tile_kpt ? s->ctx->depth_tile_kpt : 8;
    WS_TRY(launch_sort_pairs(s->sc, job, stream, nullptr, &res));
    if (res.keys != d_keys) return fail(WS_ERR_STATE, "ws_sorter_sort_depth: internal ping-pong parity error");
    if (!skip_top) return WS_OK;
    // three passes when the fourth was skipped: the result is in the scratch partners -> back in place
    if (res.keys_skipped != s->sc.keys_alt || res.vals_skipped != s->sc.vals_alt)
        return fail(WS_ERR_STATE, "ws_sorter_sort_depth: internal ping-pong parity error (skipped pass)");
    return launch_depth_copy_back(&skip_top->depth_skip_top, d_count, n, res.keys_skipped, res.vals_skipped, res.aux_skipped, d_keys,
                                  d_payload, d_aux, stream);
}

int ws_sorter_depth_range(ws_sorter* s, uint32_t* base, uint32_t* skip, uint32_t* span_class) {
    if (!s || !base || !skip || !span_class) return fail(WS_ERR_INVALID, "ws_sorter_depth_range: null argument");
    if (!s->folded)
        return fail(WS_ERR_STATE, "ws_sorter_depth_range: the last ws_sorter_sort_depth did not fold its key range "
                                  "(the context's depth_skip_top is 0, the fat-tile form ran, or no such call)");
    uint32_t w[3];  // depth_skip_top, depth_key_base, depth_span_class: adjacent words of the counters' second line
    static_assert(offsetof(FrameCounters, depth_key_base) == offsetof(FrameCounters, depth_skip_top) + 4 &&
                      offsetof(FrameCounters, depth_span_class) == offsetof(FrameCounters, depth_skip_top) + 8,
                  "FrameCounters layout");
    WS_TRY(copy_d2h(w, &s->zero.get()->counters.depth_skip_top, sizeof w, s->last_stream));
    *skip = w[0];
    *base = w[1];
    *span_class = w[2];
    return WS_OK;
}

int ws_sort_selftest(ws_context* ctx, int* passed) {
    if (!ctx || !passed) return fail(WS_ERR_INVALID, "ws_sort_selftest: null argument");
    *passed = 0;
    const uint32_t n = 8192;  // gpu_rs.rs:297
    std::vector<float> scrambled(n), expect(n);
    std::vector<uint32_t> payload(n);
    for (uint32_t i = 0; i < n; ++i) {
        scrambled[i] = (float)(n - 1 - i);
        expect[i] = (float)i;
        payload[i] = i;
    }
    ws_sorter* sorter = nullptr;
    WS_TRY(ws_sorter_create(ctx, n, &sorter));
    DeviceBuf<uint32_t> dk, dv;  // (declared first: let go after the sorter's destroyer has waited for the device)
    const std::unique_ptr<ws_sorter, SyncedDelete> s(sorter);
    WS_TRY(dk.alloc(n));
    WS_TRY(dv.alloc(n));
    hipError_t e = hipMemcpy(dk.get(), scrambled.data(), n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dv.get(), payload.data(), n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "ws_sort_selftest: upload");
    WS_TRY(ws_sorter_sort(s.get(), dk.get(), dv.get(), nullptr, n, nullptr));
    std::vector<float> got(n);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(got.data(), dk.get(), n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "ws_sort_selftest: download");
    *passed = std::memcmp(got.data(), expect.data(), n * 4) == 0 ? 1 : 0;
    return WS_OK;
}

}  // extern "C"
