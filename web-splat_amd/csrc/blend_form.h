// blend_form.h -- what one launch of the blend IS: every compile-time choice of k_blend and its sibling kernels by name, the rules
// that say which combinations exist, and the mapping from a request to its form.  Plain C++ (no HIP include): raster.hip
// instantiates exactly the legal forms from the table below, api_renderer.cpp asks the same predicate, and a CPU test enumerates both.
#pragma once

#include <stdint.h>

#include "websplat.h"

namespace ws {

// Forms of the FAST blend (k_blend's aux dimension): no auxiliary plane (the colour image only), coverage only, and the depth
// forms -- z staged beside every record, sum(w z), sum(w) and the median's crossing accumulated -- which write any of the three.
enum BlendAux { BLEND_AUX_NONE = 0, BLEND_AUX_ALPHA = 1, BLEND_AUX_Z = 2 };
// k_blend's comp dimension: two independent bits.  LOAD changes the epilogue only (one texel read in place of p.background);
// OCCLUDE stages z like BLEND_AUX_Z, folds z < D(p) into every pair and drops records behind the tile's largest D at staging.
enum BlendComp { BLEND_COMP_NONE = 0, BLEND_COMP_LOAD = 1, BLEND_COMP_OCCLUDE = 2 };
// The kernels a blend launch can be: k_blend, k_blend_strict (WS_BLEND_TARGET_PRECISION), and the experimental build's k_blend_q
// (one wave per quadrant, no LDS) and k_blend2 (barrier-free staging).
enum BlendKernel { BLEND_K = 0, BLEND_K_STRICT = 1, BLEND_K_Q = 2, BLEND_K_ASYNC = 3 };

#ifdef WS_EXPERIMENTAL  // measured-and-lost variants: compiled by `make experimental` only
constexpr bool BLEND_EXPERIMENTAL = true;
#else
constexpr bool BLEND_EXPERIMENTAL = false;
#endif

struct BlendForm {
    int kernel;    // BlendKernel; the fields below the first two are k_blend's (zero for the other kernels, comp apart)
    int format;    // ws_color_format of the target
    int qw, qh;    // quadrants (8x8 px, one wave each) per tile: 2x2, 4x2 or 4x4
    bool multi;    // several tiles per workgroup (4K-class tile counts)
    bool capture;  // analysis: walked-record counts (debug_consumed / debug_walked)
    bool dma;      // stage the Splat records with gfx950's LDS-DMA
    bool timing;   // analysis: per-wave phase times
    bool exact;    // WS_BLEND_FAST_EXACT_CUT
    int aux;       // BlendAux
    int comp;      // BlendComp bits (k_blend_strict: non-zero = its composite form, load / occluder are run-time switches there)

    // the non-type template argument of the kernels
    constexpr uint32_t bits() const {
        return (uint32_t)kernel | (uint32_t)format << 2 | (uint32_t)qw << 4 | (uint32_t)qh << 7 | (uint32_t)multi << 10 |
               (uint32_t)capture << 11 | (uint32_t)dma << 12 | (uint32_t)timing << 13 | (uint32_t)exact << 14 | (uint32_t)aux << 15 |
               (uint32_t)comp << 17;
    }
    static constexpr BlendForm of(uint32_t b) {
        return BlendForm{(int)(b & 3u), (int)(b >> 2 & 3u), (int)(b >> 4 & 7u), (int)(b >> 7 & 7u), (b >> 10 & 1u) != 0, (b >> 11 & 1u) != 0,
                         (b >> 12 & 1u) != 0, (b >> 13 & 1u) != 0, (b >> 14 & 1u) != 0, (int)(b >> 15 & 3u), (int)(b >> 17 & 3u)};
    }
    constexpr int waves() const { return qw * qh; }
    constexpr bool occlude() const { return (comp & BLEND_COMP_OCCLUDE) != 0; }
    constexpr bool stage_z() const { return aux == BLEND_AUX_Z || occlude(); }  // the third LDS plane: z beside every staged record
    // trailing kernel arguments: the AUX forms take the planes, the COMP forms the planes and the composite, the others nothing
    // (so the forms without them keep their kernel-argument layout, hidden arguments included)
    constexpr int tail_args() const { return comp != BLEND_COMP_NONE ? 2 : (aux != BLEND_AUX_NONE ? 1 : 0); }
};

// The combination rules, once: exactly the forms the library instantiates.
constexpr bool blend_form_legal(BlendForm f) {
    if (f.format != WS_FORMAT_RGBA32_FLOAT && f.format != WS_FORMAT_RGBA16_FLOAT && f.format != WS_FORMAT_RGBA8_UNORM) return false;
    if (f.comp < BLEND_COMP_NONE || f.comp > (BLEND_COMP_LOAD | BLEND_COMP_OCCLUDE)) return false;
    if (f.kernel != BLEND_K) {  // one kernel per format; k_blend_strict also has a composite form (comp = LOAD)
        const bool known = f.kernel == BLEND_K_STRICT || (BLEND_EXPERIMENTAL && (f.kernel == BLEND_K_Q || f.kernel == BLEND_K_ASYNC));
        const bool comp_ok = f.comp == BLEND_COMP_NONE || (f.kernel == BLEND_K_STRICT && f.comp == BLEND_COMP_LOAD);
        return known && comp_ok && !f.qw && !f.qh && !f.multi && !f.capture && !f.dma && !f.timing && !f.exact && f.aux == BLEND_AUX_NONE;
    }
    if (!((f.qw == 2 && f.qh == 2) || (f.qw == 4 && f.qh == 2) || (f.qw == 4 && f.qh == 4))) return false;
    if (f.aux != BLEND_AUX_NONE && f.aux != BLEND_AUX_ALPHA && f.aux != BLEND_AUX_Z) return false;
    const bool plain = f.aux == BLEND_AUX_NONE && f.comp == BLEND_COMP_NONE;
    // the timing build instruments the production form only: 32x32 tiles, rgba32float target, one tile per workgroup
    if (f.timing) return plain && f.qw == 4 && f.qh == 4 && f.format == WS_FORMAT_RGBA32_FLOAT && !f.multi && !f.capture && !f.dma && !f.exact;
    if (f.capture) return plain && f.multi && !f.dma && !f.exact;  // (the capture build is the several-tiles form, whatever tpw is)
    if (f.dma) return BLEND_EXPERIMENTAL && plain && !f.exact;     // (LDS-DMA staging: measured neutral, experimental build only)
    if (f.exact) return plain;  // the exact cut-off decision belongs to the production launch, without planes or composite
    // the auxiliary planes and the composite belong to the FAST production launch; no plane under a composite = the coverage
    // form with a null alpha pointer (one uniform branch at the store)
    return f.comp == BLEND_COMP_NONE || f.aux != BLEND_AUX_NONE;
}

// Every legal form, for the dispatcher (raster.hip) to instantiate: the cross product of the dimensions, filtered.
struct BlendFormTable {
    uint32_t n;
    uint32_t bits[256];
};
constexpr BlendFormTable blend_form_table() {
    constexpr int shapes[4][2] = {{0, 0}, {2, 2}, {4, 2}, {4, 4}};
    BlendFormTable t{};
    for (int kernel = 0; kernel < 4; ++kernel)
        for (int format = 0; format < 3; ++format)  // (ws_color_format is 0 .. 2)
            for (int sh = 0; sh < 4; ++sh)
                for (uint32_t flags = 0; flags < 32u; ++flags)
                    for (int aux = 0; aux < 3 && (kernel == BLEND_K || !(sh | flags | aux)); ++aux)
                        for (int comp = 0; comp < 4; ++comp) {
                            const BlendForm f{kernel, format, shapes[sh][0], shapes[sh][1], (flags & 1u) != 0, (flags & 2u) != 0, (flags & 4u) != 0,
                                              (flags & 8u) != 0, (flags & 16u) != 0, aux, comp};
                            if (blend_form_legal(f)) t.bits[t.n++] = f.bits();
                        }
    return t;
}

// "The FAST production launch": what the auxiliary planes and the composite need.  Every call site fills in what it knows of
// the launch (the entry points the renderer's and the context's switches, the launcher the launch's own) and leaves the rest 0.
struct BlendLaunchMode {
    bool capture, timing;
    int dma, variant;
    bool exact_cut, async_staging;
    int debug_cut;
};
constexpr bool blend_production_launch(const BlendLaunchMode& m) {
    return !m.capture && !m.timing && !m.dma && m.variant == 0 && !m.exact_cut && !m.async_staging && !m.debug_cut;
}

// The renderer's part of the decision (api_renderer.cpp render_frame), from its blend mode and the context's switches: which kernel
// family, whether the exact cut applies, whether 4x4 tiles are composited as two 4x2 halves, whether the order table is used.
struct BlendFrameRequest {
    bool target_precision, exact_mode;  // WS_BLEND_TARGET_PRECISION, WS_BLEND_FAST_EXACT_CUT (neither: WS_BLEND_FAST)
    int variant;                        // the context's (experimental) blend variant: 0 = k_blend, 1 = k_blend_q, 2 = k_blend_strict
    bool capture, timing;
    bool split_wanted, order_valid;     // halves asked for (or automatic: few tiles); the frame has a longest-list-first table
    uint32_t qw, qh;                    // the context's tile shape
};
struct BlendFrameChoice {
    int variant;
    bool exact_cut, split, ordered;
};
constexpr BlendFrameChoice blend_frame_choice(const BlendFrameRequest& q) {
    BlendFrameChoice c{};
    c.variant = q.target_precision ? 2 : q.variant;
    c.exact_cut = q.exact_mode && !q.capture && !q.timing;
    c.split = q.split_wanted && q.qw == 4u && q.qh == 4u && !q.capture && q.variant == 0 && !q.target_precision;
    c.ordered = q.order_valid && q.qw == 4u && q.qh == 4u && !c.split && !q.capture;
    return c;
}

// One launch as the launcher sees it (raster.hip launch_blend fills this from BlendParams, the planes and the composite).
struct BlendRequest {
    int format;
    uint32_t qw, qh;
    bool multi;    // more than one tile per workgroup (the resolved tpw_log2 > 0)
    bool split;    // range_row_shift != 0
    BlendLaunchMode mode;  // (debug_cut is the entry points' business: 0 here)
    int aux;       // BlendAux of the planes asked for
    int comp;      // BlendComp bits of the composite asked for
    bool has_z;    // the frame has a z plane
};
struct BlendChoice {
    int rc;           // WS_OK, or the error code and its text
    const char* why;
    BlendForm form;
};
constexpr BlendChoice blend_refuse(int rc, const char* why) { return BlendChoice{rc, why, BlendForm{}}; }
constexpr BlendChoice blend_form_of(const BlendRequest& q) {
    const BlendLaunchMode& m = q.mode;
    if (q.aux == BLEND_AUX_Z && !q.has_z) return blend_refuse(WS_ERR_STATE, "blend: the depth planes need the frame's z plane");
    if (q.aux != BLEND_AUX_NONE && m.variant != 0) return blend_refuse(WS_ERR_UNSUPPORTED, "blend: auxiliary planes need the FAST blend");
    if ((q.comp & BLEND_COMP_OCCLUDE) && !q.has_z) return blend_refuse(WS_ERR_STATE, "blend: an occluder needs the frame's z plane");
    if (q.comp != BLEND_COMP_NONE && m.variant != 0 && m.variant != 2)
        return blend_refuse(WS_ERR_UNSUPPORTED, "blend: the composite needs the FAST blend or WS_BLEND_TARGET_PRECISION");
    BlendForm f{};
    f.format = q.format;
    if (m.variant == 2) {  // WS_BLEND_TARGET_PRECISION: back to front, destination rounded after every splat
        f.kernel = BLEND_K_STRICT;
        f.comp = q.comp != BLEND_COMP_NONE ? BLEND_COMP_LOAD : BLEND_COMP_NONE;
    } else if (m.variant == 1) {  // one wave per 8x8 quadrant, no LDS (cross-check)
        if (!BLEND_EXPERIMENTAL) return blend_refuse(WS_ERR_UNSUPPORTED, "blend variant 1 (k_blend_q) is only in the experimental build");
        f.kernel = BLEND_K_Q;
    } else {
        if (!((q.qw == 2u && q.qh == 2u) || (q.qw == 4u && q.qh == 2u) || (q.qw == 4u && q.qh == 4u)))
            return blend_refuse(WS_ERR_INVALID, "blend: unsupported tile shape");
        f.qw = (int)q.qw, f.qh = (int)q.qh;
        f.multi = q.multi;
        if (q.comp != BLEND_COMP_NONE || q.aux != BLEND_AUX_NONE) {
            // the FAST production forms -- one tile or several per workgroup, split halves, the longest-first order
            if (!blend_production_launch(m))
                return blend_refuse(WS_ERR_UNSUPPORTED, "blend: auxiliary planes and the composite need the FAST production launch "
                                                        "(no capture / timing / DMA / exact cut / variants)");
            f.aux = q.aux == BLEND_AUX_Z ? BLEND_AUX_Z : BLEND_AUX_ALPHA;
            f.comp = q.comp;
        } else if (m.timing) {  // analysis: the production form with time stamps
            f.timing = true, f.capture = m.capture, f.dma = m.dma != 0;
            if (!blend_form_legal(f))
                return blend_refuse(WS_ERR_UNSUPPORTED, "blend timing: 32x32 tiles, rgba32float target, one tile per workgroup, no capture / DMA");
        } else if (m.async_staging && !BLEND_EXPERIMENTAL) {
            return blend_refuse(WS_ERR_UNSUPPORTED, "barrier-free staging (k_blend2) is only in the experimental build");
        } else if (m.dma && !BLEND_EXPERIMENTAL) {
            return blend_refuse(WS_ERR_UNSUPPORTED, "LDS-DMA staging is only in the experimental build");
        } else if (m.async_staging && q.qw == 4u && q.qh == 4u && !m.capture && !q.multi && !m.dma && !q.split) {
            // the barrier-free form: one 32x32 tile per workgroup, production launch only (any other launch stages with barriers)
            f = BlendForm{};
            f.kernel = BLEND_K_ASYNC, f.format = q.format;
        } else if (m.capture) {
            f.capture = f.multi = true;
        } else if (m.dma) {
            f.dma = true;
        } else {
            f.exact = m.exact_cut;
        }
    }
    if (!blend_form_legal(f)) return blend_refuse(WS_ERR_INVALID, "blend: unknown colour format");
    return BlendChoice{WS_OK, "", f};
}

}  // namespace ws
