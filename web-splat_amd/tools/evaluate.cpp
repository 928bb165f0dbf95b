// websplat_evaluate -- PSNR and SSIM of a scene over a cameras.json split, computed on the device (websplat.h "Image metrics"):
//   websplat_evaluate <scene.ply|.npz> <cameras.json> (--ref <other.ply|.npz> | --gt <dir>) [--split train|test] [--quantize]
//                     [--blame N [--error sq|abs|dssim]] [--removal N [--error sq|abs]] [--gradient N [--error sq|abs]] [--densify N [--error sq|abs]]
//                     [--refit EPOCHS [--lr-colour X] [--lr-opacity Y] [--views-per-step B] [--error sq|abs] [--refit-sh [--lr-sh Z]]]
//                     [--save OUT.ply]
// prints one line per camera and the means of the per-image PSNR and SSIM (the 3DGS convention).  --ref compares against
// another point cloud (a pruned one against its parent); --gt against <dir>/<img_name>[.png], rendered at each PNG's size.
// --blame N: behind that table, the N Gaussians of the scene with the largest error sum over the split (websplat.h "Attributing a
// pixel plane to Gaussians"): index, error sum, weight sum and their ratio, the mean error under the Gaussian.
// --removal N: behind all that, the N Gaussians whose deletion alone would change the split's frames most (websplat.h "Removal
// effect"): index, effect sum, plain contribution sum and their ratio, then how many drawn Gaussians have an effect of exactly 0.
// It needs no second image: --ref / --gt may be left out, and then only this table is printed.
// --gradient N: behind all that, the N Gaussians with the largest |d error / d ln opacity| over the split (websplat.h "Gradients
// of an image loss"; the error is --blame's, sq or abs, against --ref / --gt): index, opacity gradient, the three colour
// gradients, then how many drawn Gaussians have all four sums 0.
// --densify N: behind all that, the N Gaussians with the largest screen_norm / seen over the split (websplat.h "Geometry gradients":
// the INRIA trainer's densification statistic; the error as --gradient's): index, that mean, seen, |d error / d position|, then how
// many seen Gaussians have a norm of exactly 0.
// --refit EPOCHS: behind all that, Adam steps on the scene's DC colours and opacities over the TRAIN split against --ref / --gt
// (websplat.h "Refitting colour and opacity"; a step after every B views, default: one per epoch), then the first table again,
// of the refitted scene, under a line "after refit: EPOCHS epochs, S steps".  A compressed scene is refused.
// --refit-sh: the refit also moves the higher SH coefficients (websplat.h "SH gradients"), at the rate --lr-sh (default:
// lr_colour / 20, the 3DGS convention); the line then ends ", SH degree D".
// --save OUT.ply: at the end, the scene as it then stands -- after --refit, the refitted one -- as an INRIA 3DGS .ply (websplat.h
// "Saving a point cloud"), and one line "saved OUT.ply: N Gaussians, B bytes".  It needs no second image either.  A compressed
// scene is refused with the library's message.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "websplat.h"
#include "websplat_env.h"  // the harness-side translation of WS_* switches (the library reads no environment)

// the value of an option that takes a positive integer; false: not one
static bool positive(const char* text, long* value) {
    char* end = nullptr;
    *value = std::strtol(text, &end, 10);
    return !*end && *value > 0;
}

// the indices of the `want` largest keys among np (all of them when there are fewer), largest first, ties by index
template <class Key>
static std::vector<uint32_t> top_by(uint32_t np, long want, Key key) {
    std::vector<uint32_t> order(np);
    for (uint32_t i = 0; i < np; ++i) order[i] = i;
    const size_t top = std::min<size_t>((size_t)want, np);
    std::partial_sort(order.begin(), order.begin() + top, order.end(), [&](uint32_t a, uint32_t b) { return key(a) != key(b) ? key(a) > key(b) : a < b; });
    order.resize(top);
    return order;
}

int main(int argc, char** argv) {
    const char *ref = nullptr, *gt = nullptr, *save = nullptr;
    int split = WS_SPLIT_TEST;
    uint32_t flags = 0;
    long blame = 0, removal = 0, gradient = 0, densify = 0, refit = 0, views_per_step = 0;
    double lr_colour = 0.0025, lr_opacity = 0.01, lr_sh = -1.0;  // (lr_sh < 0: lr_colour / 20)
    bool have_refit_option = false, refit_sh = false;
    int kind = WS_ERROR_SQ;
    bool bad = argc < 3, have_error = false;
    for (int i = 3; i < argc && !bad; ++i) {
        if (!std::strcmp(argv[i], "--ref") && i + 1 < argc) ref = argv[++i];
        else if (!std::strcmp(argv[i], "--gt") && i + 1 < argc) gt = argv[++i];
        else if (!std::strcmp(argv[i], "--save") && i + 1 < argc) save = argv[++i];
        else if (!std::strcmp(argv[i], "--split") && i + 1 < argc) {
            ++i;
            if (!std::strcmp(argv[i], "train")) split = WS_SPLIT_TRAIN;
            else if (!std::strcmp(argv[i], "test")) split = WS_SPLIT_TEST;
            else bad = true;
        } else if (!std::strcmp(argv[i], "--quantize")) flags |= WS_METRICS_QUANTIZE_U8;
        else if (!std::strcmp(argv[i], "--blame") && i + 1 < argc) bad = !positive(argv[++i], &blame);
        else if (!std::strcmp(argv[i], "--removal") && i + 1 < argc) bad = !positive(argv[++i], &removal);
        else if (!std::strcmp(argv[i], "--gradient") && i + 1 < argc) bad = !positive(argv[++i], &gradient);
        else if (!std::strcmp(argv[i], "--densify") && i + 1 < argc) bad = !positive(argv[++i], &densify);
        else if (!std::strcmp(argv[i], "--refit") && i + 1 < argc) bad = !positive(argv[++i], &refit);
        else if (!std::strcmp(argv[i], "--views-per-step") && i + 1 < argc) {
            have_refit_option = true;
            bad = !positive(argv[++i], &views_per_step);
        } else if (!std::strcmp(argv[i], "--refit-sh")) {
            have_refit_option = refit_sh = true;
        } else if ((!std::strcmp(argv[i], "--lr-colour") || !std::strcmp(argv[i], "--lr-opacity") || !std::strcmp(argv[i], "--lr-sh")) && i + 1 < argc) {
            double& lr = !std::strcmp(argv[i], "--lr-colour") ? lr_colour : !std::strcmp(argv[i], "--lr-opacity") ? lr_opacity : lr_sh;
            char* end = nullptr;
            lr = std::strtod(argv[++i], &end);
            have_refit_option = true;
            if (*end || !(lr >= 0.0) || !std::isfinite(lr)) bad = true;
        } else if (!std::strcmp(argv[i], "--error") && i + 1 < argc) {
            ++i;
            have_error = true;
            if (!std::strcmp(argv[i], "sq")) kind = WS_ERROR_SQ;
            else if (!std::strcmp(argv[i], "abs")) kind = WS_ERROR_ABS;
            else if (!std::strcmp(argv[i], "dssim")) kind = WS_ERROR_DSSIM;
            else bad = true;
        } else bad = true;
    }
    if (have_error && blame == 0 && removal == 0 && gradient == 0 && densify == 0 && refit == 0) bad = true;
    if ((removal > 0 || gradient > 0 || densify > 0 || refit > 0) && kind == WS_ERROR_DSSIM) bad = true;
    if (have_refit_option && refit == 0) bad = true;
    if (lr_sh >= 0.0 && !refit_sh) bad = true;
    const bool compare = ref != nullptr || gt != nullptr;  // (--removal alone needs no second image)
    if ((blame > 0 || gradient > 0 || densify > 0 || refit > 0) && !compare) bad = true;
    if (bad || (ref != nullptr && gt != nullptr) || (!compare && removal == 0 && !save)) {
        std::fprintf(stderr, "usage: %s <scene.ply|.npz> <cameras.json> (--ref <other.ply|.npz> | --gt <dir>) [--split train|test] [--quantize] "
                             "[--blame N [--error sq|abs|dssim]] [--removal N [--error sq|abs]] [--gradient N [--error sq|abs]] [--densify N [--error sq|abs]] "
                             "[--refit EPOCHS [--lr-colour X] [--lr-opacity Y] [--views-per-step B] [--error sq|abs] [--refit-sh [--lr-sh Z]]] [--save OUT.ply]\n", argv[0]);
        return 2;
    }
    ws_context* ctx = nullptr;
    ws_pointcloud *pc = nullptr, *ref_pc = nullptr;
    ws_scene* scene = nullptr;
    ws_metrics* m = nullptr;
    ws_context_config cfg;
    ws_context_config_from_env(&cfg);
    int rc = ws_context_create_with_config(0, &cfg, &ctx);
    if (rc == WS_OK) rc = ws_scene_load_json(argv[2], &scene);
    if (rc == WS_OK) rc = ws_pointcloud_load(ctx, argv[1], &pc);
    if (rc == WS_OK && ref) rc = ws_pointcloud_load(ctx, ref, &ref_pc);
    const uint32_t n = rc == WS_OK ? ws_scene_cameras(scene, split, 0, nullptr) : 0;
    std::vector<ws_scene_camera> cams(n);
    std::vector<ws_image_metrics> recs(n);
    uint32_t frames = 0, count = 0;
    if (rc == WS_OK && n == 0) {
        std::fprintf(stderr, "the split has no cameras\n");
        rc = WS_ERR_INVALID;
    }
    if (rc == WS_OK) ws_scene_cameras(scene, split, n, cams.data());
    if (rc == WS_OK && compare) rc = ws_metrics_create(ctx, n, &m);
    // the table of per-camera PSNR and SSIM and their means, of the scene as it is now
    auto table = [&]() {
        int trc = ws_metrics_reset(m, nullptr);
        if (trc == WS_OK) trc = ws_scene_evaluate(ctx, pc, scene, split, ref_pc, gt, flags, m, &frames);
        if (trc == WS_OK) trc = ws_metrics_download(m, n, recs.data(), &count);
        if (trc != WS_OK) return trc;
        double psnr = 0.0, ssim = 0.0;
        for (uint32_t i = 0; i < count; ++i) {
            std::printf("%5u %-32s %4ux%-4u PSNR %8.4f  SSIM %.6f\n", cams[i].id, cams[i].img_name, recs[i].width, recs[i].height, recs[i].psnr,
                        recs[i].ssim);
            psnr += recs[i].psnr;
            ssim += recs[i].ssim;
        }
        std::printf("mean over %u images: PSNR %.4f  SSIM %.6f\n", count, psnr / count, ssim / count);
        return (int)WS_OK;
    };
    if (rc == WS_OK && compare) rc = table();
    ws_contrib *err = nullptr, *weight = nullptr;
    if (rc == WS_OK && blame > 0) {
        const uint32_t np = ws_pointcloud_num_points(pc);
        std::vector<uint64_t> e(np), w(np);
        rc = ws_contrib_create(ctx, np, &err);
        if (rc == WS_OK) rc = ws_contrib_create(ctx, np, &weight);
        if (rc == WS_OK) rc = ws_scene_accumulate_error(ctx, pc, scene, split, ref_pc, gt, kind, flags, err, weight, &frames);
        if (rc == WS_OK) rc = ws_contrib_download(err, np, e.data(), nullptr);
        if (rc == WS_OK) rc = ws_contrib_download(weight, np, w.data(), nullptr);
        if (rc == WS_OK) {
            const std::vector<uint32_t> order = top_by(np, blame, [&](uint32_t i) { return e[i]; });
            std::printf("blame (%s error over %u frames): %zu of %u Gaussians by error sum\n",
                        kind == WS_ERROR_SQ ? "sq" : (kind == WS_ERROR_ABS ? "abs" : "dssim"), frames, order.size(), np);
            std::printf("%10s %16s %16s %12s\n", "index", "error sum", "weight sum", "error/weight");
            for (const uint32_t i : order) {
                const double es = (double)e[i] / WS_CONTRIB_SUM_SCALE, wsum = (double)w[i] / WS_CONTRIB_SUM_SCALE;
                std::printf("%10u %16.9f %16.6f %12.6g\n", i, es, wsum, w[i] ? es / wsum : 0.0);
            }
        }
    }
    ws_contrib *effect = nullptr, *drawn = nullptr;
    if (rc == WS_OK && removal > 0) {
        const uint32_t np = ws_pointcloud_num_points(pc);
        std::vector<uint64_t> e(np), w(np);
        rc = ws_contrib_create(ctx, np, &effect);
        if (rc == WS_OK) rc = ws_contrib_create(ctx, np, &drawn);
        if (rc == WS_OK) rc = ws_scene_accumulate_removal(ctx, pc, scene, split, kind, 1.0f, effect, drawn, &frames);
        if (rc == WS_OK) rc = ws_contrib_download(effect, np, e.data(), nullptr);
        if (rc == WS_OK) rc = ws_contrib_download(drawn, np, w.data(), nullptr);
        if (rc == WS_OK) {
            const std::vector<uint32_t> order = top_by(np, removal, [&](uint32_t i) { return e[i]; });
            std::printf("removal (%s effect over %u frames): %zu of %u Gaussians by effect sum\n", kind == WS_ERROR_SQ ? "sq" : "abs", frames, order.size(), np);
            std::printf("%10s %16s %16s %12s\n", "index", "effect sum", "weight sum", "effect/weight");
            for (const uint32_t i : order) {
                const double es = (double)e[i] / WS_CONTRIB_SUM_SCALE, wsum = (double)w[i] / WS_CONTRIB_SUM_SCALE;
                std::printf("%10u %16.9g %16.6f %12.6g\n", i, es, wsum, w[i] ? es / wsum : 0.0);
            }
            uint32_t drawn_n = 0, zero_n = 0;
            for (uint32_t i = 0; i < np; ++i) {
                drawn_n += w[i] != 0;
                zero_n += w[i] != 0 && e[i] == 0;
            }
            std::printf("removal: %u of %u drawn Gaussians have an effect of exactly 0\n", zero_n, drawn_n);
        }
    }
    ws_grad* grad = nullptr;
    ws_contrib* grad_drawn = nullptr;
    if (rc == WS_OK && gradient > 0) {
        const uint32_t np = ws_pointcloud_num_points(pc);
        std::vector<int64_t> q((size_t)np * WS_GRAD_CHANNELS);
        std::vector<uint64_t> w(np);
        rc = ws_grad_create(ctx, np, &grad);
        if (rc == WS_OK) rc = ws_contrib_create(ctx, np, &grad_drawn);
        if (rc == WS_OK) rc = ws_scene_accumulate_gradient(ctx, pc, scene, split, ref_pc, gt, kind, 1.0f, 1.0f, grad, &frames);
        if (rc == WS_OK) rc = ws_scene_accumulate_contrib(ctx, pc, scene, split, grad_drawn, nullptr);
        if (rc == WS_OK) rc = ws_grad_download(grad, np, q.data());
        if (rc == WS_OK) rc = ws_contrib_download(grad_drawn, np, w.data(), nullptr);
        if (rc == WS_OK) {
            const std::vector<uint32_t> order = top_by(np, gradient, [&](uint32_t i) {
                return q[(size_t)i * 4 + 3] < 0 ? 0ull - (uint64_t)q[(size_t)i * 4 + 3] : (uint64_t)q[(size_t)i * 4 + 3];
            });
            std::printf("gradient (%s error over %u frames): %zu of %u Gaussians by |opacity gradient|\n", kind == WS_ERROR_SQ ? "sq" : "abs", frames, order.size(), np);
            std::printf("%10s %16s %16s %16s %16s\n", "index", "d/d ln opacity", "d/d red", "d/d green", "d/d blue");
            for (const uint32_t i : order) {
                const int64_t* g = &q[(size_t)i * 4];
                std::printf("%10u %16.9g %16.9g %16.9g %16.9g\n", i, (double)g[3] / WS_GRAD_SUM_SCALE, (double)g[0] / WS_GRAD_SUM_SCALE,
                            (double)g[1] / WS_GRAD_SUM_SCALE, (double)g[2] / WS_GRAD_SUM_SCALE);
            }
            uint32_t drawn_n = 0, zero_n = 0;
            for (uint32_t i = 0; i < np; ++i) {
                const int64_t* g = &q[(size_t)i * 4];
                drawn_n += w[i] != 0;
                zero_n += w[i] != 0 && g[0] == 0 && g[1] == 0 && g[2] == 0 && g[3] == 0;
            }
            std::printf("gradient: %u of %u drawn Gaussians have all four sums exactly 0\n", zero_n, drawn_n);
        }
    }
    // the densification statistic of the INRIA trainer: the mean norm of the screen-space positional gradient over the frames that saw
    // the Gaussian (websplat.h "Geometry gradients")
    ws_geomgrad* geo = nullptr;
    if (rc == WS_OK && densify > 0) {
        const uint32_t np = ws_pointcloud_num_points(pc);
        std::vector<double> pos((size_t)np * 3), norm(np);
        std::vector<uint64_t> seen(np);
        rc = ws_geomgrad_create(ctx, np, &geo);
        if (rc == WS_OK) rc = ws_scene_accumulate_geometry_gradient(ctx, pc, scene, split, ref_pc, gt, kind, 1.0f, 1.0f, geo, &frames);
        if (rc == WS_OK) rc = ws_geomgrad_download(geo, np, pos.data(), nullptr, norm.data(), seen.data());
        if (rc == WS_OK) {
            const auto mean = [&](uint32_t i) { return seen[i] ? norm[i] / (double)seen[i] : 0.0; };
            const std::vector<uint32_t> order = top_by(np, densify, mean);
            std::printf("densify (%s error over %u frames): %zu of %u Gaussians by screen_norm / seen\n", kind == WS_ERROR_SQ ? "sq" : "abs", frames, order.size(), np);
            std::printf("%10s %16s %8s %16s\n", "index", "screen_norm/seen", "seen", "|d/d position|");
            for (const uint32_t i : order) {
                const double* g = &pos[(size_t)i * 3];
                std::printf("%10u %16.9g %8llu %16.9g\n", i, mean(i), (unsigned long long)seen[i], std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]));
            }
            uint32_t seen_n = 0, zero_n = 0;
            for (uint32_t i = 0; i < np; ++i) {
                seen_n += seen[i] != 0;
                zero_n += seen[i] != 0 && norm[i] == 0.0;
            }
            std::printf("densify: %u of %u seen Gaussians have a norm of exactly 0\n", zero_n, seen_n);
        }
    }
    ws_refit* fit = nullptr;
    if (rc == WS_OK && refit > 0) {
        ws_refit_sh_params sp;
        std::memset(&sp, 0, sizeof sp);
        ws_refit_params& rp = sp.base;
        rp.lr_colour = (float)lr_colour;
        rp.lr_opacity = (float)lr_opacity;
        rp.beta1 = 0.9f;
        rp.beta2 = 0.999f;
        rp.eps = 1e-15f;
        rp.opacity_min = 0.0f;
        sp.lr_sh = lr_sh >= 0.0 ? (float)lr_sh : rp.lr_colour / 20.0f;
        uint32_t steps = 0;
        rc = ws_refit_create(ctx, pc, &fit);
        if (rc == WS_OK)
            rc = refit_sh ? ws_scene_refit_sh(ctx, pc, scene, WS_SPLIT_TRAIN, ref_pc, gt, kind, 1.0f / 128.0f, fit, &sp, (uint32_t)refit, (uint32_t)views_per_step, &steps)
                          : ws_scene_refit(ctx, pc, scene, WS_SPLIT_TRAIN, ref_pc, gt, kind, 1.0f / 128.0f, fit, &rp, (uint32_t)refit, (uint32_t)views_per_step, &steps);
        if (rc == WS_OK) {
            if (refit_sh) std::printf("after refit: %ld epochs, %u steps, SH degree %u\n", refit, steps, ws_pointcloud_sh_deg(pc));
            else std::printf("after refit: %ld epochs, %u steps\n", refit, steps);
            rc = table();
        }
    }
    if (rc == WS_OK && save) {
        rc = ws_pointcloud_save_ply(pc, save);
        if (rc == WS_OK) {
            long bytes = -1;
            if (FILE* f = std::fopen(save, "rb")) {
                if (std::fseek(f, 0, SEEK_END) == 0) bytes = std::ftell(f);
                std::fclose(f);
            }
            std::printf("saved %s: %u Gaussians, %ld bytes\n", save, ws_pointcloud_num_points(pc), bytes);
        }
    }
    if (rc != WS_OK) {
        std::fprintf(stderr, "error %d: %s\n", rc, ws_last_error());
    }
    if (fit) ws_refit_destroy(fit);
    if (grad) ws_grad_destroy(grad);
    if (grad_drawn) ws_contrib_destroy(grad_drawn);
    if (geo) ws_geomgrad_destroy(geo);
    if (effect) ws_contrib_destroy(effect);
    if (drawn) ws_contrib_destroy(drawn);
    if (err) ws_contrib_destroy(err);
    if (weight) ws_contrib_destroy(weight);
    if (m) ws_metrics_destroy(m);
    if (ref_pc) ws_pointcloud_destroy(ref_pc);
    if (pc) ws_pointcloud_destroy(pc);
    if (scene) ws_scene_destroy(scene);
    if (ctx) ws_context_destroy(ctx);
    return rc == WS_OK ? 0 : 1;
}
