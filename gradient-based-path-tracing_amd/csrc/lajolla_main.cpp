// lajolla_main.cpp — drop-in `./lajolla [-t num_threads] [-o output_file_name] filename.xml` for the
// GradPath path (reference CLI: src/main.cpp:11-51). Host C++ over the C ABI in include/gdpt.h.
//
// Same flags, same stdout lines ("Parsing and constructing scene ...", "Done. Took X seconds.",
// "Rendering...", "Image written to ..."), same output-name quirk (with several scenes the first
// scene's name sticks, src/main.cpp:42). Extra flags, because the reference hard-codes them:
//   --spp N       samples per pixel (default: the scene's <sampler sampleCount>)
//   --ref-spp     the reference's hard-coded 1000 spp (src/render.cpp:293)
//   --rng tile|sample   PCG stream assignment (default sample; tile = the reference's order, slow)
//   --alpha A     Poisson data weight (default 0.04, src/render.cpp:353)
//   --device D    GPU index
//   --film WxH    replace the scene's <film> extent (benchmark configurations quote their own)
//   --gpus N      shard the tile loop into N row bands over devices 0..N-1 (gdpt_multi_*: one host thread per GPU, as
//                 the reference's -t threads share the tile grid, src/parallel.cpp:183-256); --devices a,b,.. names them
//   --exchange rccl|peer   transport of the halo row + all-gather between the bands (default rccl)
//   --plan-rows R   cut every pixel's samples into work items as for a band of R rows (GdptRenderParams::plan_rows): a
//                 single-device run with the R of an N-band run (its largest band) writes that run's image bit for bit
//   --reconstruct l2|l1   final reconstruction: l2 = the reference's fourierSolve (default), l1 = IRLS, robust to fireflies in
//                 the gradient buffers (include/gdpt.h: gdpt_reconstruct); --irls-iters N reweighted rounds (default 20),
//                 --irls-eps INIT[,DECAY[,FLOOR]] (default 0.05,0.5,1e-3). Single device only
//                 wl2 | wl1 = the variance-weighted reconstruction of a session (gdpt_reconstruct_weighted: generalised least
//                 squares / its IRLS form on the session's per-pixel variances); they need --pass-spp. --conf-floor X: the
//                 confidence floor (default 0.05); --confidence FILE writes kappa of the data, x-edge and y-edge rows as the
//                 three channels of an image
//   --pass-spp N  progressive session (include/gdpt.h: gdpt_progressive_*): passes of N samples per pixel up to the budget --spp; the
//                 output is the session's reconstruction (Integrator::Path scenes: the mean). --target-error E stops at the first
//                 pass (from the second on) whose estimated relative RMSE of the primal is <= E; --variance FILE writes the
//                 variance of the primal mean. Single device, --rng sample only
//   --sample-devices a,b,..   the session's samples split over these devices (HIP ordinals, repeats allowed) on the sample axis
//                 (gdpt_progressive_group_*: device i draws streams [i B / N, (i+1) B / N) of every pixel's block of B = --spp, the
//                 merged total is what is reconstructed). Needs --pass-spp; not with --gpus / --devices (row bands are another thing)
//                 --target-recon-error E (in the place of --target-error) stops on the estimated relative RMSE of the RECONSTRUCTION,
//                 taken from the spread of the members' own reconstructions (gdpt_progressive_group_run_recon); --error-map FILE
//                 writes that estimate's per-pixel variance map (all three channels), --error-radius R (0..8) averages it over a
//                 (2R+1)^2 window. They need two or more entries (0,0 is fine on one GPU): one session has no independent halves
//   --denoised FILE   also writes the session's primal mean (buffer 0: the image of an Integrator::Path scene, the primal of a GradPath
//                 scene) filtered by non-local means on its per-pixel variance (gdpt_progressive_denoise); -o receives what it
//                 receives without the flag. --nlm-window R (0..10, default 10), --nlm-patch F (0..3, default 3), --nlm-k K (default
//                 0.45). Needs --pass-spp: the filter is driven by the variance of the mean, and no variance exists without passes
//                 --nlm-guide albedo,normal[,depth] lets first-hit features cap the colour weights (gdpt_progressive_denoise_guided):
//                 one group per name, rendered with --feature-spp samples along the session's own camera rays. depth needs
//                 --nlm-depth-tau T, a squared world-space distance (no default: the scale of depth belongs to the scene); --nlm-kf
//                 sets k_f (default 0.6). With --nlm-guide and no --nlm-k, k is 1.0: features only ever lower a weight, so their
//                 gain shows once the colour term is loosened. Without --nlm-guide every output file is what it was
//                 --nlm-demodulate filters the illumination, not the colour (gdpt_progressive_denoise_demod): the mean is divided by
//                 the first-hit albedo (rendered with --feature-spp samples, coverage counted in), the quotient is filtered and the
//                 albedo multiplied back; --nlm-albedo-floor X is the least divisor (default 1e-3). It combines with --nlm-guide
//                 normal[,depth], not with a guide that names albedo: the albedo is already divided out, so an albedo group only
//                 takes samples away. Without --nlm-demodulate every output file is what it was
//                 --nlm-var-smooth S (0..4) runs the chosen filter on the variance averaged over a (2S+1)^2 window
//                 (gdpt_progressive_denoise_smoothed): the variance of a few passes is mostly noise, and it sets the weights. With
//                 --nlm-demodulate the average is taken of variance / albedo^2. It combines with --nlm-guide and --nlm-demodulate.
//                 Without --nlm-var-smooth every output file is what it was
//                 --nlm-levels L (1..4) runs the chosen filter on L levels of a 2 x 2 mean pyramid and replaces each level's low
//                 frequencies by the filtered coarser level (gdpt_progressive_denoise_multiscale): the blotches a single window
//                 cannot reach. It combines with --nlm-guide, --nlm-demodulate and --nlm-var-smooth. Without --nlm-levels every
//                 output file is what it was
//                 --nlm-regress albedo,normal[,depth] replaces the weighted mean by a weighted linear fit of the colour on the named
//                 first-hit features inside the window, read at the centre pixel (gdpt_progressive_denoise_regress): where the
//                 colour is locally affine in them the weighted mean's bias vanishes, so the weights can be wide. depth needs
//                 --nlm-depth-scale S > 0, a world-space distance (no default: the scale of depth belongs to the scene); --nlm-ridge L
//                 sets the ridge (default 1e-2). With --nlm-regress and no --nlm-guide the guide is the albedo group alone, and with
//                 no --nlm-k, k is 4.0: the configuration measured in DESIGN.md section 4.12. Not combined with --nlm-demodulate,
//                 --nlm-var-smooth or --nlm-levels. Without --nlm-regress every output file is what it was
//                 --nlm-collaborative (with --nlm-regress) gives every pixel the weighted average of all fits whose windows cover
//                 it in the place of its own fit's centre value (gdpt_progressive_denoise_collab). The
//                 result carries no variance estimate: error_out prints as nan. Without the flag every output file is what it was
//                 --atrous-levels L (1..6) writes the edge-avoiding a-trous wavelet filter's result in the place of the non-local
//                 means' (gdpt_progressive_denoise_atrous), the cheap filter for previews: L passes of a 5 x 5 B3-spline kernel whose
//                 taps are spread by 1, 2, 4, .. pixels, every tap weighted by the variance-cancelling pixel distance and capped by
//                 the feature distance. --atrous-k K sets its k (default 2.0). The guide is --nlm-guide's (with --nlm-depth-tau,
//                 --nlm-kf), albedo,normal when the flag is absent; --nlm-demodulate, --nlm-albedo-floor and --feature-spp act as
//                 they do above, and under --nlm-demodulate the default guide is the normal alone. Not combined with --nlm-window,
//                 --nlm-patch, --nlm-k, --nlm-var-smooth, --nlm-levels or --nlm-regress. Without --atrous-levels every output file
//                 is what it was
//                 --select LIST writes, per pixel, the candidate whose error two independent halves of the samples estimate smallest
//                 (gdpt_progressive_group_denoise_select). LIST names 1..8 of mean,nlm,guided,demod,regress,atrous,atrous-demod,collab, each
//                 once, separated by commas; each is what its own flag gives without further flags: mean the unfiltered mean; nlm
//                 the plain filter (k 0.45); guided --nlm-guide albedo,normal (k 1.0); demod --nlm-demodulate (no guide); regress
//                 --nlm-regress albedo,normal (the albedo group as guide, k 4.0); collab the same with --nlm-collaborative; atrous --atrous-levels 5 (guide albedo,normal);
//                 atrous-demod --atrous-levels 5 --nlm-demodulate (guide normal). --nlm-var-smooth S acts on nlm, guided and demod;
//                 --nlm-kf on every guide; --nlm-depth-tau T adds the depth group to the guides of guided, atrous and atrous-demod;
//                 --nlm-albedo-floor on demod and atrous-demod; --feature-spp as above. --select-radius S (0..8, default 4) is the
//                 window of the estimate; --select-map FILE writes the index of the winning candidate in LIST (-1: pixel left out)
//                 and --select-mse FILE the winning estimate, in all three channels. It needs --sample-devices with two or more
//                 entries (0,0 is two slices on one GPU); not combined with --nlm-window, --nlm-patch, --nlm-k, --nlm-guide,
//                 --nlm-demodulate, --nlm-levels, --nlm-regress, --nlm-ridge, --nlm-depth-scale, --atrous-levels or --atrous-k.
//                 Without --select every output file is what it was
//                 --nlm-joint (GradPath scenes) writes to FILE the reconstruction of the JOINTLY FILTERED c, cx, cy instead
//                 (gdpt_progressive_denoise_reconstruct): the filter's weights, from the primal and its variance, average the gradients and
//                 all three variances too; -o stays the plain reconstruction. It honours --nlm-window / -patch / -k, --nlm-guide (with
//                 --nlm-kf, --nlm-depth-tau, --feature-spp), --nlm-var-smooth (the weights' variance only), --reconstruct l2 | wl2 | wl1
//                 (the weighted ones on the filtered variances) and --conf-floor; not --reconstruct l1, --nlm-demodulate, --nlm-regress,
//                 --nlm-levels, --atrous-levels, --select or --gpus
//   --features PREFIX   writes the first-hit feature buffers of the film (gdpt_features_render): PREFIX_albedo.exr, PREFIX_normal.exr
//                 and PREFIX_depth.pfm, means over --feature-spp N samples (default min(16, spp)) of the render's own camera rays.
//                 Single device (not with --gpus / --devices / --sample-devices)
//   --frames N    renders N frames of a moving camera on one uploaded scene (gdpt_scene_set_camera) and writes NAME_0000.exr,
//                 NAME_0001.exr, ... from -o NAME.exr. Frame f turns cam_to_world by f times --orbit DEG degrees (default 0) about the
//                 world's vertical (y) axis through the centre of the scene's bounds, and draws the sample window [f spp, (f + 1) spp)
//                 of every pixel's N spp streams in passes of --pass-spp (needed, at least two passes a frame): frames never repeat
//                 samples. Without --temporal a frame's file is its own image (the mean of an Integrator::Path scene, the
//                 reconstruction of a GradPath one). --temporal carries the accumulated primal mean, its variance and the history
//                 length from frame to frame through the first-hit depth (gdpt_temporal_push; --feature-spp as above, default the
//                 frame's spp; --temporal-max-history M, default 32) and writes the accumulated mean; with it --denoised FILE
//                 --atrous-levels L [--atrous-k K] also writes FILE_0000 ..., the a-trous filter on the accumulated mean and variance
//                 under the frame's features (default guide). A camera that leaves the extent the scene was uploaded with is refused.
//                 --temporal-gradients (with --temporal, GradPath scenes) carries the assembled gradients cx, cy and their variances along,
//                 transformed by the Jacobian of the reprojection (gdpt_temporal_push_gradients), and writes to NAME_0000.exr ... the
//                 reconstruction of the accumulated c, cx, cy: --reconstruct l2 (default) | wl2 | wl1, the weighted ones on the
//                 accumulated variances; --denoised stays the a-trous filter on the accumulated primal.
//                 --orbit, --temporal and --temporal-max-history need --frames; none of them is combined with --gpus / --devices,
//                 --sample-devices or --select, nor with the other filter, reconstruction and feature options
// `-t` is accepted for compatibility; rendering runs on the GPU, so it has no effect.
#include "../../include/gdpt.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

namespace {

// NAME.ext -> NAME_0007.ext
std::string frame_name(const std::string &file, int f) {
    char tag[16];
    std::snprintf(tag, sizeof(tag), "_%04d", f);
    const size_t dot = file.find_last_of('.'), slash = file.find_last_of('/');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return file + tag;
    return file.substr(0, dot) + tag + file.substr(dot);
}

// the centre of the bounds of the description's shapes
void scene_centre(const GdptSceneDesc *desc, double c[3]) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int s = 0; s < desc->num_shapes; s++) {
        const GdptShape &sh = desc->shapes[s];
        if (sh.type == GDPT_SHAPE_SPHERE)
            for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], sh.center[k] - sh.radius); hi[k] = std::max(hi[k], sh.center[k] + sh.radius); }
        else if (sh.positions)
            for (int i = 0; i < sh.num_vertices; i++)
                for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], sh.positions[3 * i + k]); hi[k] = std::max(hi[k], sh.positions[3 * i + k]); }
    }
    for (int k = 0; k < 3; k++) c[k] = lo[k] <= hi[k] ? 0.5 * (lo[k] + hi[k]) : 0.0;
}

// `cam` with cam_to_world turned by `deg` degrees about the vertical axis through c: T(c) R_y(deg) T(-c) cam_to_world
GdptCamera orbit_camera(const GdptCamera &cam, const double c[3], double deg) {
    const double a = deg * 3.14159265358979323846 / 180.0, cs = std::cos(a), sn = std::sin(a);
    // rows of T(c) R_y T(-c)
    const double R[4][4] = {{cs, 0, sn, c[0] - cs * c[0] - sn * c[2]}, {0, 1, 0, 0}, {-sn, 0, cs, c[2] + sn * c[0] - cs * c[2]}, {0, 0, 0, 1}};
    GdptCamera out = cam;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = 0;
            for (int k = 0; k < 4; k++) v += R[i][k] * cam.cam_to_world[4 * k + j];
            out.cam_to_world[4 * i + j] = v;
        }
    return out;
}

struct FrameOptions {
    int frames = 0, spp = 0, pass_spp = 0, feature_spp = 0, max_history = 0, device = 0;
    double orbit = 0.0, alpha = 0.04;
    bool temporal = false, atrous = false, gradients = false;
    int recon_norm = GDPT_RECON_L2;      // with gradients: the reconstruction of the accumulated triple ...
    bool recon_weighted = false;         // ... on its accumulated variances (wl2 | wl1)
    GdptAtrousParams atrous_params{};
    std::string output, denoised;
};

// --frames: returns 0, or the status main ends with (the message is printed)
int render_frames(GdptScene *scene, const GdptSceneDesc *desc, const FrameOptions &o) {
    const int w = desc->camera.width, h = desc->camera.height;
    const bool path = desc->integrator == GDPT_INTEGRATOR_PATH;
    const int spp = o.spp > 0 ? o.spp : desc->samples_per_pixel;
    if (spp < 2 * o.pass_spp) { std::cerr << "--frames: a frame's spp must hold at least two passes of --pass-spp" << std::endl; return 2; }
    const size_t plane = (size_t)w * h;
    std::vector<double> mean(plane * 3), var(plane * 3), out(plane * 3), var_out(plane * 3), filtered(plane * 3);
    std::vector<double> fmean(plane * GDPT_FEATURE_CHANNELS), fvar(plane * GDPT_FEATURE_CHANNELS);
    // --temporal-gradients: the session's other four means, the assembled cx, cy, the three assembled variances, the accumulated
    // gradients with their variances, and the reconstruction of the accumulated triple
    std::vector<std::vector<double>> raw(4), asm_var(3), grad(2), grad_out(4);
    std::vector<double> recon_out;
    if (o.gradients) {
        for (auto *set : {&raw, &asm_var, &grad, &grad_out}) for (auto &b : *set) b.resize(plane * 3);
        recon_out.resize(plane * 3);
    }
    double centre[3];
    scene_centre(desc, centre);
    GdptTemporal *temporal = nullptr;
    GdptTemporalParams tp{};
    gdpt_temporal_default_params(&tp);
    if (o.max_history > 0) tp.max_history = o.max_history;
    GdptNlmGuide guide{};
    gdpt_nlm_default_guide(&guide);
    auto fail = [&]() { std::cerr << "terminate: " << gdpt_last_error() << std::endl; gdpt_temporal_free(temporal); return 134; };
    if (o.temporal && gdpt_temporal_create(w, h, o.device, nullptr, &temporal) != 0) return fail();
    GdptProgressiveConfig cfg{};
    cfg.mode = path ? GDPT_PROGRESSIVE_PATH : GDPT_PROGRESSIVE_GRADPATH; cfg.shift_mode = GDPT_SHIFT_REFERENCE; cfg.budget_spp = o.frames * spp;
    for (int f = 0; f < o.frames; f++) {
        const GdptCamera cam = orbit_camera(desc->camera, centre, f * o.orbit);
        if (gdpt_scene_set_camera(scene, &cam) != 0) return fail();
        GdptProgressive *session = nullptr;
        int rc = gdpt_progressive_create_slice(scene, &cfg, f * spp, spp, nullptr, &session);
        for (int done = 0; rc == 0 && done < spp; done += o.pass_spp) rc = gdpt_progressive_add_pass(session, std::min(o.pass_spp, spp - done), nullptr);
        double *means[5] = {mean.data(), nullptr, nullptr, nullptr, nullptr}, *vars[5] = {var.data(), nullptr, nullptr, nullptr, nullptr};
        double *asm_vars[3] = {nullptr, nullptr, nullptr};
        if (o.gradients) {
            for (int k = 0; k < 4; k++) means[1 + k] = raw[k].data();
            for (int k = 0; k < 3; k++) asm_vars[k] = asm_var[k].data();
        }
        if (rc == 0) rc = gdpt_progressive_read(session, 0, means, vars, o.gradients ? asm_vars : nullptr);
        const double *image = mean.data();
        if (rc == 0 && !o.temporal && !path) { rc = gdpt_progressive_reconstruct(session, o.alpha, nullptr, 0, out.data(), nullptr); image = out.data(); }
        const std::string err = rc != 0 ? gdpt_last_error() : "";
        gdpt_progressive_free(session);
        if (rc != 0) { std::cerr << "terminate: " << err << std::endl; gdpt_temporal_free(temporal); return 134; }
        GdptTemporalStats ts{};
        GdptTemporalGradStats gs{};
        if (o.temporal) {
            GdptRenderParams fp{};
            fp.spp = o.feature_spp > 0 ? o.feature_spp : spp; fp.rng_scheme = GDPT_RNG_SAMPLE;
            const GdptSampleWindow win{o.frames * spp, f * spp};
            if (gdpt_features_render(scene, &fp, &win, fmean.data(), fvar.data(), nullptr) != 0) return fail();
            if (o.gradients) {
                // cx = cx0 + cx1(x - 1, y), cy = cy0 + cy1(x, y - 1): one addition a value, the bits of gdpt_assemble_device
                const size_t row = (size_t)w * 3;
                for (size_t i = 0; i < plane * 3; i++) {
                    grad[0][i] = (i % row < 3) ? raw[0][i] : raw[0][i] + raw[2][i - 3];
                    grad[1][i] = (i < row) ? raw[1][i] : raw[1][i] + raw[3][i - row];
                }
                if (gdpt_temporal_push_gradients(temporal, &cam, mean.data(), asm_var[0].data(), fmean.data(), grad[0].data(), asm_var[1].data(),
                                                 grad[1].data(), asm_var[2].data(), &tp, nullptr, out.data(), var_out.data(), nullptr,
                                                 grad_out[0].data(), grad_out[1].data(), grad_out[2].data(), grad_out[3].data(), nullptr, &gs) != 0)
                    return fail();
                ts = gs.base;
                if (o.recon_weighted) {
                    GdptWeightedReconParams wp{};
                    wp.recon.norm = o.recon_norm;
                    if (gdpt_reconstruct_weighted(w, h, out.data(), grad_out[0].data(), grad_out[2].data(), var_out.data(), grad_out[1].data(),
                                                  grad_out[3].data(), o.alpha, &wp, recon_out.data(), nullptr, nullptr) != 0) return fail();
                } else {
                    GdptReconParams rp{};
                    rp.norm = GDPT_RECON_L2;
                    if (gdpt_reconstruct(w, h, out.data(), grad_out[0].data(), grad_out[2].data(), o.alpha, &rp, recon_out.data(), nullptr) != 0) return fail();
                }
            } else if (gdpt_temporal_push(temporal, &cam, mean.data(), var.data(), fmean.data(), &tp, out.data(), var_out.data(), nullptr, &ts) != 0) return fail();
            image = o.gradients ? recon_out.data() : out.data();
            if (o.atrous) {
                if (gdpt_denoise_atrous(w, h, out.data(), var_out.data(), fmean.data(), fvar.data(), GDPT_FEATURE_CHANNELS, &o.atrous_params, &guide, nullptr,
                                        filtered.data(), nullptr, nullptr) != 0) return fail();
                if (gdpt_imwrite(frame_name(o.denoised, f).c_str(), w, h, filtered.data()) != 0) return fail();
            }
        }
        const std::string name = frame_name(o.output, f);
        if (gdpt_imwrite(name.c_str(), w, h, image) != 0) return fail();
        std::cout << "[gdpt] frame " << f << ": orbit " << f * o.orbit << " degrees, " << spp << " spp";
        if (o.temporal)
            std::cout << ", mean history " << ts.sum_history / (double)plane << " frames, " << ts.pixels_reset << " pixels reset, " << ts.pixels_background
                      << " background, " << ts.pixels_left_out << " left out, push " << ts.push_ms << " ms";
        if (o.gradients)
            std::cout << ", mean gradient history " << gs.sum_gradient_history / (double)plane << " frames, " << gs.pixels_gradient_reset
                      << " gradients reset";
        std::cout << ", written to " << name << std::endl;
    }
    gdpt_temporal_free(temporal);
    return 0;
}

} // namespace

int main(int argc, char *argv[]) {
    if (argc <= 1) {
        std::cout << "[Usage] ./lajolla [-t num_threads] [-o output_file_name] filename.xml" << std::endl;
        return 0;
    }
    int num_threads = 0, spp = 0, device = 0, rng = GDPT_RNG_SAMPLE, shift = GDPT_SHIFT_REFERENCE;
    int film_w = 0, film_h = 0, plan_rows = 0, pass_spp = 0;
    double target_error = 0.0, target_recon_error = 0.0;
    int error_radius = 0;
    bool error_radius_set = false;
    std::string error_map_file = "";
    std::string variance_file = "", confidence_file = "";
    bool weighted = false;
    std::string denoised_file = "";
    GdptNlmParams nlm{};
    gdpt_nlm_default_params(&nlm);
    bool nlm_option = false, nlm_k_set = false, nlm_guide_option = false, nlm_demodulate = false;
    double nlm_albedo_floor = 0.0;
    int nlm_var_smooth = -1;          // < 0: not given
    bool nlm_joint = false;
    int nlm_levels = 0;               // 0: not given
    std::string features_prefix = "", nlm_guide_names = "", nlm_regress_names = "";
    double nlm_ridge = 0.0, nlm_depth_scale = 0.0;
    bool nlm_regress_option = false, nlm_collaborative = false;
    int atrous_levels = 0;            // 0: not given
    double atrous_k = 0.0;
    bool atrous_k_set = false;
    int feature_spp = 0;
    int frames = 0, temporal_max_history = 0;      // 0: not given
    double orbit = 0.0;
    bool orbit_set = false, temporal_on = false, temporal_gradients = false, reconstruct_set = false;
    std::string select_list = "", select_map_file = "", select_mse_file = "";
    int select_radius = 4;
    bool select_radius_set = false;
    double nlm_depth_tau = 0.0, nlm_kf = 0.0;
    double conf_floor = 0.0;
    GdptMultiConfig multi{};          // num_devices == 0: single-device entry points
    std::vector<int32_t> sample_devices;      // --sample-devices: a progressive group
    GdptReconParams recon{};          // norm == GDPT_RECON_L2: the reference's reconstruction
    double alpha = 0.04;
    std::string outputfile = "";
    std::vector<std::string> filenames;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::cerr << "missing value for " << a << std::endl; std::exit(2); } return argv[++i]; };
        if (a == "-t") num_threads = std::stoi(next());
        else if (a == "-o") outputfile = next();
        else if (a == "--spp") spp = std::stoi(next());
        else if (a == "--ref-spp") spp = 1000;
        else if (a == "--alpha") alpha = std::stod(next());
        else if (a == "--device") device = std::stoi(next());
        else if (a == "--film") {
            std::string v = next();
            size_t xpos = v.find('x');
            if (xpos == std::string::npos) { std::cerr << "--film expects WxH" << std::endl; return 2; }
            film_w = std::stoi(v.substr(0, xpos)); film_h = std::stoi(v.substr(xpos + 1));
        }
        else if (a == "--gpus") {
            multi.num_devices = std::stoi(next());
            if (multi.num_devices < 1 || multi.num_devices > GDPT_MULTI_MAX_DEVICES) { std::cerr << "--gpus out of range" << std::endl; return 2; }
            for (int k = 0; k < multi.num_devices; k++) multi.devices[k] = k;
        }
        else if (a == "--devices") {      // comma-separated HIP ordinals, band order
            std::string v = next();
            multi.num_devices = 0;
            size_t pos = 0;
            while (pos <= v.size()) {
                size_t c = v.find(',', pos);
                if (c == std::string::npos) c = v.size();
                if (multi.num_devices >= GDPT_MULTI_MAX_DEVICES) { std::cerr << "--devices: too many" << std::endl; return 2; }
                multi.devices[multi.num_devices++] = std::stoi(v.substr(pos, c - pos));
                pos = c + 1;
            }
        }
        else if (a == "--sample-devices") {
            std::string v = next();
            sample_devices.clear();
            size_t pos = 0;
            while (pos <= v.size()) {
                size_t c = v.find(',', pos);
                if (c == std::string::npos) c = v.size();
                if (sample_devices.size() >= GDPT_MULTI_MAX_DEVICES) { std::cerr << "--sample-devices: too many" << std::endl; return 2; }
                if (c == pos || v.find_first_not_of("0123456789", pos) < c || c - pos > 9) { std::cerr << "--sample-devices expects a,b,.. (HIP device ordinals)" << std::endl; return 2; }
                sample_devices.push_back(std::stoi(v.substr(pos, c - pos)));
                pos = c + 1;
            }
        }
        else if (a == "--exchange") {
            std::string v = next();
            if (v == "rccl") multi.exchange = GDPT_EXCHANGE_RCCL;
            else if (v == "peer") multi.exchange = GDPT_EXCHANGE_PEER_COPY;
            else { std::cerr << "unknown --exchange " << v << " (rccl | peer)" << std::endl; return 2; }
        }
        else if (a == "--plan-rows") plan_rows = std::stoi(next());
        else if (a == "--pass-spp") { pass_spp = std::stoi(next()); if (pass_spp <= 0) { std::cerr << "--pass-spp must be > 0" << std::endl; return 2; } }
        else if (a == "--target-error") target_error = std::stod(next());
        else if (a == "--target-recon-error") target_recon_error = std::stod(next());
        else if (a == "--error-map") error_map_file = next();
        else if (a == "--error-radius") { error_radius = std::stoi(next()); error_radius_set = true; }
        else if (a == "--variance") variance_file = next();
        else if (a == "--denoised") denoised_file = next();
        else if (a == "--nlm-window") { nlm.window_radius = std::stoi(next()); nlm_option = true; }
        else if (a == "--nlm-patch") { nlm.patch_radius = std::stoi(next()); nlm_option = true; }
        else if (a == "--nlm-k") { nlm.k = std::stod(next()); nlm_option = true; nlm_k_set = true; }
        else if (a == "--nlm-guide") nlm_guide_names = next();
        else if (a == "--nlm-depth-tau") { nlm_depth_tau = std::stod(next()); nlm_guide_option = true; }
        else if (a == "--nlm-kf") { nlm_kf = std::stod(next()); nlm_guide_option = true; }
        else if (a == "--nlm-regress") nlm_regress_names = next();
        else if (a == "--nlm-collaborative") nlm_collaborative = true;
        else if (a == "--nlm-ridge") { nlm_ridge = std::stod(next()); nlm_regress_option = true; }
        else if (a == "--nlm-depth-scale") { nlm_depth_scale = std::stod(next()); nlm_regress_option = true; }
        else if (a == "--atrous-levels") {
            atrous_levels = std::stoi(next());
            if (atrous_levels < 1 || atrous_levels > GDPT_ATROUS_MAX_LEVELS) { std::cerr << "--atrous-levels takes a number of levels from 1 to 6" << std::endl; return 2; }
        }
        else if (a == "--atrous-k") { atrous_k = std::stod(next()); atrous_k_set = true; }
        else if (a == "--nlm-demodulate") nlm_demodulate = true;
        else if (a == "--nlm-joint") nlm_joint = true;
        else if (a == "--nlm-albedo-floor") nlm_albedo_floor = std::stod(next());
        else if (a == "--nlm-levels") {
            nlm_levels = std::stoi(next());
            if (nlm_levels < 1 || nlm_levels > GDPT_NLM_MAX_LEVELS) { std::cerr << "--nlm-levels takes a number of levels from 1 to 4" << std::endl; return 2; }
        }
        else if (a == "--nlm-var-smooth") {
            nlm_var_smooth = std::stoi(next());
            if (nlm_var_smooth < 0 || nlm_var_smooth > GDPT_VAR_SMOOTH_MAX_RADIUS) { std::cerr << "--nlm-var-smooth takes a radius from 0 to 4" << std::endl; return 2; }
        }
        else if (a == "--frames") { frames = std::stoi(next()); if (frames < 1) { std::cerr << "--frames takes a number of frames >= 1" << std::endl; return 2; } }
        else if (a == "--orbit") { orbit = std::stod(next()); orbit_set = true; if (!std::isfinite(orbit)) { std::cerr << "--orbit takes a finite angle in degrees" << std::endl; return 2; } }
        else if (a == "--temporal") temporal_on = true;
        else if (a == "--temporal-gradients") temporal_gradients = true;
        else if (a == "--temporal-max-history") {
            temporal_max_history = std::stoi(next());
            if (temporal_max_history < 1) { std::cerr << "--temporal-max-history takes a number of frames >= 1" << std::endl; return 2; }
        }
        else if (a == "--select") select_list = next();
        else if (a == "--select-radius") {
            select_radius = std::stoi(next()); select_radius_set = true;
            if (select_radius < 0 || select_radius > GDPT_SELECT_MAX_RADIUS) { std::cerr << "--select-radius takes a radius from 0 to 8" << std::endl; return 2; }
        }
        else if (a == "--select-map") select_map_file = next();
        else if (a == "--select-mse") select_mse_file = next();
        else if (a == "--features") features_prefix = next();
        else if (a == "--feature-spp") { feature_spp = std::stoi(next()); if (feature_spp <= 0) { std::cerr << "--feature-spp must be > 0" << std::endl; return 2; } }
        else if (a == "--rng") { std::string v = next(); rng = (v == "tile") ? GDPT_RNG_TILE : GDPT_RNG_SAMPLE; }
        else if (a == "--shift") {        // extension: "reconnect" = GDPT_SHIFT_RECONNECT (include/gdpt.h); default = the reference's offsets
            std::string v = next();
            if (v == "reconnect") shift = GDPT_SHIFT_RECONNECT;
            else if (v == "reference") shift = GDPT_SHIFT_REFERENCE;
            else { std::cerr << "unknown --shift " << v << " (reference | reconnect)" << std::endl; return 2; }
        }
        else if (a == "--reconstruct") {
            std::string v = next();
            reconstruct_set = true;
            if (v == "l1") recon.norm = GDPT_RECON_L1;
            else if (v == "l2") recon.norm = GDPT_RECON_L2;
            else if (v == "wl1") { recon.norm = GDPT_RECON_L1; weighted = true; }
            else if (v == "wl2") { recon.norm = GDPT_RECON_L2; weighted = true; }
            else { std::cerr << "unknown --reconstruct " << v << " (l2 | l1 | wl2 | wl1)" << std::endl; return 2; }
        }
        else if (a == "--conf-floor") conf_floor = std::stod(next());
        else if (a == "--confidence") confidence_file = next();
        else if (a == "--irls-iters") { int n = std::stoi(next()); recon.irls_iters = n > 0 ? n : -1; }
        else if (a == "--irls-eps") {     // INIT[,DECAY[,FLOOR]]
            std::string v = next();
            double *dst[3] = {&recon.eps_init, &recon.eps_decay, &recon.eps_floor};
            size_t pos = 0;
            for (int k = 0; k < 3 && pos <= v.size(); k++) {
                size_t c = v.find(',', pos);
                if (c == std::string::npos) c = v.size();
                *dst[k] = std::stod(v.substr(pos, c - pos));
                pos = c + 1;
            }
        }
        else filenames.push_back(a);
    }
    if (nlm_joint) {
        if (denoised_file.empty()) { std::cerr << "--nlm-joint needs --denoised" << std::endl; return 2; }
        if (multi.num_devices > 0) { std::cerr << "--nlm-joint is a single-device option (not with --gpus / --devices)" << std::endl; return 2; }
        if (nlm_demodulate || !nlm_regress_names.empty() || nlm_levels > 0 || atrous_levels > 0 || !select_list.empty()) {
            std::cerr << "--nlm-joint is not combined with --nlm-demodulate, --nlm-regress, --nlm-levels, --atrous-levels or --select: the joint filter is the "
                         "plain or guided non-local-means filter on the primal and the gradients" << std::endl;
            return 2;
        }
        if (recon.norm == GDPT_RECON_L1 && !weighted) {
            std::cerr << "--nlm-joint is not combined with --reconstruct l1: the unweighted IRLS solve has no variant that takes the filtered variances "
                         "(use l2, wl2 or wl1)" << std::endl;
            return 2;
        }
    }
    if (frames == 0 && (orbit_set || temporal_on || temporal_max_history > 0)) {
        std::cerr << "--orbit, --temporal and --temporal-max-history need --frames" << std::endl;
        return 2;
    }
    if (temporal_gradients && !temporal_on) { std::cerr << "--temporal-gradients needs --temporal (and --frames)" << std::endl; return 2; }
    if (frames > 0 && reconstruct_set && !temporal_gradients) {
        std::cerr << "--frames takes --reconstruct only with --temporal-gradients: the reconstruction of the accumulated c, cx, cy" << std::endl;
        return 2;
    }
    if (temporal_gradients && recon.norm == GDPT_RECON_L1 && !weighted) {
        std::cerr << "--temporal-gradients takes --reconstruct l2 | wl2 | wl1 (not l1)" << std::endl;
        return 2;
    }
    if (frames > 0) {
        if (multi.num_devices > 0 || !sample_devices.empty() || !select_list.empty()) {
            std::cerr << "--frames, --orbit and --temporal are single-device options (not with --gpus / --devices, --sample-devices or --select)" << std::endl;
            return 2;
        }
        if (pass_spp <= 0) { std::cerr << "--frames needs --pass-spp: a frame is a session of at least two passes, so that a variance exists" << std::endl; return 2; }
        if (temporal_max_history > 0 && !temporal_on) { std::cerr << "--temporal-max-history needs --temporal" << std::endl; return 2; }
        if (!denoised_file.empty() && !(temporal_on && atrous_levels > 0)) {
            std::cerr << "--frames writes --denoised only with --temporal and --atrous-levels: the a-trous filter on the accumulated mean" << std::endl;
            return 2;
        }
        if (nlm_option || !nlm_guide_names.empty() || nlm_guide_option || nlm_demodulate || nlm_var_smooth >= 0 || nlm_joint || nlm_levels > 0 ||
            !nlm_regress_names.empty() || nlm_regress_option || nlm_collaborative || !features_prefix.empty() || !variance_file.empty() ||
            !confidence_file.empty() || ((weighted || recon.norm != GDPT_RECON_L2) && !temporal_gradients) || target_error != 0.0 || target_recon_error != 0.0 ||
            !error_map_file.empty() || rng == GDPT_RNG_TILE || shift != GDPT_SHIFT_REFERENCE) {
            std::cerr << "--frames is combined with -o, --spp, --pass-spp, --film, --device, --alpha, --feature-spp, --denoised, --atrous-levels and --atrous-k only"
                      << std::endl;
            return 2;
        }
    }
    if (recon.norm == GDPT_RECON_L1 && multi.num_devices > 0) { std::cerr << "--reconstruct l1 is a single-device option (not with --gpus / --devices)" << std::endl; return 2; }
    if (!sample_devices.empty() && pass_spp <= 0) { std::cerr << "--sample-devices needs --pass-spp (it splits a progressive session)" << std::endl; return 2; }
    if (!sample_devices.empty() && multi.num_devices > 0) { std::cerr << "--sample-devices splits samples, --gpus / --devices split rows: not together" << std::endl; return 2; }
    if (pass_spp > 0 && multi.num_devices > 0) { std::cerr << "--pass-spp is a single-device option (not with --gpus / --devices)" << std::endl; return 2; }
    if (pass_spp > 0 && rng == GDPT_RNG_TILE) { std::cerr << "--pass-spp needs --rng sample (the tile streams have no sample window)" << std::endl; return 2; }
    if (pass_spp <= 0 && (target_error != 0.0 || !variance_file.empty())) { std::cerr << "--target-error and --variance need --pass-spp" << std::endl; return 2; }
    if (!denoised_file.empty() && pass_spp <= 0) {
        std::cerr << "--denoised needs --pass-spp: the filter is driven by the variance of the mean, and no variance exists without passes" << std::endl;
        return 2;
    }
    // --select: the names of LIST in order; what the single-filter flags would refuse beside each other is refused here at once
    enum { SelMean, SelNlm, SelGuided, SelDemod, SelRegress, SelAtrous, SelAtrousDemod, SelCollab };
    std::vector<int> select_names;
    const bool select_on = !select_list.empty();
    double select_kf = 0.0, select_depth_tau = 0.0, select_floor = 0.0;
    if (select_on) {
        static const char *const names[] = {"mean", "nlm", "guided", "demod", "regress", "atrous", "atrous-demod", "collab"};
        if (denoised_file.empty()) { std::cerr << "--select needs --denoised" << std::endl; return 2; }
        if (sample_devices.size() < 2) {
            std::cerr << "--select needs --sample-devices with two or more entries: the estimate comes from two independent halves of the samples "
                         "(0,0 is two slices on one GPU)" << std::endl;
            return 2;
        }
        if (nlm_option || !nlm_guide_names.empty() || nlm_demodulate || nlm_levels > 0 || !nlm_regress_names.empty() || nlm_regress_option || atrous_levels > 0 ||
            atrous_k_set) {
            std::cerr << "--select is not combined with --nlm-window, --nlm-patch, --nlm-k, --nlm-guide, --nlm-demodulate, --nlm-levels, --nlm-regress, --nlm-ridge, "
                         "--nlm-depth-scale, --atrous-levels or --atrous-k: every name in its list carries its own configuration" << std::endl;
            return 2;
        }
        size_t at = 0;
        while (at <= select_list.size()) {
            const size_t comma = std::min(select_list.find(',', at), select_list.size());
            const std::string name = select_list.substr(at, comma - at);
            int which = -1;
            for (int k = 0; k < 8; k++) if (name == names[k]) which = k;
            if (which < 0 || std::find(select_names.begin(), select_names.end(), which) != select_names.end()) {
                std::cerr << "--select takes mean, nlm, guided, demod, regress, atrous and atrous-demod, each once, separated by commas; and collab, the collaborative "
                             "form of regress, likewise" << std::endl;
                return 2;
            }
            select_names.push_back(which);
            at = comma + 1;
        }
        if (nlm_kf != 0.0 && !(nlm_kf > 0.0)) { std::cerr << "--nlm-kf must be > 0" << std::endl; return 2; }
        if (nlm_depth_tau != 0.0 && !(nlm_depth_tau > 0.0)) { std::cerr << "--nlm-depth-tau must be > 0" << std::endl; return 2; }
        if (nlm_albedo_floor != 0.0 && !(nlm_albedo_floor > 0.0)) { std::cerr << "--nlm-albedo-floor must be > 0" << std::endl; return 2; }
        // taken over here: below they belong to --nlm-guide and --nlm-demodulate
        select_kf = nlm_kf; select_depth_tau = nlm_depth_tau; select_floor = nlm_albedo_floor;
        nlm_kf = nlm_depth_tau = nlm_albedo_floor = 0.0; nlm_guide_option = false;
    } else if (select_radius_set || !select_map_file.empty() || !select_mse_file.empty()) {
        std::cerr << "--select-radius, --select-map and --select-mse need --select" << std::endl;
        return 2;
    }
    if (nlm_option && denoised_file.empty()) { std::cerr << "--nlm-window, --nlm-patch and --nlm-k need --denoised" << std::endl; return 2; }
    GdptNlmGuide guide{};
    gdpt_nlm_default_guide(&guide);
    const bool guided = !nlm_guide_names.empty();
    if (guided) {
        if (denoised_file.empty()) { std::cerr << "--nlm-guide needs --denoised" << std::endl; return 2; }
        guide.num_groups = 0;
        bool seen[3] = {false, false, false};
        size_t at = 0;
        while (at <= nlm_guide_names.size()) {
            const size_t comma = std::min(nlm_guide_names.find(',', at), nlm_guide_names.size());
            const std::string name = nlm_guide_names.substr(at, comma - at);
            const int which = name == "albedo" ? 0 : name == "normal" ? 1 : name == "depth" ? 2 : -1;
            if (which < 0 || seen[which]) { std::cerr << "--nlm-guide takes albedo, normal and depth, each once, separated by commas" << std::endl; return 2; }
            seen[which] = true;
            if (which == 2 && !(nlm_depth_tau > 0.0)) {
                std::cerr << "--nlm-guide depth needs --nlm-depth-tau T > 0, a squared world-space distance: the scale of depth belongs to the scene" << std::endl;
                return 2;
            }
            GdptNlmFeatureGroup &grp = guide.groups[guide.num_groups++];
            grp.first_channel = which == 2 ? 6 : 3 * which; grp.num_channels = which == 2 ? 1 : 3; grp.tau = which == 2 ? nlm_depth_tau : 1e-3;
            at = comma + 1;
        }
        if (nlm_kf != 0.0) guide.k_f = nlm_kf;
        if (!nlm_k_set) nlm.k = 1.0;
    } else if (nlm_guide_option) { std::cerr << "--nlm-depth-tau and --nlm-kf need --nlm-guide" << std::endl; return 2; }
    GdptNlmDemod demod{};
    gdpt_nlm_default_demod(&demod);
    if (nlm_demodulate) {
        if (denoised_file.empty()) { std::cerr << "--nlm-demodulate needs --denoised" << std::endl; return 2; }
        for (int j = 0; j < (guided ? guide.num_groups : 0); j++)
            if (guide.groups[j].first_channel == 0) {
                std::cerr << "--nlm-demodulate is not combined with --nlm-guide albedo: the albedo is already divided out of what is filtered, so an albedo group "
                             "only takes samples away (use --nlm-guide normal[,depth])" << std::endl;
                return 2;
            }
        if (nlm_albedo_floor != 0.0) {
            if (!(nlm_albedo_floor > 0.0)) { std::cerr << "--nlm-albedo-floor must be > 0" << std::endl; return 2; }
            demod.floor = nlm_albedo_floor;
        }
    } else if (nlm_albedo_floor != 0.0) { std::cerr << "--nlm-albedo-floor needs --nlm-demodulate" << std::endl; return 2; }
    GdptNlmRegress regress{};
    gdpt_nlm_default_regress(&regress);
    const bool regressed = !nlm_regress_names.empty();
    if (nlm_collaborative && !regressed) {
        std::cerr << "--nlm-collaborative needs --nlm-regress: it averages the fits of the first-order regression" << std::endl;
        return 2;
    }
    if (regressed) {
        if (denoised_file.empty()) { std::cerr << "--nlm-regress needs --denoised" << std::endl; return 2; }
        if (nlm_demodulate || nlm_var_smooth >= 0 || nlm_levels > 0) {
            std::cerr << "--nlm-regress is not combined with --nlm-demodulate, --nlm-var-smooth or --nlm-levels: the fit is defined on the session's own mean "
                         "and variance at one scale" << std::endl;
            return 2;
        }
        regress.num_regressors = 0;
        bool seen[3] = {false, false, false};
        size_t at = 0;
        while (at <= nlm_regress_names.size()) {
            const size_t comma = std::min(nlm_regress_names.find(',', at), nlm_regress_names.size());
            const std::string name = nlm_regress_names.substr(at, comma - at);
            const int which = name == "albedo" ? 0 : name == "normal" ? 1 : name == "depth" ? 2 : -1;
            if (which < 0 || seen[which]) { std::cerr << "--nlm-regress takes albedo, normal and depth, each once, separated by commas" << std::endl; return 2; }
            seen[which] = true;
            if (which == 2 && !(nlm_depth_scale > 0.0)) {
                std::cerr << "--nlm-regress depth needs --nlm-depth-scale S > 0, a world-space distance: the scale of depth belongs to the scene" << std::endl;
                return 2;
            }
            for (int c = 0; c < (which == 2 ? 1 : 3); c++) {
                regress.channel[regress.num_regressors] = which == 2 ? 6 : 3 * which + c;
                regress.scale[regress.num_regressors++] = which == 2 ? nlm_depth_scale : 1.0;
            }
            at = comma + 1;
        }
        if (nlm_ridge != 0.0) {
            if (!(nlm_ridge > 0.0)) { std::cerr << "--nlm-ridge must be > 0" << std::endl; return 2; }
            regress.ridge = nlm_ridge;
        }
        if (!guided) { guide.num_groups = 1; guide.groups[0] = GdptNlmFeatureGroup{0, 3, 1e-3}; }
        if (!nlm_k_set) nlm.k = 4.0;
    } else if (nlm_regress_option) { std::cerr << "--nlm-ridge and --nlm-depth-scale need --nlm-regress" << std::endl; return 2; }
    GdptAtrousParams atrous{};
    gdpt_atrous_default_params(&atrous);
    const bool atrous_on = atrous_levels > 0;
    if (atrous_on) {
        if (denoised_file.empty()) { std::cerr << "--atrous-levels needs --denoised" << std::endl; return 2; }
        if (nlm_option || nlm_var_smooth >= 0 || nlm_levels > 0 || regressed) {
            std::cerr << "--atrous-levels is not combined with --nlm-window, --nlm-patch, --nlm-k, --nlm-var-smooth, --nlm-levels or --nlm-regress: the a-trous "
                         "filter has no window, no patch and a k of its own (--atrous-k), and is not composed with the other filters" << std::endl;
            return 2;
        }
        atrous.levels = atrous_levels;
        if (atrous_k_set) {
            if (!(atrous_k > 0.0)) { std::cerr << "--atrous-k must be > 0" << std::endl; return 2; }
            atrous.k = atrous_k;
        }
        // without --nlm-guide: albedo and normal (the default guide), the normal alone over a demodulated mean
        if (!guided && nlm_demodulate) { guide.num_groups = 1; guide.groups[0] = GdptNlmFeatureGroup{3, 3, 1e-3}; }
    } else if (atrous_k_set) { std::cerr << "--atrous-k needs --atrous-levels" << std::endl; return 2; }
    if (nlm_var_smooth >= 0 && denoised_file.empty()) { std::cerr << "--nlm-var-smooth needs --denoised" << std::endl; return 2; }
    if (nlm_levels > 0 && denoised_file.empty()) { std::cerr << "--nlm-levels needs --denoised" << std::endl; return 2; }
    if (!features_prefix.empty() && (multi.num_devices > 0 || !sample_devices.empty())) {
        std::cerr << "--features is a single-device option (not with --gpus / --devices / --sample-devices)" << std::endl;
        return 2;
    }
    if (feature_spp > 0 && features_prefix.empty() && !guided && !nlm_demodulate && !regressed && !atrous_on && !select_on && !temporal_on) { std::cerr << "--feature-spp needs --features or --nlm-guide" << std::endl; return 2; }
    if (!features_prefix.empty() && rng == GDPT_RNG_TILE) { std::cerr << "--features needs --rng sample (the feature render draws per-sample streams)" << std::endl; return 2; }
    if (weighted && pass_spp <= 0) { std::cerr << "--reconstruct wl2 | wl1 needs --pass-spp: a one-shot render has no variances" << std::endl; return 2; }
    if (!weighted && (conf_floor != 0.0 || !confidence_file.empty())) { std::cerr << "--conf-floor and --confidence need --reconstruct wl2 | wl1" << std::endl; return 2; }
    const bool recon_error = target_recon_error != 0.0 || !error_map_file.empty();
    if ((recon_error || error_radius_set) && sample_devices.size() < 2) {
        std::cerr << "--target-recon-error, --error-map and --error-radius need --sample-devices with two or more entries: the estimate is the spread of "
                     "the members' reconstructions, and one session has no independent halves" << std::endl;
        return 2;
    }
    if (target_recon_error != 0.0 && target_error != 0.0) { std::cerr << "--target-error and --target-recon-error exclude each other: one target per run" << std::endl; return 2; }
    if (!(target_recon_error >= 0.0)) { std::cerr << "--target-recon-error must be >= 0" << std::endl; return 2; }
    if (error_radius < 0 || error_radius > 8) { std::cerr << "--error-radius must be in [0, 8]" << std::endl; return 2; }
    if (error_radius_set && error_map_file.empty()) { std::cerr << "--error-radius needs --error-map" << std::endl; return 2; }
    if (recon_error && !confidence_file.empty()) { std::cerr << "--confidence is not written with --target-recon-error / --error-map" << std::endl; return 2; }
    (void)num_threads;

    using clock = std::chrono::system_clock;
    for (const std::string &filename : filenames) {
        auto t0 = clock::now();
        std::cout << "Parsing and constructing scene " << filename << "." << std::endl;
        GdptSceneDesc *desc = nullptr;
        if (gdpt_parse_scene_film(filename.c_str(), film_w, film_h, &desc) != 0) {
            std::cerr << "terminate: " << gdpt_last_error() << std::endl;   // the reference dies on an uncaught fl_exception
            return 134;
        }
        if (desc->integrator != GDPT_INTEGRATOR_GRADPATH && desc->integrator != GDPT_INTEGRATOR_PATH) {
            std::cerr << "terminate: this build implements Integrator::GradPath and Integrator::Path (scene asks for another integrator)" << std::endl;
            return 134;
        }
        const bool sharded = multi.num_devices > 0 && desc->integrator == GDPT_INTEGRATOR_GRADPATH;
        const bool grouped = !sample_devices.empty();
        GdptScene *scene = nullptr;
        GdptMulti *mscene = nullptr;
        GdptProgressiveGroup *group = nullptr;
        const bool path = desc->integrator == GDPT_INTEGRATOR_PATH;
        if (nlm_joint && path) {
            std::cerr << "--nlm-joint needs a GradPath scene: an Integrator::Path scene has no gradients to filter beside the image" << std::endl;
            return 2;
        }
        if (temporal_gradients && path) {
            std::cerr << "--temporal-gradients needs a GradPath scene: an Integrator::Path scene renders no gradients" << std::endl;
            return 2;
        }
        GdptProgressiveConfig cfg{};      // of the session or group that --pass-spp asks for
        cfg.mode = path ? GDPT_PROGRESSIVE_PATH : GDPT_PROGRESSIVE_GRADPATH; cfg.shift_mode = shift; cfg.budget_spp = spp;
        if ((grouped   ? gdpt_progressive_group_create(desc, sample_devices.data(), (int)sample_devices.size(), &cfg, &group)
             : sharded ? gdpt_multi_create(desc, &multi, &mscene)
                       : gdpt_scene_upload(desc, device, &scene)) != 0) {
            std::cerr << "terminate: " << gdpt_last_error() << std::endl;
            return 134;
        }
        auto t1 = clock::now();
        std::cout << "Done. Took " << std::chrono::duration<double>(t1 - t0).count() << " seconds." << std::endl;
        std::cout << "Rendering..." << std::endl;
        if (frames > 0) {
            FrameOptions fo;
            fo.frames = frames; fo.spp = spp; fo.pass_spp = pass_spp; fo.feature_spp = feature_spp; fo.max_history = temporal_max_history;
            fo.orbit = orbit; fo.alpha = alpha; fo.device = device; fo.temporal = temporal_on; fo.atrous = atrous_on; fo.atrous_params = atrous;
            fo.gradients = temporal_gradients; fo.recon_norm = recon.norm; fo.recon_weighted = weighted;
            fo.output = outputfile.empty() ? desc->output_filename : outputfile; fo.denoised = denoised_file;
            const int status = render_frames(scene, desc, fo);
            gdpt_scene_free(scene);
            gdpt_free_scene_desc(desc);
            if (status != 0) return status;
            continue;
        }
        const int w = desc->camera.width, h = desc->camera.height;
        std::vector<double> image((size_t)w * h * 3);
        GdptRenderParams p{};
        p.spp = spp; p.rng_scheme = rng; p.shift_mode = shift; p.plan_rows = plan_rows;
        GdptRenderStats rs{};
        GdptPoissonStats ps{};
        GdptMultiStats ms{};
        GdptReconStats cs{};
        // render() dispatches on the integrator (src/render.cpp:374-392)
        int rc;
        GdptProgressiveStatus prog{};
        GdptReconSpreadStats spread{};
        GdptNlmStats nlm_stats{};
        GdptNlmJointStats joint_stats{};
        GdptVarSmoothStats smooth_stats{};
        GdptNlmPyramidStats pyramid_stats{};
        GdptSelectStats select_stats{};
        GdptGroupReconParams gp{};        // the reconstruction the estimate of --target-recon-error / --error-map goes through
        gp.dataCost = alpha; gp.weighted = weighted ? 1 : 0; gp.map_radius = error_radius;
        gp.recon = recon; gp.wrecon.recon = recon; gp.wrecon.conf_floor = conf_floor;
        if (pass_spp > 0) {
            GdptProgressive *session = nullptr;
            if (grouped) {                // the merged total is a session like any other: everything below reads it
                rc = target_recon_error > 0.0 ? gdpt_progressive_group_run_recon(group, target_recon_error, pass_spp, 0, 1, &gp, &prog, nullptr)
                                              : gdpt_progressive_group_run(group, target_error, pass_spp, 0, &prog);
                session = gdpt_progressive_group_total(group);
            } else {
                rc = gdpt_progressive_create(scene, &cfg, nullptr, &session);
                if (rc == 0) rc = gdpt_progressive_run(session, target_error, pass_spp, 0, &prog);
            }
            double *means[5] = {path ? image.data() : nullptr, nullptr, nullptr, nullptr, nullptr};
            if (rc == 0 && path) rc = gdpt_progressive_read(session, 0, means, nullptr, nullptr);
            if (rc == 0 && recon_error) {    // the total's reconstruction (the same bits as below) with the spread of the members' around it
                std::vector<double> emap((size_t)w * h);
                rc = gdpt_progressive_group_reconstruct_error(group, &gp, 0, image.data(), emap.data(), nullptr, &spread, &cs);
                ps.iterations = cs.cg_iters_total; ps.solve_ms = cs.solve_ms;
                if (rc == 0 && !error_map_file.empty()) {
                    std::vector<double> rgb((size_t)w * h * 3);
                    for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 3; k++) rgb[3 * i + k] = emap[i];
                    rc = gdpt_imwrite(error_map_file.c_str(), w, h, rgb.data());
                }
            } else if (rc == 0 && !path && weighted) {
                GdptWeightedReconParams wp{};
                wp.recon = recon; wp.conf_floor = conf_floor;
                GdptWeightedReconStats ws{};
                std::vector<double> kappa[3];
                double *planes[3] = {nullptr, nullptr, nullptr};
                if (!confidence_file.empty()) for (int k = 0; k < 3; k++) { kappa[k].resize((size_t)w * h); planes[k] = kappa[k].data(); }
                rc = gdpt_progressive_reconstruct_weighted(session, alpha, &wp, 0, image.data(), planes, &ws);
                cs = ws.recon;
                ps.iterations = cs.cg_iters_total; ps.solve_ms = cs.solve_ms;
                if (rc == 0 && !confidence_file.empty()) {
                    std::vector<double> conf((size_t)w * h * 3);
                    for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 3; k++) conf[3 * i + k] = kappa[k][i];
                    rc = gdpt_imwrite(confidence_file.c_str(), w, h, conf.data());
                }
            } else if (rc == 0 && !path) {
                rc = gdpt_progressive_reconstruct(session, alpha, recon.norm == GDPT_RECON_L1 ? &recon : nullptr, 0, image.data(), &cs);
                ps.iterations = cs.cg_iters_total; ps.solve_ms = cs.solve_ms;
            }
            if (rc == 0 && !variance_file.empty()) {
                std::vector<double> variance((size_t)w * h * 3);
                double *vars[5] = {variance.data(), nullptr, nullptr, nullptr, nullptr};
                rc = gdpt_progressive_read(session, 0, nullptr, vars, nullptr);
                if (rc == 0) rc = gdpt_imwrite(variance_file.c_str(), w, h, variance.data());
            }
            if (rc == 0 && !denoised_file.empty()) {
                std::vector<double> filtered((size_t)w * h * 3);
                if (select_on) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    const int n = (int)select_names.size();
                    // one set of blocks per kind, as the kind's own flag would set them
                    GdptNlmParams p_plain = nlm, p_guided = nlm, p_regress = nlm;
                    p_guided.k = 1.0; p_regress.k = 4.0;
                    auto with_depth = [&](GdptNlmGuide g) {
                        if (select_kf > 0.0) g.k_f = select_kf;
                        if (select_depth_tau > 0.0) g.groups[g.num_groups++] = GdptNlmFeatureGroup{6, 1, select_depth_tau};
                        return g;
                    };
                    GdptNlmGuide g_default{}, g_normal{}, g_albedo{};
                    gdpt_nlm_default_guide(&g_default);
                    g_normal = g_default; g_normal.num_groups = 1; g_normal.groups[0] = GdptNlmFeatureGroup{3, 3, 1e-3};
                    g_albedo = g_default; g_albedo.num_groups = 1; g_albedo.groups[0] = GdptNlmFeatureGroup{0, 3, 1e-3};
                    if (select_kf > 0.0) g_albedo.k_f = select_kf;
                    g_default = with_depth(g_default); g_normal = with_depth(g_normal);
                    GdptNlmDemod dm{};
                    gdpt_nlm_default_demod(&dm);
                    if (select_floor > 0.0) dm.floor = select_floor;
                    GdptNlmRegress rg{};
                    gdpt_nlm_default_regress(&rg);
                    GdptAtrousParams at{};
                    gdpt_atrous_default_params(&at);
                    std::vector<GdptSelectCandidate> cands((size_t)n);
                    for (int j = 0; j < n; j++) {
                        GdptSelectCandidate &c = cands[(size_t)j];
                        c = GdptSelectCandidate{};
                        c.var_smooth_radius = -1;
                        switch (select_names[(size_t)j]) {
                        case SelMean: c.filter = GDPT_SELECT_MEAN; break;
                        case SelNlm: c.filter = GDPT_SELECT_NLM; c.nlm = &p_plain; c.var_smooth_radius = nlm_var_smooth; break;
                        case SelGuided: c.filter = GDPT_SELECT_NLM_GUIDED; c.nlm = &p_guided; c.guide = &g_default; c.var_smooth_radius = nlm_var_smooth; break;
                        case SelDemod: c.filter = GDPT_SELECT_NLM_DEMOD; c.nlm = &p_plain; c.demod = &dm; c.var_smooth_radius = nlm_var_smooth; break;
                        case SelRegress: c.filter = GDPT_SELECT_NLM_REGRESS; c.nlm = &p_regress; c.guide = &g_albedo; c.regress = &rg; break;
                        case SelAtrous: c.filter = GDPT_SELECT_ATROUS; c.atrous = &at; c.guide = &g_default; break;
                        case SelCollab: c.filter = GDPT_SELECT_NLM_COLLAB; c.nlm = &p_regress; c.guide = &g_albedo; c.regress = &rg; break;
                        default: c.filter = GDPT_SELECT_ATROUS; c.atrous = &at; c.guide = &g_normal; c.demod = &dm; break;
                        }
                    }
                    GdptSelectParams sp{};
                    gdpt_select_default_params(&sp);
                    sp.radius = select_radius;
                    std::vector<int32_t> sel((size_t)w * h);
                    std::vector<double> mse((size_t)w * h);
                    rc = gdpt_progressive_group_denoise_select(group, cands.data(), n, &sp, feature_spp > 0 ? feature_spp : std::min(16, budget), 0, filtered.data(),
                                                               sel.data(), mse.data(), nullptr, nullptr, &select_stats, nullptr);
                    std::vector<double> rgb((size_t)w * h * 3);
                    if (rc == 0 && !select_map_file.empty()) {
                        for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 3; k++) rgb[3 * i + k] = (double)sel[i];
                        rc = gdpt_imwrite(select_map_file.c_str(), w, h, rgb.data());
                    }
                    if (rc == 0 && !select_mse_file.empty()) {
                        for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 3; k++) rgb[3 * i + k] = mse[i];
                        rc = gdpt_imwrite(select_mse_file.c_str(), w, h, rgb.data());
                    }
                } else if (nlm_joint) {      // the reconstruction of the jointly filtered c, cx, cy
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    GdptVarSmoothParams sp{};
                    gdpt_var_smooth_default_params(&sp);
                    sp.radius = nlm_var_smooth;
                    GdptWeightedReconParams wp{};
                    wp.recon = recon; wp.conf_floor = conf_floor;
                    rc = gdpt_progressive_denoise_reconstruct(session, &nlm, guided ? &guide : nullptr, feature_spp > 0 ? feature_spp : std::min(16, budget),
                                                              nlm_var_smooth >= 0 ? &sp : nullptr, alpha, weighted ? &wp : nullptr, 0, filtered.data(), nullptr,
                                                              nullptr, &joint_stats, nullptr);
                    nlm_stats = joint_stats.guide;
                    smooth_stats.radius = nlm_var_smooth;
                } else if (atrous_on) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    rc = gdpt_progressive_denoise_atrous(session, &atrous, &guide, nlm_demodulate ? &demod : nullptr,
                                                         feature_spp > 0 ? feature_spp : std::min(16, budget), 0, filtered.data(), nullptr, nullptr, nullptr,
                                                         &nlm_stats);
                } else if (regressed) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    if (nlm_collaborative)
                        rc = gdpt_progressive_denoise_collab(session, &nlm, &guide, &regress, feature_spp > 0 ? feature_spp : std::min(16, budget), 0,
                                                             filtered.data(), nullptr, nullptr, &nlm_stats);
                    else
                        rc = gdpt_progressive_denoise_regress(session, &nlm, &guide, &regress, feature_spp > 0 ? feature_spp : std::min(16, budget), 0,
                                                              filtered.data(), nullptr, nullptr, nullptr, &nlm_stats);
                } else if (nlm_levels > 0) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    GdptVarSmoothParams sp{};
                    gdpt_var_smooth_default_params(&sp);
                    sp.radius = nlm_var_smooth;
                    rc = gdpt_progressive_denoise_multiscale(session, nlm_demodulate ? GDPT_DENOISE_DEMOD : guided ? GDPT_DENOISE_GUIDED : GDPT_DENOISE_PLAIN,
                                                             nlm_levels, nlm_var_smooth >= 0 ? &sp : nullptr, &nlm, guided ? &guide : nullptr,
                                                             nlm_demodulate ? &demod : nullptr, feature_spp > 0 ? feature_spp : std::min(16, budget), 0,
                                                             filtered.data(), nullptr, nullptr, nullptr, &pyramid_stats);
                    nlm_stats = pyramid_stats.level[0];
                    smooth_stats.radius = nlm_var_smooth;
                } else if (nlm_var_smooth >= 0) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    GdptVarSmoothParams sp{};
                    gdpt_var_smooth_default_params(&sp);
                    sp.radius = nlm_var_smooth;
                    rc = gdpt_progressive_denoise_smoothed(session, nlm_demodulate ? GDPT_DENOISE_DEMOD : guided ? GDPT_DENOISE_GUIDED : GDPT_DENOISE_PLAIN, &sp,
                                                           &nlm, guided ? &guide : nullptr, nlm_demodulate ? &demod : nullptr,
                                                           feature_spp > 0 ? feature_spp : std::min(16, budget), 0, filtered.data(), nullptr, nullptr, nullptr,
                                                           nullptr, &nlm_stats, &smooth_stats);
                } else if (nlm_demodulate) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    rc = gdpt_progressive_denoise_demod(session, &nlm, guided ? &guide : nullptr, &demod, feature_spp > 0 ? feature_spp : std::min(16, budget), 0,
                                                        filtered.data(), nullptr, nullptr, nullptr, &nlm_stats);
                } else if (guided) {
                    const int budget = spp > 0 ? spp : desc->samples_per_pixel;
                    rc = gdpt_progressive_denoise_guided(session, &nlm, &guide, feature_spp > 0 ? feature_spp : std::min(16, budget), 0, filtered.data(),
                                                         nullptr, nullptr, nullptr, &nlm_stats);
                } else rc = gdpt_progressive_denoise(session, &nlm, 0, filtered.data(), nullptr, &nlm_stats);
                if (rc == 0) rc = gdpt_imwrite(denoised_file.c_str(), w, h, filtered.data());
            }
            std::string err = rc != 0 ? gdpt_last_error() : "";
            if (!grouped) gdpt_progressive_free(session);
            if (rc != 0) { std::cerr << "terminate: " << err << std::endl; return 134; }
            rs = prog.totals;
        } else if (sharded) {
            rc = gdpt_multi_gradient_path_render(mscene, &p, alpha, image.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &rs, &ms);
            ps.solve_ms = ms.solve_ms; ps.solver = GDPT_SOLVER_DEFAULT;
        } else if (desc->integrator == GDPT_INTEGRATOR_PATH) rc = gdpt_path_render(scene, &p, image.data(), &rs);
        else if (recon.norm == GDPT_RECON_L1) {
            rc = gdpt_gradient_path_render_recon(scene, &p, alpha, &recon, image.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &rs, &cs);
            ps.iterations = cs.cg_iters_total; ps.solve_ms = cs.solve_ms;
        } else rc = gdpt_gradient_path_render(scene, &p, alpha, image.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &rs, &ps);
        if (rc != 0) {
            std::cerr << "terminate: " << gdpt_last_error() << std::endl;
            return 134;
        }
        if (!features_prefix.empty()) {
            // the camera rays of the render's own first samples: the window {spp, 0} of every pixel's stream block
            const int budget = spp > 0 ? spp : desc->samples_per_pixel;
            GdptRenderParams fp{};
            fp.spp = feature_spp > 0 ? feature_spp : std::min(16, budget); fp.rng_scheme = GDPT_RNG_SAMPLE;
            const GdptSampleWindow win{budget, 0};
            const size_t plane = (size_t)w * h;
            std::vector<double> fmean(plane * GDPT_FEATURE_CHANNELS), fvar(plane * GDPT_FEATURE_CHANNELS), rgb(plane * 3);
            GdptRenderStats fs{};
            rc = gdpt_features_render(scene, &fp, &win, fmean.data(), fvar.data(), &fs);
            static const char *const suffix[3] = {"_albedo.exr", "_normal.exr", "_depth.pfm"};
            for (int k = 0; k < 3 && rc == 0; k++) {
                for (size_t i = 0; i < plane; i++) for (int c = 0; c < 3; c++) rgb[3 * i + c] = fmean[(size_t)(k == 2 ? 6 : 3 * k + c) * plane + i];
                rc = gdpt_imwrite((features_prefix + suffix[k]).c_str(), w, h, rgb.data());
            }
            if (rc != 0) { std::cerr << "terminate: " << gdpt_last_error() << std::endl; return 134; }
            std::cout << "[gdpt] features: " << fp.spp << " samples per pixel, " << fs.rays << " rays, render " << fs.render_ms << " ms, written to "
                      << features_prefix << "_albedo.exr, _normal.exr, _depth.pfm" << std::endl;
        }
        // the reference prints one progress line per finished tile and a final 100% line (src/progress_reporter.h:22-29)
        unsigned long long tiles = (unsigned long long)((w + 15) / 16) * ((h + 15) / 16);
        std::fprintf(stdout, "\r %.2f Percent Done (%llu / %llu)\n", 100.0, tiles, tiles);
        if (outputfile.compare("") == 0) outputfile = desc->output_filename;
        auto t2 = clock::now();
        std::cout << "Done. Took " << std::chrono::duration<double>(t2 - t1).count() << " seconds." << std::endl;
        if (gdpt_imwrite(outputfile.c_str(), w, h, image.data()) != 0) {
            std::cerr << "terminate: " << gdpt_last_error() << std::endl;
            return 134;
        }
        std::cout << "Image written to " << outputfile << std::endl;
        std::cout << "[gdpt] " << rs.samples << " samples, " << rs.rays << " rays, render " << rs.render_ms << " ms ("
                  << (rs.render_ms > 0 ? rs.samples / rs.render_ms / 1e3 : 0.0) << " Msamples/s), Poisson " << ps.iterations
                  << " CG iterations " << ps.solve_ms << " ms, non-finite samples " << rs.nonfinite_samples << std::endl;
        if (pass_spp > 0) {
            static const char *const why[] = {"none", "target", "budget", "max_passes"};
            int budget = prog.budget_spp;
            if (grouped) {                // (the total reports as its budget what has been merged in: the group's is its members' slices together)
                budget = 0;
                for (int k = 0; k < (int)sample_devices.size(); k++) {
                    GdptProgressiveStatus st{};
                    if (gdpt_progressive_group_member_status(group, k, &st) != 0) { std::cerr << "terminate: " << gdpt_last_error() << std::endl; return 134; }
                    budget += st.budget_spp;
                }
            }
            std::cout << "[gdpt] progressive: " << prog.passes << " passes, " << prog.spp_done << " of " << budget
                      << " samples per pixel, error estimate " << prog.error_estimate << " (" << prog.pixels_left_out
                      << " pixels left out), stopped by " << why[prog.stop_reason] << std::endl;
            if (select_on) {
                static const char *const names[] = {"mean", "nlm", "guided", "demod", "regress", "atrous", "atrous-demod", "collab"};
                const double valid = (double)((size_t)w * h - select_stats.pixels_left_out);
                std::cout << "[gdpt] selected: radius " << select_stats.radius << ", " << select_stats.pixels_left_out << " pixels left out;";
                for (int j = 0; j < select_stats.num_candidates; j++)
                    std::cout << " " << names[select_names[(size_t)j]] << " " << (valid > 0 ? 100.0 * (double)select_stats.chosen[j] / valid : 0.0) << " % (error "
                              << (select_stats.sum_sq_out > 0 ? std::sqrt(std::max(0.0, select_stats.sum_e[j]) / select_stats.sum_sq_out) : 0.0) << ");";
                std::cout << " select_ms " << select_stats.select_ms << ", written to " << denoised_file << std::endl;
            } else if (nlm_joint) {
                auto ratio = [](double out, double in) { return in > 0.0 ? out / in : 0.0; };
                std::cout << "[gdpt] joint: " << joint_stats.guide.pixels_left_out << " pixels left out; variance c \u00d7"
                          << ratio(joint_stats.guide.sum_var_out, joint_stats.guide.sum_var_in) << ", cx \u00d7"
                          << ratio(joint_stats.sum_var_out[0], joint_stats.sum_var_in[0]) << ", cy \u00d7"
                          << ratio(joint_stats.sum_var_out[1], joint_stats.sum_var_in[1]) << std::endl;
            } else if (!denoised_file.empty())
                std::cout << "[gdpt] denoised: error_in " << nlm_stats.error_in << ", error_out " << nlm_stats.error_out << " (weights taken as fixed, bias left out; "
                          << nlm_stats.pixels_left_out << " pixels left out), window " << nlm_stats.window_radius << ", patch " << nlm_stats.patch_radius
                          << ", filter_ms " << nlm_stats.filter_ms << (guided ? ", guided by " + nlm_guide_names : std::string())
                          << (atrous_on ? ", a-trous wavelet filter over " + std::to_string(atrous.levels) + " levels (window: the reach of the last)" : std::string())
                          << (regressed ? ", first-order regression on " + nlm_regress_names + " (ridge " + std::to_string(regress.ridge) + ")" : std::string())
                          << (nlm_collaborative ? ", collaborative (no variance estimate)" : "") << (nlm_demodulate ? ", demodulated by the first-hit albedo" : "")
                          << (nlm_var_smooth >= 0 ? ", variance smoothed over radius " + std::to_string(smooth_stats.radius) : std::string())
                          << (nlm_levels > 0 ? ", " + std::to_string(pyramid_stats.levels) + " levels in " + std::to_string(pyramid_stats.total_ms) + " ms (the figures before are the finest level's)" : std::string())
                          << ", written to "
                          << denoised_file
                          << std::endl;
            if (recon_error)
                std::cout << "[gdpt] reconstruction: error estimate " << spread.error_estimate << " from the spread of " << spread.members
                          << " members (" << spread.pixels_left_out << " pixels left out), map radius " << spread.radius << ", spread "
                          << spread.spread_ms << " ms" << std::endl;
        }
        if (grouped) {
            const int n = (int)sample_devices.size();
            int first = 0;                // the slices are contiguous, in member order: each member reports its size
            std::cout << "[gdpt] " << n << " sample slices:";
            for (int k = 0; k < n; k++) {
                GdptProgressiveStatus st{};
                if (gdpt_progressive_group_member_status(group, k, &st) != 0) { std::cerr << "terminate: " << gdpt_last_error() << std::endl; return 134; }
                std::cout << " device " << sample_devices[(size_t)k] << " [" << first << "," << first + st.budget_spp << ") " << st.spp_done << " spp in " << st.passes
                          << " passes, render " << st.totals.render_ms << " ms;";
                first += st.budget_spp;
            }
            std::cout << " last merge " << prog.fold_ms << " ms" << std::endl;
        }
        if (sharded) {
            std::cout << "[gdpt] " << ms.num_devices << " row bands (" << (ms.exchange == GDPT_EXCHANGE_RCCL ? "RCCL" : "peer copies") << "): render";
            for (int k = 0; k < ms.num_devices; k++) std::cout << " " << ms.render_ms[k];
            std::cout << " ms, halo+assemble+gather " << ms.exchange_ms << " ms, solve " << ms.solve_ms << " ms, wall " << ms.wall_ms << " ms" << std::endl;
        }
        gdpt_progressive_group_free(group);
        gdpt_multi_free(mscene);
        gdpt_scene_free(scene);
        gdpt_free_scene_desc(desc);
    }
    return 0;
}
