// denoise_nlm.hip — non-local means with variance-cancelling patch distances on (mean, variance of the mean), for gfx950
// (include/gdpt.h: gdpt_denoise_nlm*, where the definition stands; Rousselle, Knaus, Zwicker 2012, sections 4-5).
//
// Kernels: two forms of the one definition, chosen by the test knob nlm_direct (include/gdpt_debug.h). Both loop over 16 x 16 tiles
// as box_kernel (recon_spread.hip) does, a thread on a pixel of the tile, and both leave block partials through leave_block_sum for
// finish_kernel (image_kernels.h): a fixed order, the same bits every time.
//   direct_kernel   the literal definition: the loops over the window offsets o and the patch taps n read global memory, every
//                   pair distance e_o(p + n) is computed where it is used, (2r+1)^2 (2f+1)^2 of them per pixel.
//   tiled_kernel    the tile and its halo staged in LDS (nlm::Stage, nlm_device.h, where the layout and its banking stand); exp, and
//                   the three numerators, the weight sum and the three w^2 v sums accumulate in registers.
// Both are templates on GUIDED (gdpt_denoise_nlm_guided*). A guided kernel adds the feature planes to a pixel's validity and caps the
// colour weight of a pair (p, p+o) with the pair's feature distance. The thread keeps its own pixel's feature values and variances in
// registers (the loops over groups and channels are unrolled to the caps, so every index is static) and reads those of p+o from global
// memory: the planes are planar, a wave's read of one plane is four 128-byte rows, served from L1 / L2. The stage gets no feature
// planes: at (r, f) = (10, 3) it already takes 108 624 of the 163 840 bytes a workgroup may declare, and 2 x 6 planes of (16 + 2r)^2
// doubles would be another 124 KB.
// And on DEMOD (gdpt_denoise_nlm_demod*). A demodulated kernel filters u / a~, v / a~^2 for the effective albedo a~ of include/gdpt.h:
// load_pixel adds the albedo and coverage planes to a pixel's validity and divides, so the tiled kernel's stage holds the quotients and
// needs no LDS of its own; finish_pixel multiplies a~ back. A thread recomputes its own a~ from the planar planes there, and reloads
// its own original triples for the colour-domain sums: (u / a~) a~ is not always u.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_host.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

namespace nlm {

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void direct_kernel(ArgsOf<GUIDED, DEMOD> a) {
    __shared__ double red[kBlock / 64];
    const int r = a.r;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_pixel(a, x, y, u, v); };
    Sums s;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (!load_pixel(a, x, y, u, v)) { keep_pixel(a, i, u, v, s); continue; }
        OwnFeatures own;
        if constexpr (GUIDED) own.load(a.gd, (size_t)y * a.g.w + x);
        Accum acc;
        for (int oy = -r; oy <= r; oy++)
            for (int ox = -r; ox <= r; ox++) {
                const int qx = x + ox, qy = y + oy;
                if (qx < 0 || qy < 0 || qx >= a.g.w || qy >= a.g.h) continue;
                double uq[3], vq[3];
                if (!load_pixel(a, qx, qy, uq, vq)) continue;
                double S;
                int C;
                patch_distance(a, load, x, y, ox, oy, S, C);      // (C >= 1: the tap n = 0 counts)
                if constexpr (GUIDED) acc.template add<true>(S, C, uq, vq, own.distance(a.gd, (size_t)qy * a.g.w + qx));
                else acc.add(S, C, uq, vq);
            }
        finish_pixel(a, i, u, v, acc, s);
    }
    leave_partials(a, s, red);
}

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void tiled_kernel(ArgsOf<GUIDED, DEMOD> a) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    Stage st;
    st.lay_out(a.r, a.f, lds);
    const int pc = st.pc;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_pixel(a, x, y, u, v); };
    Sums s;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage has been read
        st.fill(a.g, tp.x0, tp.y0, load);
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const bool okp = inside && st.sflag[pc] != 0;
        OwnFeatures own;
        if constexpr (GUIDED) { if (okp) own.load(a.gd, (size_t)y * a.g.w + x); }
        Accum acc;
        st.sweep(a.k2, a.alpha, a.eps, okp, [&](int iq, double S, int C, int oy, int ox) {
            double uq[3], vq[3];
            st.mean(iq, uq); st.variance(iq, vq);
            if constexpr (GUIDED) acc.template add<true>(S, C, uq, vq, own.distance(a.gd, (size_t)(y + oy) * a.g.w + (x + ox)));
            else acc.add(S, C, uq, vq);
        });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (okp) {
            st.mean(pc, u); st.variance(pc, v);
            finish_pixel(a, i, u, v, acc, s);
        } else {
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlm

namespace gdpt {

namespace {

// leaked on purpose: no HIP call is made from a static destructor (as the solver's registry, poisson_kernels.hip); a pair's entry
// goes with forget_stream (device_mem.h)
PerStream<SumsWorkspace> &g_workspaces = *new PerStream<SumsWorkspace>();

// one form of one instantiation, enqueued on `stream`
template <bool GUIDED, bool DEMOD>
void launch_form(const nlm::ArgsOf<GUIDED, DEMOD> &a, bool direct, hipStream_t stream) {
    if (direct) hipLaunchKernelGGL((nlm::direct_kernel<GUIDED, DEMOD>), dim3(a.g.blocks), dim3(film::kBlock), 0, stream, a);
    else launch_staged(nlm::tiled_kernel<GUIDED, DEMOD>, a.g.blocks, a.r, a.f, stream, a, "hipFuncSetAttribute(nlm stage)");
}

// Device pointers on the current device; the arguments have been checked. Enqueued on `stream`; waits for it if `stats` is asked for.
// `guide` (nullable): the guided kernels, on `d_feat`, `d_feat_var`. `demod` (nullable): the demodulated kernels, on the same planes.
void denoise_nlm_launch(int w, int h, const double *d_img, const double *d_var, const GdptNlmParams &p, double *d_out, double *d_var_out,
                        hipStream_t stream, GdptNlmStats *stats, const GdptNlmGuide *guide = nullptr, const double *d_feat = nullptr,
                        const double *d_feat_var = nullptr, const GdptNlmDemod *demod = nullptr) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    SumsWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    ws.prepare("nlm");

    nlm::GuidedArgs a{};
    fill_base(a, w, h, p, d_img, d_var, d_out, d_var_out, ws.partials);
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    if (guide) fill_guide(a.gd, *guide, d_feat, d_feat_var, (size_t)w * h);
    const nlm::Args &plain = a;       // (the unguided kernels take the plain argument block)
    const bool direct = debug_knob("nlm_direct", 0) != 0;
    if (demod) {
        const nlm::Demod dm{d_feat, d_feat_var, (size_t)w * h, demod->albedo_channel, demod->coverage_channel, demod->floor};
        if (guide) {
            nlm::GuidedDemodArgs ad{};
            static_cast<nlm::GuidedArgs &>(ad) = a; ad.dm = dm;
            launch_form<true, true>(ad, direct, stream);
        } else {
            nlm::DemodArgs ad{};
            static_cast<nlm::Args &>(ad) = plain; ad.dm = dm;
            launch_form<false, true>(ad, direct, stream);
        }
    } else if (guide) launch_form<true, false>(a, direct, stream);
    else launch_form<false, false>(plain, direct, stream);
    ck(hipGetLastError(), "nlm launch");
    if (!stats) return;
    ws.read_stats(a.g.blocks, stream, "nlm", stats);
    stats->window_radius = p.window_radius; stats->patch_radius = p.patch_radius;
}

} // namespace

void nlm_check_params(const std::string &who, const GdptNlmParams &p) {
    if (p.window_radius < 0 || p.window_radius > nlm::kMaxR)
        throw std::runtime_error(who + ": window_radius must be in [0, " + std::to_string(nlm::kMaxR) + "]");
    if (p.patch_radius < 0 || p.patch_radius > nlm::kMaxF)
        throw std::runtime_error(who + ": patch_radius must be in [0, " + std::to_string(nlm::kMaxF) + "]");
    if (!std::isfinite(p.k) || !(p.k > 0)) throw std::runtime_error(who + ": k must be finite and > 0");
    if (!std::isfinite(p.alpha) || !(p.alpha >= 0)) throw std::runtime_error(who + ": alpha must be finite and >= 0");
    if (!std::isfinite(p.epsilon) || !(p.epsilon > 0)) throw std::runtime_error(who + ": epsilon must be finite and > 0");
    if (p.reserved[0] != 0 || p.reserved[1] != 0) throw std::runtime_error(who + ": reserved must be 0");
}

void nlm_check_guide(const std::string &who, const GdptNlmGuide &g) {
    if (g.num_channels < 0 || g.num_channels > nlm::kMaxChannels)
        throw std::runtime_error(who + ": num_channels must be in [0, " + std::to_string(nlm::kMaxChannels) + "]");
    if (g.num_groups < 0 || g.num_groups > nlm::kMaxGroups)
        throw std::runtime_error(who + ": num_groups must be in [0, " + std::to_string(nlm::kMaxGroups) + "]");
    for (int j = 0; j < g.num_groups; j++) {
        const GdptNlmFeatureGroup &grp = g.groups[j];
        const std::string at = who + ": groups[" + std::to_string(j) + "]";
        if (grp.num_channels < 1) throw std::runtime_error(at + ".num_channels must be >= 1");
        if (grp.first_channel < 0 || (long long)grp.first_channel + grp.num_channels > (long long)g.num_channels)
            throw std::runtime_error(at + ".first_channel: the group leaves [0, num_channels)");
        if (!std::isfinite(grp.tau) || !(grp.tau > 0)) throw std::runtime_error(at + ".tau must be finite and > 0");
    }
    if (!std::isfinite(g.k_f) || !(g.k_f > 0)) throw std::runtime_error(who + ": k_f must be finite and > 0");
    if (!std::isfinite(g.alpha_f) || !(g.alpha_f >= 0)) throw std::runtime_error(who + ": alpha_f must be finite and >= 0");
    if (g.reserved[0] != 0 || g.reserved[1] != 0) throw std::runtime_error(who + ": guide reserved must be 0");
}

void denoise_nlm_guided_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               const GdptNlmParams &p, const GdptNlmGuide &g, double *d_out, double *d_var_out, hipStream_t stream,
                               GdptNlmStats *stats) {
    denoise_nlm_launch(w, h, d_img, d_var, p, d_out, d_var_out, stream, stats, &g, d_feat, d_feat_var);
}

void nlm_check_demod(const std::string &who, const GdptNlmDemod &d, int num_channels) {
    if (num_channels < 0 || num_channels > nlm::kMaxChannels)
        throw std::runtime_error(who + ": num_channels must be in [0, " + std::to_string(nlm::kMaxChannels) + "]");
    if (d.albedo_channel < 0 || d.albedo_channel > num_channels - 3)
        throw std::runtime_error(who + ": albedo_channel must be in [0, num_channels - 3]");
    if (d.coverage_channel < -1 || d.coverage_channel >= num_channels)
        throw std::runtime_error(who + ": coverage_channel must be in [-1, num_channels)");
    if (d.coverage_channel >= d.albedo_channel && d.coverage_channel < d.albedo_channel + 3)
        throw std::runtime_error(who + ": coverage_channel lies inside the albedo triple");
    if (!std::isfinite(d.floor) || !(d.floor > 0)) throw std::runtime_error(who + ": floor must be finite and > 0");
    if (d.reserved[0] != 0 || d.reserved[1] != 0) throw std::runtime_error(who + ": demod reserved must be 0");
}

void denoise_nlm_demod_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                              const GdptNlmParams &p, const GdptNlmGuide *g, const GdptNlmDemod &d, double *d_out, double *d_var_out,
                              hipStream_t stream, GdptNlmStats *stats) {
    denoise_nlm_launch(w, h, d_img, d_var, p, d_out, d_var_out, stream, stats, g, d_feat, d_feat_var, &d);
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// what both entry points refuse; `who` names the caller. Returns the parameters in force.
GdptNlmParams check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const GdptNlmParams *params,
                              const double *out, const double *var_out) {
    gdpt::check_film(who, width, height, img, var, out, var_out);
    GdptNlmParams p;
    if (params) p = *params;
    else gdpt_nlm_default_params(&p);
    gdpt::nlm_check_params(who, p);
    return p;
}

// ... and what the guided ones refuse beside it. Returns the guide in force.
GdptNlmGuide check_guided_arguments(const std::string &who, const double *feat, const double *feat_var, const GdptNlmGuide *guide,
                                    const double *out, const double *var_out) {
    GdptNlmGuide g;
    if (guide) g = *guide;
    else gdpt_nlm_default_guide(&g);
    gdpt::nlm_check_guide(who, g);
    if (g.num_groups > 0) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    if (feat && (out == feat || out == feat_var)) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && feat && (var_out == feat || var_out == feat_var)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    return g;
}

// ... and the demodulated ones: the guide (`guided`: whether there is one) and the block in force
GdptNlmDemod check_demod_arguments(const std::string &who, const double *feat, const double *feat_var, int num_channels, const GdptNlmGuide *guide,
                                   const GdptNlmDemod *demod, const double *out, const double *var_out) {
    if (guide) {
        gdpt::nlm_check_guide(who, *guide);
        if (guide->num_channels != num_channels) throw std::runtime_error(who + ": guide num_channels must equal num_channels");
    }
    GdptNlmDemod d;
    if (demod) d = *demod;
    else gdpt_nlm_default_demod(&d);
    gdpt::nlm_check_demod(who, d, num_channels);
    if (!feat) throw std::runtime_error(who + ": feat is null");
    if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    if (out == feat || out == feat_var) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && (var_out == feat || var_out == feat_var)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    return d;
}

} // namespace

extern "C" {

void gdpt_nlm_default_params(GdptNlmParams *p) {
    if (!p) return;
    *p = GdptNlmParams{};
    p->window_radius = GDPT_NLM_MAX_WINDOW_RADIUS; p->patch_radius = GDPT_NLM_MAX_PATCH_RADIUS;
    p->k = 0.45; p->alpha = 1.0; p->epsilon = 1e-10;
}

int gdpt_denoise_nlm_device(int width, int height, const double *d_img, const double *d_var, const GdptNlmParams *params, double *d_out,
                            double *d_var_out, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_device";
        const GdptNlmParams p = check_arguments(who, width, height, d_img, d_var, params, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_launch(width, height, d_img, d_var, p, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

void gdpt_nlm_default_guide(GdptNlmGuide *g) {
    if (!g) return;
    *g = GdptNlmGuide{};
    g->num_channels = GDPT_FEATURE_CHANNELS; g->num_groups = 2;
    g->groups[0] = GdptNlmFeatureGroup{0, 3, 1e-3};      // albedo
    g->groups[1] = GdptNlmFeatureGroup{3, 3, 1e-3};      // shading normal
    g->k_f = 0.6; g->alpha_f = 1.0;
}

int gdpt_denoise_nlm_guided_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const GdptNlmParams *params, const GdptNlmGuide *guide, double *d_out, double *d_var_out, void *stream,
                                   GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_guided_device";
        const GdptNlmParams p = check_arguments(who, width, height, d_img, d_var, params, d_out, d_var_out);
        const GdptNlmGuide g = check_guided_arguments(who, d_feat, d_feat_var, guide, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_guided_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, g, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_guided(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                            const GdptNlmParams *params, const GdptNlmGuide *guide, double *out, double *var_out, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_guided";
        const GdptNlmParams p = check_arguments(who, width, height, img, var, params, out, var_out);
        const GdptNlmGuide g = check_guided_arguments(who, feat, feat_var, guide, out, var_out);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, g.num_groups > 0 ? (size_t)width * height * g.num_channels : 0, out, var_out);
        gdpt::denoise_nlm_guided_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, p, g, m.out.d, m.var_out.d, nullptr, stats);
        m.down(out, var_out);
    });
}

void gdpt_nlm_default_demod(GdptNlmDemod *d) {
    if (!d) return;
    *d = GdptNlmDemod{};
    d->albedo_channel = 0; d->coverage_channel = GDPT_FEATURE_CHANNELS - 1; d->floor = 1e-3;
}

int gdpt_denoise_nlm_demod_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                  int num_channels, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *d_out,
                                  double *d_var_out, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_demod_device";
        const GdptNlmParams p = check_arguments(who, width, height, d_img, d_var, params, d_out, d_var_out);
        const GdptNlmDemod d = check_demod_arguments(who, d_feat, d_feat_var, num_channels, guide, demod, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_demod_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, guide, d, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_demod(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int num_channels,
                           const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *out, double *var_out,
                           GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_demod";
        const GdptNlmParams p = check_arguments(who, width, height, img, var, params, out, var_out);
        const GdptNlmDemod d = check_demod_arguments(who, feat, feat_var, num_channels, guide, demod, out, var_out);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, (size_t)width * height * num_channels, out, var_out);
        gdpt::denoise_nlm_demod_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, p, guide, d, m.out.d, m.var_out.d, nullptr, stats);
        m.down(out, var_out);
    });
}

int gdpt_denoise_nlm(int width, int height, const double *img, const double *var, const GdptNlmParams *params, double *out, double *var_out,
                     GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm";
        const GdptNlmParams p = check_arguments(who, width, height, img, var, params, out, var_out);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, nullptr, nullptr, 0, out, var_out);
        gdpt::denoise_nlm_launch(width, height, m.img.d, m.var.d, p, m.out.d, m.var_out.d, nullptr, stats);
        m.down(out, var_out);
    });
}

} // extern "C"
