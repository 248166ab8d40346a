// nlm_regress.hip — a first-order feature regression on the non-local-means weights, for gfx950 (include/gdpt.h:
// gdpt_denoise_nlm_regress*, where the definition stands; Bitterli et al. 2016, section 4, on the weights of Rousselle, Manzi, Zwicker 2013).
//
// Kernels: two forms of the one definition, chosen by the test knob nlm_direct (include/gdpt_debug.h), beside those of denoise_nlm.hip
// and built as they are: 16 x 16 tiles, a thread on a pixel of the tile, block partials through leave_block_sum for finish_kernel
// (image_kernels.h), the same bits every time.
//   regress_direct_kernel   the literal definition: every pair distance is computed where it is used, from global memory.
//   regress_tiled_kernel    tiled_kernel<true, false> of denoise_nlm.hip with the fit in the place of the weighted mean, on the same
//                           stage (nlm::Stage, nlm_device.h).
// Both run the loop over the window offsets twice. The first sweep accumulates the normal equations of the thread's pixel; the
// thread then solves them (LDL^T in the header's order); the second sweep recomputes every weight and accumulates
// (w_o q^T z(p, o))^2 v(p+o), which needs the q that only the solve gives. The stage is still in LDS for it; no weight is stored per
// pixel (at 512 x 512 and r = 10 that would be 925 MB). The second sweep is left out when neither var_out nor the sums are asked for.
// Registers: the thread keeps the lower triangle of A (36 doubles at d = 8) and the three b (24 doubles) in registers. Every loop over
// unknowns is unrolled to the cap d = 8 so that every index is static; an unused regressor has z = 0, which leaves a row of A that is
// zero but for its diagonal ridge W: its L entries are 0 and the arithmetic of the other unknowns is what it would be without it.
// profiles/nlm_kernel_resources.txt has what the compiler makes of it.
// A regression kernel is a guided, not demodulated kernel to the helpers of nlm_device.h, whose guide's `used` mask also names the
// regressors' planes. What the collaborative form (nlm_collab.hip) shares with these kernels alone is in nlm_regress_device.h.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_regress.h"
#include "nlm_regress_device.h"
#include "nlm_host.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

namespace nlmr {

using namespace nlm;              // nlm_device.h; and film's kBlock, TileGrid, leave_block_sum through it

// beta_c[0] and q of the pixel's equations (which the call leaves with their ridge added)
__device__ __forceinline__ void solve_fit(Fit &fit, double ridge, double o[3], double q[kD]) {
    const double W = fit.A[0];
#pragma unroll
    for (int j = 1; j < kD; j++) fit.A[tri(j, j)] += ridge * W;
    Ldlt ld;
    ld.factor(fit.A);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        ld.solve(fit.b[c]);
        o[c] = fit.b[c][0];
    }
#pragma unroll
    for (int i = 0; i < kD; i++) q[i] = i == 0 ? 1.0 : 0.0;
    ld.solve(q);
}

// a tap's term of var_out
__device__ __forceinline__ void add_variance(double w, const double q[kD], const double z[kD], const double v[3], double vo[3]) {
    double l = q[0];
#pragma unroll
    for (int j = 1; j < kD; j++) l += q[j] * z[j];
    const double t = w * l;
#pragma unroll
    for (int c = 0; c < 3; c++) vo[c] += (t * t) * v[c];
}

// the pixel's outputs and its terms of the film sums; u, v: its valid input triples
__device__ __forceinline__ void finish_pixel(const Args &a, size_t i, const double u[3], const double v[3], const double o[3], const double vo[3],
                                             Sums &s) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.out[i + c] = o[c];
        if (a.var_out) a.var_out[i + c] = vo[c];
    }
    add_sums(s, u, v, o, vo);
}

__global__ __launch_bounds__(kBlock) void regress_direct_kernel(Args a) {
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
        OwnRegressors reg;
        own.load(a.gd, (size_t)y * a.g.w + x);
        reg.load(a.rg, a.gd, (size_t)y * a.g.w + x);
        double o[3], q[kD], vo[3] = {0.0, 0.0, 0.0};
        for (int sweep = 0; sweep < (a.second ? 2 : 1); sweep++) {
            Fit fit;
            if (sweep == 0) fit.clear();
            for (int oy = -r; oy <= r; oy++)
                for (int ox = -r; ox <= r; ox++) {
                    const int qx = x + ox, qy = y + oy;
                    if (qx < 0 || qy < 0 || qx >= a.g.w || qy >= a.g.h) continue;
                    double uq[3], vq[3];
                    if (!load_pixel(a, qx, qy, uq, vq)) continue;
                    double S;
                    int C;
                    patch_distance(a, load, x, y, ox, oy, S, C);      // (C >= 1: the tap n = 0 counts)
                    const size_t iq = (size_t)qy * a.g.w + qx;
                    const double w = pair_weight(S, C, own.distance(a.gd, iq));
                    double z[kD];
                    reg.design(a.rg, a.gd, iq, z);
                    if (sweep == 0) fit.add(w, z, uq);
                    else add_variance(w, q, z, vq, vo);
                }
            if (sweep == 0) solve_fit(fit, a.rg.ridge, o, q);
        }
        finish_pixel(a, i, u, v, o, vo, s);
    }
    leave_partials(a, s, red);
}

__global__ __launch_bounds__(kBlock) void regress_tiled_kernel(Args a) {
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
        OwnRegressors reg;
        if (okp) { own.load(a.gd, (size_t)y * a.g.w + x); reg.load(a.rg, a.gd, (size_t)y * a.g.w + x); }
        double o[3] = {0.0, 0.0, 0.0}, q[kD], vo[3] = {0.0, 0.0, 0.0};
        {
            Fit fit;
            fit.clear();
            st.sweep(a.k2, a.alpha, a.eps, okp, [&](int iq, double S, int C, int oy, int ox) {
                const size_t gq = (size_t)(y + oy) * a.g.w + (x + ox);
                const double w = pair_weight(S, C, own.distance(a.gd, gq));
                double uq[3], z[kD];
                st.mean(iq, uq);
                reg.design(a.rg, a.gd, gq, z);
                fit.add(w, z, uq);
            });
            if (okp) solve_fit(fit, a.rg.ridge, o, q);
        }
        if (a.second)
            st.sweep(a.k2, a.alpha, a.eps, okp, [&](int iq, double S, int C, int oy, int ox) {
                const size_t gq = (size_t)(y + oy) * a.g.w + (x + ox);
                const double w = pair_weight(S, C, own.distance(a.gd, gq));
                double vq[3], z[kD];
                st.variance(iq, vq);
                reg.design(a.rg, a.gd, gq, z);
                add_variance(w, q, z, vq, vo);
            });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (okp) {
            st.mean(pc, u); st.variance(pc, v);
            finish_pixel(a, i, u, v, o, vo, s);
        } else {
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlmr

namespace gdpt {

namespace {

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<SumsWorkspace> &g_workspaces = *new PerStream<SumsWorkspace>();

} // namespace

void nlm_check_regress(const std::string &who, const GdptNlmRegress &r, int num_channels) {
    if (r.num_regressors < 0 || r.num_regressors > nlmr::kMaxM)
        throw std::runtime_error(who + ": num_regressors must be in [0, " + std::to_string(nlmr::kMaxM) + "]");
    for (int j = 0; j < r.num_regressors; j++) {
        const std::string at = who + ": regress channel[" + std::to_string(j) + "]";
        if (r.channel[j] < 0 || r.channel[j] >= num_channels) throw std::runtime_error(at + " must be in [0, num_channels)");
        for (int k = 0; k < j; k++)
            if (r.channel[k] == r.channel[j]) throw std::runtime_error(at + " is listed twice");
        if (!std::isfinite(r.scale[j]) || !(r.scale[j] > 0))
            throw std::runtime_error(who + ": regress scale[" + std::to_string(j) + "] must be finite and > 0");
    }
    if (!std::isfinite(r.ridge) || !(r.ridge > 0)) throw std::runtime_error(who + ": ridge must be finite and > 0");
    if (r.reserved[0] != 0 || r.reserved[1] != 0) throw std::runtime_error(who + ": regress reserved must be 0");
}

void denoise_nlm_regress_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                const GdptNlmParams &p, const GdptNlmGuide &g, const GdptNlmRegress &rg, double *d_out, double *d_var_out,
                                hipStream_t stream, GdptNlmStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    SumsWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    ws.prepare("nlm regress");

    nlmr::Args a{};
    fill_base(a, w, h, p, d_img, d_var, d_out, d_var_out, ws.partials);
    a.second = (d_var_out || stats) ? 1 : 0;
    fill_guide(a.gd, g, d_feat, d_feat_var, (size_t)w * h);
    fill_regress(a.rg, a.gd, rg);
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    if (debug_knob("nlm_direct", 0) != 0) hipLaunchKernelGGL(nlmr::regress_direct_kernel, dim3(a.g.blocks), dim3(film::kBlock), 0, stream, a);
    else launch_staged(nlmr::regress_tiled_kernel, a.g.blocks, a.r, a.f, stream, a, "hipFuncSetAttribute(nlm regress stage)");
    ck(hipGetLastError(), "nlm regress launch");
    if (!stats) return;
    ws.read_stats(a.g.blocks, stream, "nlm regress", stats);
    stats->window_radius = p.window_radius; stats->patch_radius = p.patch_radius;
}

// The blocks in force of a call, every argument checked: what the guided entry points refuse (the films, params, the guide, an output
// aliasing an input) and what the regression block adds. `who` names the caller.
NlmRegressBlocks nlm_regress_check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                             const double *feat_var, const GdptNlmParams *params, const GdptNlmGuide *guide,
                                             const GdptNlmRegress *regress, const double *out, const double *var_out) {
    check_film(who, width, height, img, var, out, var_out);
    NlmRegressBlocks b;
    if (params) b.p = *params; else gdpt_nlm_default_params(&b.p);
    nlm_check_params(who, b.p);
    if (guide) b.g = *guide; else gdpt_nlm_default_guide(&b.g);
    nlm_check_guide(who, b.g);
    if (regress) b.rg = *regress; else gdpt_nlm_default_regress(&b.rg);
    nlm_check_regress(who, b.rg, b.g.num_channels);
    if (b.planes()) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    if (feat && (out == feat || out == feat_var)) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && feat && (var_out == feat || var_out == feat_var)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    return b;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

} // namespace

extern "C" {

void gdpt_nlm_default_regress(GdptNlmRegress *r) {
    if (!r) return;
    *r = GdptNlmRegress{};
    r->num_regressors = 6;
    for (int j = 0; j < 6; j++) { r->channel[j] = j; r->scale[j] = 1.0; }      // albedo, shading normal
    r->ridge = 1e-2;
}

int gdpt_denoise_nlm_regress_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                    const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *d_out,
                                    double *d_var_out, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_regress_device";
        const gdpt::NlmRegressBlocks b = gdpt::nlm_regress_check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, params, guide, regress, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_regress_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_regress(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                             const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *out, double *var_out,
                             GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_regress";
        const gdpt::NlmRegressBlocks b = gdpt::nlm_regress_check_arguments(who, width, height, img, var, feat, feat_var, params, guide, regress, out, var_out);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, b.feature_elems(width, height), out, var_out);
        gdpt::denoise_nlm_regress_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, b.p, b.g, b.rg, m.out.d, m.var_out.d, nullptr, stats);
        m.down(out, var_out);
    });
}

} // extern "C"
