// nlm_collab.hip — the collaborative form of the first-order feature regression, for gfx950 (include/gdpt.h: gdpt_denoise_nlm_collab*,
// where the definition stands; Bitterli et al. 2016, section 4.3 "collaborative filtering").
//
// Two passes with a coefficient film between them: 3 d channel-planar planes of W H doubles, plane c d + j holding beta_c,j.
//   collab_fit_*      the first sweep of the regression kernels (nlm_regress.hip) and the LDL^T solve of the three right-hand sides: the
//                     same nlm::Stage::sweep, Fit::add and Ldlt, so plane c d + 0 is gdpt_denoise_nlm_regress's out channel c bit for bit.
//                     There is no second sweep; the thread stores its 3 d coefficients.
//   collab_gather_*   every valid q averages the fits of the valid p = q + t, |t|_inf <= r, at its own regressor values, under the
//                     weight the fit centred at p gave its partner q: w_{-t}(p). Neither distance is symmetric in its variances, so
//                     the pair distances are taken with p's triple first and the feature distance with p in the centre's place.
// Each in two forms chosen by the test knob nlm_direct (include/gdpt_debug.h), built as the regression's: 16 x 16 tiles, a thread on
// a pixel, the nlm grid rule of image_kernels.h, block partials through leave_block_sum for finish_kernel. The tiled gather runs the
// stage's sweep (nlm::Stage, nlm_device.h) with the roles of an offset's two pixels swapped; p's feature values and its coefficients come from global
// memory (the film does not fit LDS: 24 doubles on 36 x 36 pixels are 249 KB), q's own features and regressors stay in registers. Every
// loop over unknowns runs to the cap d = 8 with static indices. A gather, never a scatter: every sum comes out in one order.
// No pass writes a plane it reads: the fit reads the inputs and writes the coefficient film, the gather reads both and writes out.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_regress.h"
#include "nlm_regress_device.h"
#include "nlm_collab.h"
#include "nlm_host.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

namespace nlmc {

using namespace nlmr;             // nlm_regress_device.h; and nlm's, film's helpers through it

struct Args {
    nlmr::Args a;                // the regression's block: out is the gather's output, var_out null, `second` unused
    double *coef;                // the coefficient film: 3 d planes of a.gd.plane doubles
    int d;                       // 1 + a.rg.m
};

// the ridge, the factorisation and the three solutions of a pixel's equations: fit.b[c] leaves as beta_c
__device__ __forceinline__ void solve_fit(Fit &fit, double ridge) {
    const double W = fit.A[0];
#pragma unroll
    for (int j = 1; j < kD; j++) fit.A[tri(j, j)] += ridge * W;
    Ldlt ld;
    ld.factor(fit.A);
#pragma unroll
    for (int c = 0; c < 3; c++) ld.solve(fit.b[c]);
}

// pixel ip's planes of the coefficient film
__device__ __forceinline__ void store_fit(const Args &k, size_t ip, const Fit &fit) {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < kD; j++)
            if (j < k.d) k.coef[(size_t)(c * k.d + j) * k.a.gd.plane + ip] = fit.b[c][j];
}
// ... of an invalid pixel: its input bits and zeros, which nobody reads
__device__ __forceinline__ void store_input(const Args &k, size_t ip, const double u[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < kD; j++)
            if (j < k.d) k.coef[(size_t)(c * k.d + j) * k.a.gd.plane + ip] = j == 0 ? u[c] : 0.0;
}

// D^f of the pair whose centre is the valid pixel ip and whose partner is the thread's own pixel: OwnFeatures::distance with the
// roles swapped, operand for operand
__device__ __forceinline__ double distance_from(const Guide &gd, const OwnFeatures &own, size_t ip) {
    double Df = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxGroups; j++) {
        if (j >= gd.groups) continue;
        double phi = 0.0;
#pragma unroll
        for (int c = 0; c < kMaxChannels; c++) {
            if (c < gd.first[j] || c >= gd.first[j] + gd.count[j]) continue;
            const double gp = gd.feat[c * gd.plane + ip], sp = gd.fvar[c * gd.plane + ip];
            const double d = gp - own.g[c];
            phi += (d * d - gd.alpha_f * (sp + fmin(own.s[c], sp))) / (gd.kf2 * fmax(gd.tau[j], sp + own.s[c]));
        }
        Df = fmax(Df, phi / (double)gd.count[j]);
    }
    return Df;
}

// a pixel's gathered sums
struct Gather {
    double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
    // the fit of the valid pixel ip, read at the thread's own regressor values, under the weight w
    __device__ __forceinline__ void add(const Args &k, const OwnRegressors &reg, size_t ip, double w) {
        const Regress &rg = k.a.rg;
        const Guide &gd = k.a.gd;
        double z[kD];
        z[0] = 1.0;
#pragma unroll
        for (int j = 0; j < kMaxM; j++) {
            z[j + 1] = 0.0;
            if (j < rg.m) {
                const double d = reg.g[j] - gd.feat[rg.ch[j] * gd.plane + ip];
                z[j + 1] = rg.scale[j] == 1.0 ? d : d / rg.scale[j];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double y = k.coef[(size_t)(c * k.d) * gd.plane + ip];
#pragma unroll
            for (int j = 1; j < kD; j++)
                if (j < k.d) y += k.coef[(size_t)(c * k.d + j) * gd.plane + ip] * z[j];
            num[c] += w * y;
        }
        den += w;
    }
};

// the gathered pixel's output and its terms of the film sums; u, v: its valid input triples
__device__ __forceinline__ void finish_pixel(const Args &k, size_t i, const double u[3], const double v[3], const Gather &ga, Sums &s) {
    double o[3];
    const double vo[3] = {0.0, 0.0, 0.0};               // (no variance is estimated: the sum stays 0)
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = ga.num[c] / ga.den;
        k.a.out[i + c] = o[c];
    }
    add_sums(s, u, v, o, vo);
}

__global__ __launch_bounds__(kBlock) void collab_fit_direct_kernel(Args k) {
    const nlmr::Args &a = k.a;
    const int r = a.r;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_pixel(a, x, y, u, v); };
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t ip = (size_t)y * a.g.w + x;
        double u[3], v[3];
        if (!load_pixel(a, x, y, u, v)) { store_input(k, ip, u); continue; }
        OwnFeatures own;
        OwnRegressors reg;
        own.load(a.gd, ip);
        reg.load(a.rg, a.gd, ip);
        Fit fit;
        fit.clear();
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
                fit.add(w, z, uq);
            }
        solve_fit(fit, a.rg.ridge);
        store_fit(k, ip, fit);
    }
}

__global__ __launch_bounds__(kBlock) void collab_gather_direct_kernel(Args k) {
    __shared__ double red[kBlock / 64];
    const nlmr::Args &a = k.a;
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
        Gather ga;
        for (int ty = -r; ty <= r; ty++)
            for (int tx = -r; tx <= r; tx++) {
                const int px = x + tx, py = y + ty;
                if (px < 0 || py < 0 || px >= a.g.w || py >= a.g.h) continue;
                double up[3], vp[3];
                if (!load_pixel(a, px, py, up, vp)) continue;
                double S;
                int C;
                patch_distance(a, load, px, py, -tx, -ty, S, C);     // the fit centred at p, its offset o = -t
                const size_t ip = (size_t)py * a.g.w + px;
                ga.add(k, reg, ip, pair_weight(S, C, distance_from(a.gd, own, ip)));
            }
        finish_pixel(k, i, u, v, ga, s);
    }
    leave_partials(a, s, red);
}

__global__ __launch_bounds__(kBlock) void collab_fit_tiled_kernel(Args k) {
    extern __shared__ double lds[];
    const nlmr::Args &a = k.a;
    Stage st;
    st.lay_out(a.r, a.f, lds);
    const int pc = st.pc;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_pixel(a, x, y, u, v); };
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage has been read
        st.fill(a.g, tp.x0, tp.y0, load);
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const bool okp = inside && st.sflag[pc] != 0;
        const size_t ip = (size_t)y * a.g.w + x;
        OwnFeatures own;
        OwnRegressors reg;
        if (okp) { own.load(a.gd, ip); reg.load(a.rg, a.gd, ip); }
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
        if (!inside) continue;
        if (okp) {
            solve_fit(fit, a.rg.ridge);
            store_fit(k, ip, fit);
        } else {
            double u[3], v[3];
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            store_input(k, ip, u);
        }
    }
}

__global__ __launch_bounds__(kBlock) void collab_gather_tiled_kernel(Args k) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    const nlmr::Args &a = k.a;
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
        const bool okq = inside && st.sflag[pc] != 0;
        OwnFeatures own;
        OwnRegressors reg;
        if (okq) { own.load(a.gd, (size_t)y * a.g.w + x); reg.load(a.rg, a.gd, (size_t)y * a.g.w + x); }
        Gather ga;
        // the thread's pixel is the partner q of every fit centred at a valid p = q + t: S and C of p's offset -t
        st.sweep<true>(a.k2, a.alpha, a.eps, okq, [&](int, double S, int C, int ty, int tx) {
            const size_t gp = (size_t)(y + ty) * a.g.w + (x + tx);
            ga.add(k, reg, gp, pair_weight(S, C, distance_from(a.gd, own, gp)));
        });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (okq) {
            st.mean(pc, u); st.variance(pc, v);
            finish_pixel(k, i, u, v, ga, s);
        } else {
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlmc

namespace gdpt {

namespace {

// the sums' ([1]'s sum var out is not estimated), and the coefficient film of a call that brings none, grown on demand
struct CollabWorkspace : SumsWorkspace {
    DeviceBuffer<double> coef;
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<CollabWorkspace> &g_workspaces = *new PerStream<CollabWorkspace>();

} // namespace

void denoise_nlm_collab_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               const GdptNlmParams &p, const GdptNlmGuide &g, const GdptNlmRegress &rg, double *d_out, double *d_coef,
                               hipStream_t stream, GdptNlmStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    CollabWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    ws.prepare("nlm collab");
    const int d = 1 + rg.num_regressors;
    if (!d_coef) {
        ws.coef.grow((size_t)3 * d * w * h, stream, "hipMalloc(nlm collab coefficients)");
        d_coef = ws.coef;
    }

    nlmc::Args k{};
    nlmr::Args &a = k.a;
    fill_base(a, w, h, p, d_img, d_var, d_out, nullptr, ws.partials);
    a.second = 0;
    fill_guide(a.gd, g, d_feat, d_feat_var, (size_t)w * h);
    fill_regress(a.rg, a.gd, rg);
    k.coef = d_coef; k.d = d;
    const int nb = a.g.blocks;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    const int pass = debug_knob_int("nlm_collab_pass", 0);      // measurements: 1 the fit alone, 2 the gather alone
    const bool fit = pass != 2, gather = pass != 1;
    if (debug_knob("nlm_direct", 0) != 0) {
        if (fit) hipLaunchKernelGGL(nlmc::collab_fit_direct_kernel, dim3(nb), dim3(film::kBlock), 0, stream, k);
        if (gather) hipLaunchKernelGGL(nlmc::collab_gather_direct_kernel, dim3(nb), dim3(film::kBlock), 0, stream, k);
    } else {
        if (fit) launch_staged(nlmc::collab_fit_tiled_kernel, nb, a.r, a.f, stream, k, "hipFuncSetAttribute(nlm collab stage)");
        if (gather) launch_staged(nlmc::collab_gather_tiled_kernel, nb, a.r, a.f, stream, k, "hipFuncSetAttribute(nlm collab stage)");
    }
    ck(hipGetLastError(), "nlm collab launch");
    if (!stats) return;
    if (!gather) ck(hipMemsetAsync(ws.partials, 0, 6 * film::kMaxBlocks * sizeof(double), stream), "hipMemsetAsync(nlm collab partials)");      // (no sums)
    ws.read_stats(nb, stream, "nlm collab", stats);
    stats->sum_var_out = stats->error_out = std::numeric_limits<double>::quiet_NaN();      // not estimated
    stats->window_radius = p.window_radius; stats->patch_radius = p.patch_radius;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// whether [a, a + na) and [b, b + nb) doubles share an address; a null range shares none
bool overlap(const double *a, size_t na, const double *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(double), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(double);
    return a0 < b1 && b0 < a1;
}

// The blocks in force of a call, every argument checked: what the regression's entry points refuse, and a coefficient film that
// overlaps an input or out. `who` names the caller.
gdpt::NlmRegressBlocks check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                       const double *feat_var, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress,
                                       const double *out, const double *coef) {
    const gdpt::NlmRegressBlocks b = gdpt::nlm_regress_check_arguments(who, width, height, img, var, feat, feat_var, params, guide, regress, out, nullptr);
    const size_t px = (size_t)width * height, nc = 3 * (size_t)(1 + b.rg.num_regressors) * px, nf = b.feature_elems(width, height);
    if (overlap(coef, nc, img, 3 * px) || overlap(coef, nc, var, 3 * px) || overlap(coef, nc, out, 3 * px) || overlap(coef, nc, feat, nf) ||
        overlap(coef, nc, feat_var, nf))
        throw std::runtime_error(who + ": coef must not overlap an input or out");
    return b;
}

} // namespace

extern "C" {

int gdpt_denoise_nlm_collab_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *d_out,
                                   double *d_coef, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_collab_device";
        const gdpt::NlmRegressBlocks b = check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, params, guide, regress, d_out, d_coef);
        need_a_device(who);
        gdpt::denoise_nlm_collab_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_coef, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_collab(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                            const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *out, double *coef,
                            GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_collab";
        const gdpt::NlmRegressBlocks b = check_arguments(who, width, height, img, var, feat, feat_var, params, guide, regress, out, coef);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, b.feature_elems(width, height), out, nullptr);
        const size_t celems = m.elems * (size_t)(1 + b.rg.num_regressors);
        gdpt::Mirror m_coef;
        m_coef.make(coef, celems);
        gdpt::denoise_nlm_collab_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, b.p, b.g, b.rg, m.out.d, m_coef.d, nullptr, stats);
        m.down(out, nullptr);
        m_coef.down(coef, celems);
    });
}

} // extern "C"
