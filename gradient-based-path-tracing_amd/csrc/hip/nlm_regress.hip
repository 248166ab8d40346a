// nlm_regress.hip — a first-order feature regression on the non-local-means weights, for gfx950 (include/gdpt.h:
// gdpt_denoise_nlm_regress*, where the definition stands; Bitterli et al. 2016, section 4, on the weights of Rousselle, Manzi, Zwicker 2013).
//
// Kernels: two forms of the one definition, chosen by the test knob nlm_direct (include/gdpt_debug.h), beside those of denoise_nlm.hip
// and built as they are: 16 x 16 tiles, a thread on a pixel of the tile, block partials through leave_block_sum for finish_kernel
// (image_kernels.h), the same bits every time.
//   regress_direct_kernel   the literal definition: every pair distance is computed where it is used, from global memory.
//   regress_tiled_kernel    tiled_kernel<true, false> of denoise_nlm.hip with the fit in the place of the weighted mean: the same LDS
//                           stage (the tile with a halo of r + f pixels, three u, three v and a validity flag), the same separable box
//                           and the same two barriers per window offset.
// Both run the loop over the window offsets twice. The first sweep accumulates the normal equations of the thread's pixel; the
// thread then solves them (LDL^T in the header's order); the second sweep recomputes every weight and accumulates
// (w_o q^T z(p, o))^2 v(p+o), which needs the q that only the solve gives. The stage is still in LDS for it; no weight is stored per
// pixel (at 512 x 512 and r = 10 that would be 925 MB). The second sweep is left out when neither var_out nor the sums are asked for.
// Registers: the thread keeps the lower triangle of A (36 doubles at d = 8) and the three b (24 doubles) in registers. Every loop over
// unknowns is unrolled to the cap d = 8 so that every index is static; an unused regressor has z = 0, which leaves a row of A that is
// zero but for its diagonal ridge W: its L entries are 0 and the arithmetic of the other unknowns is what it would be without it.
// profiles/nlm_kernel_resources.txt has what the compiler makes of it.
// The device helpers (pair_distance, load_pixel, OwnFeatures, valid_features, the LDS sizing and the sums) are those of denoise_nlm.hip's
// kernels, in nlm_device.h: a regression kernel is a guided, not demodulated kernel to them, whose guide's `used` mask also names the
// regressors' planes. What the collaborative form (nlm_collab.hip) shares with these kernels, the argument block, the fit, the LDL^T and
// the stage with its sweep, is in nlm_regress_device.h.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_regress.h"
#include "nlm_regress_device.h"

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
    s.var_in += (v[0] + v[1]) + v[2];
    s.sq_in += (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    s.var_out += (vo[0] + vo[1]) + vo[2];
    s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
}

__global__ __launch_bounds__(kBlock) void regress_direct_kernel(Args a) {
    __shared__ double red[kBlock / 64];
    const int r = a.r;
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
                    patch_distance(a, x, y, ox, oy, S, C);      // (C >= 1: the tap n = 0 counts)
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
    st.r = a.r; st.f = a.f;
    const int halo = a.r + a.f;
    st.sw = kTile + 2 * halo; st.sn = st.sw * st.sw;       // the stage: the tile and its halo
    st.ew = kTile + 2 * a.f;                               // the points the tile's patches touch, a row
    const int en = st.ew * st.ew;
    st.ep = e_pitch(a.f); st.taps = 2 * a.f + 1;
    st.su = lds; st.sv = lds + 3 * st.sn;                  // plane c at su + c sn, sv + c sn
    st.pe = lds + 6 * st.sn;                               // e_o of the current offset, pitch ep
    st.ph = st.pe + st.ep * st.ew;                         // its row sums, pitch 16
    st.sflag = (int *)(st.ph + kTile * st.ew);
    st.ce = st.sflag + st.sn; st.ch = st.ce + st.ep * st.ew;
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
    st.tid = tid;
    // the (at most two) pair distances and row sums of an offset that fall to this thread
    for (int k = 0; k < 2; k++) {
        const int q = tid + k * kBlock;
        const int qy = q / st.ew, qx = q - qy * st.ew;
        st.ia[k] = q < en ? (qy + a.r) * st.sw + qx + a.r : -1;
        st.ie[k] = qy * st.ep + qx;
        st.jrow[k] = q < kTile * st.ew ? (q / kTile) * st.ep + (q & (kTile - 1)) : -1;
    }
    st.pc = (ly + halo) * st.sw + lx + halo;               // the thread's own pixel in the stage
    const int sn = st.sn, sw = st.sw, pc = st.pc;
    double *const su = st.su, *const sv = st.sv;
    Sums s;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int x0 = tp.x0, y0 = tp.y0;
        __syncthreads();                                // the previous tile's stage has been read
        for (int k = tid; k < sn; k += kBlock) {
            const int ry = k / sw, rx = k - ry * sw;
            const int gx = x0 - halo + rx, gy = y0 - halo + ry;
            double u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
            bool ok = false;
            if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) ok = load_pixel(a, gx, gy, u, v);
#pragma unroll
            for (int c = 0; c < 3; c++) { su[c * sn + k] = ok ? u[c] : 0.0; sv[c * sn + k] = ok ? v[c] : 0.0; }
            st.sflag[k] = ok ? 1 : 0;
        }
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
            st.sweep(a, okp, [&](int iq, double S, int C, int oy, int ox) {
                const size_t gq = (size_t)(y + oy) * a.g.w + (x + ox);
                const double w = pair_weight(S, C, own.distance(a.gd, gq));
                const double uq[3] = {su[iq], su[sn + iq], su[2 * sn + iq]};
                double z[kD];
                reg.design(a.rg, a.gd, gq, z);
                fit.add(w, z, uq);
            });
            if (okp) solve_fit(fit, a.rg.ridge, o, q);
        }
        if (a.second)
            st.sweep(a, okp, [&](int iq, double S, int C, int oy, int ox) {
                const size_t gq = (size_t)(y + oy) * a.g.w + (x + ox);
                const double w = pair_weight(S, C, own.distance(a.gd, gq));
                const double vq[3] = {sv[iq], sv[sn + iq], sv[2 * sn + iq]};
                double z[kD];
                reg.design(a.rg, a.gd, gq, z);
                add_variance(w, q, z, vq, vo);
            });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        if (okp) {
            const double u[3] = {su[pc], su[sn + pc], su[2 * sn + pc]}, v[3] = {sv[pc], sv[sn + pc], sv[2 * sn + pc]};
            finish_pixel(a, i, u, v, o, vo, s);
        } else {
            double u[3], v[3];
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlmr

namespace gdpt {

namespace {

struct RegressWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;
    DeviceBuffer<film::Estimate> d_est;     // [0] sum var in, sum u^2 in, left out; [1] sum var out, sum u^2 out, left out
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<RegressWorkspace> &g_workspaces = *new PerStream<RegressWorkspace>();

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
    RegressWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    if (!ws.partials) ws.partials.alloc(6 * film::kMaxBlocks, "hipMalloc(nlm regress partials)");
    if (!ws.d_est) ws.d_est.alloc(2, "hipMalloc(nlm regress sums)");
    if (!ws.h_est) ws.h_est.alloc(2, "hipHostMalloc(nlm regress sums)");
    for (auto &e : ws.ev) if (!e) e.create();

    nlmr::Args a{};
    a.g = film::tile_grid(w, h, kNlmTile, kNlmTile); a.r = p.window_radius; a.f = p.patch_radius;
    a.k2 = p.k * p.k; a.alpha = p.alpha; a.eps = p.epsilon;
    a.img = d_img; a.var = d_var; a.out = d_out; a.var_out = d_var_out; a.partials = ws.partials;
    a.second = (d_var_out || stats) ? 1 : 0;
    nlm::Guide &gd = a.gd;
    gd.feat = d_feat; gd.fvar = d_feat_var; gd.plane = (size_t)w * h;
    gd.groups = g.num_groups; gd.kf2 = g.k_f * g.k_f; gd.alpha_f = g.alpha_f;
    for (int j = 0; j < g.num_groups; j++) {
        const GdptNlmFeatureGroup &grp = g.groups[j];
        gd.first[j] = grp.first_channel; gd.count[j] = grp.num_channels; gd.tau[j] = grp.tau;
        for (int c = grp.first_channel; c < grp.first_channel + grp.num_channels; c++) gd.used |= 1u << c;
    }
    a.rg.m = rg.num_regressors; a.rg.ridge = rg.ridge;
    for (int j = 0; j < nlmr::kMaxM; j++) { a.rg.ch[j] = 0; a.rg.scale[j] = 1.0; }
    for (int j = 0; j < rg.num_regressors; j++) { a.rg.ch[j] = rg.channel[j]; a.rg.scale[j] = rg.scale[j]; gd.used |= 1u << rg.channel[j]; }
    const int nb = a.g.blocks;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    if (debug_knob("nlm_direct", 0) != 0) {
        hipLaunchKernelGGL(nlmr::regress_direct_kernel, dim3(nb), dim3(film::kBlock), 0, stream, a);
    } else {
        const size_t lds = (size_t)nlm::lds_doubles(a.r, a.f) * sizeof(double) + (size_t)nlm::lds_ints(a.r, a.f) * sizeof(int);
        ck(hipFuncSetAttribute(reinterpret_cast<const void *>(nlmr::regress_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "hipFuncSetAttribute(nlm regress stage)");
        hipLaunchKernelGGL(nlmr::regress_tiled_kernel, dim3(nb), dim3(film::kBlock), lds, stream, a);
    }
    ck(hipGetLastError(), "nlm regress launch");
    if (!stats) return;
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    film::launch_finish(nb, ws.partials.data() + 3 * nb, ws.d_est.data() + 1, stream);
    ck(hipGetLastError(), "nlm regress reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, 2 * sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(nlm regress sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm regress)");
    *stats = GdptNlmStats{};
    const film::Estimate &in = ws.h_est.data()[0], &out = ws.h_est.data()[1];
    stats->pixels_left_out = (uint64_t)in.left_out;
    stats->sum_var_in = in.sum_var; stats->sum_sq_in = in.sum_mean2;
    stats->sum_var_out = out.sum_var; stats->sum_sq_out = out.sum_mean2;
    stats->error_in = std::sqrt(in.sum_var / in.sum_mean2);
    stats->error_out = std::sqrt(out.sum_var / out.sum_mean2);
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->filter_ms = ms; }
    stats->window_radius = p.window_radius; stats->patch_radius = p.patch_radius;
}

} // namespace gdpt

namespace {

using gdpt::ck;

// The blocks in force of a call, every argument checked: what the guided entry points refuse (the films, params, the guide, an output
// aliasing an input) and what the regression block adds. `who` names the caller.
struct Blocks { GdptNlmParams p; GdptNlmGuide g; GdptNlmRegress rg; };
Blocks check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                       const double *feat_var, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress,
                       const double *out, const double *var_out) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (out == img || out == var) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && (var_out == img || var_out == var || var_out == out)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    Blocks b;
    if (params) b.p = *params; else gdpt_nlm_default_params(&b.p);
    gdpt::nlm_check_params(who, b.p);
    if (guide) b.g = *guide; else gdpt_nlm_default_guide(&b.g);
    gdpt::nlm_check_guide(who, b.g);
    if (regress) b.rg = *regress; else gdpt_nlm_default_regress(&b.rg);
    gdpt::nlm_check_regress(who, b.rg, b.g.num_channels);
    if (b.g.num_groups > 0 || b.rg.num_regressors > 0) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    if (feat && (out == feat || out == feat_var)) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && feat && (var_out == feat || var_out == feat_var)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    return b;
}

void need_a_device(const std::string &who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }      // (without a device the count itself is an error)
    if (ndev <= 0) throw std::runtime_error(who + ": no HIP device visible (this library has no CPU fallback)");
}

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
        const Blocks b = check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, params, guide, regress, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_regress_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_regress(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                             const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *out, double *var_out,
                             GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_regress";
        const Blocks b = check_arguments(who, width, height, img, var, feat, feat_var, params, guide, regress, out, var_out);
        need_a_device(who);
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        const bool planes = b.g.num_groups > 0 || b.rg.num_regressors > 0;
        const size_t felems = planes ? (size_t)width * height * b.g.num_channels : 0, fbytes = felems * sizeof(double);
        gdpt::DeviceBuffer<double> d_img, d_var, d_out, d_var_out, d_feat, d_feat_var;
        d_img.alloc(elems, "hipMalloc(nlm io)"); d_var.alloc(elems, "hipMalloc(nlm io)"); d_out.alloc(elems, "hipMalloc(nlm io)");
        if (var_out) d_var_out.alloc(elems, "hipMalloc(nlm io)");
        d_feat.alloc(felems, "hipMalloc(nlm features)"); d_feat_var.alloc(felems, "hipMalloc(nlm features)");
        ck(hipMemcpy(d_img, img, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        if (felems) {
            ck(hipMemcpy(d_feat, feat, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            ck(hipMemcpy(d_feat_var, feat_var, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        }
        gdpt::denoise_nlm_regress_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_var_out, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (var_out) ck(hipMemcpy(var_out, d_var_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
