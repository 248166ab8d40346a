// denoise_nlm.hip — non-local means with variance-cancelling patch distances on (mean, variance of the mean), for gfx950
// (include/gdpt.h: gdpt_denoise_nlm*, where the definition stands; Rousselle, Knaus, Zwicker 2012, sections 4-5).
//
// Kernels: two forms of the one definition, chosen by the test knob nlm_direct (include/gdpt_debug.h). Both loop over 16 x 16 tiles
// as box_kernel (recon_spread.hip) does, a thread on a pixel of the tile, and both leave block partials through leave_block_sum for
// finish_kernel (image_kernels.h): a fixed order, the same bits every time.
//   direct_kernel   the literal definition: the loops over the window offsets o and the patch taps n read global memory, every
//                   pair distance e_o(p + n) is computed where it is used, (2r+1)^2 (2f+1)^2 of them per pixel.
//   tiled_kernel    the tile with a halo of r + f pixels staged in LDS, plane by plane (three u, three v, a validity flag; out-of-film
//                   and invalid entries are u = v = 0, flag 0), sized by the call's r and f: (16 + 2(r+f))^2 entries of 52 bytes,
//                   42 x 42 = 91.7 KB at r = 10, f = 3. Per window offset: e_o and its count on the (16 + 2f)^2 points the tile's
//                   patches touch, into LDS; row sums of 2f + 1 taps; column sums of the row sums (the separable box of box_kernel);
//                   exp, and the three numerators, the weight sum and the three w^2 v sums accumulate in registers. (16 + 2f)^2
//                   pair distances per offset and tile instead of 256 (2f+1)^2: 484 against 12544 at f = 3.
//                   LDS banking: every plane is a plane of doubles or of ints, so consecutive lanes read consecutive elements. In the
//                   row pass a half-wave covers two rows of 16 outputs; the e plane's pitch is 16 (f = 0) or 48 doubles, = 16 mod 32,
//                   which puts the second row's 16 doubles on the other half of the 64 banks. In the column pass a half-wave reads 32
//                   consecutive doubles of the row sums (pitch 16).
// Both are templates on GUIDED (gdpt_denoise_nlm_guided*): the unguided instantiations are the kernels above as they were, argument
// block included. A guided kernel adds the feature planes to a pixel's validity and caps the colour weight of a pair (p, p+o) with the
// pair's feature distance. The thread keeps its own pixel's feature values and variances in registers (the loops over groups and
// channels are unrolled to the caps, so every index is static) and reads those of p+o from global memory: the planes are planar, a
// wave's read of one plane is four 128-byte rows, served from L1 / L2. The stage gets no feature planes: at (r, f) = (10, 3) it
// already takes 108 624 of the 163 840 bytes a workgroup may declare, and 2 x 6 planes of (16 + 2r)^2 doubles would be another 124 KB.
// And on DEMOD (gdpt_denoise_nlm_demod*): the four DEMOD = false instantiations are the kernels above as they were, argument blocks
// included. A demodulated kernel filters u / a~, v / a~^2 for the effective albedo a~ of include/gdpt.h: load_pixel adds the albedo and
// coverage planes to a pixel's validity and divides, so the tiled kernel's stage holds the quotients and needs no LDS of its own;
// finish_pixel multiplies a~ back. A thread recomputes its own a~ from the planar planes there, and reloads its own original triples
// for the colour-domain sums: (u / a~) a~ is not always u.
// The device helpers of all of them (the guide's and the divisor's blocks, load_pixel, pair_distance, OwnFeatures, the LDS sizing, the
// sums, and a pixel's weighted sums: Accum, finish_pixel) are in nlm_device.h, which nlm_regress.hip and nlm_joint.hip share.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>
#include <vector>

namespace nlm {

struct Args {
    static constexpr bool kGuided = false, kDemod = false;
    TileGrid g;                  // 16 x 16 tiles
    int r, f;
    double k2, alpha, eps;
    const double *img, *var;
    double *out, *var_out;       // var_out nullable
    double *partials;            // [0] sum var in, [1] sum u^2 in, [2] pixels left out, [3] sum var out, [4] sum u^2 out, [5] = [2]; gridDim.x doubles each
};

struct GuidedArgs : Args {
    static constexpr bool kGuided = true;
    Guide gd;
};
struct DemodArgs : Args {
    static constexpr bool kDemod = true;
    Demod dm;
};
struct GuidedDemodArgs : GuidedArgs {
    static constexpr bool kDemod = true;
    Demod dm;
};
template <bool GUIDED, bool DEMOD>
using ArgsOf = typename std::conditional<GUIDED, typename std::conditional<DEMOD, GuidedDemodArgs, GuidedArgs>::type,
                                         typename std::conditional<DEMOD, DemodArgs, Args>::type>::type;

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void direct_kernel(ArgsOf<GUIDED, DEMOD> a) {
    __shared__ double red[kBlock / 64];
    const int r = a.r, f = a.f;
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
                double S = 0.0;
                int C = 0;
                for (int ny = -f; ny <= f; ny++)
                    for (int nx = -f; nx <= f; nx++) {
                        const int ax = x + nx, ay = y + ny, bx = ax + ox, by = ay + oy;
                        if (ax < 0 || ay < 0 || ax >= a.g.w || ay >= a.g.h || bx < 0 || by < 0 || bx >= a.g.w || by >= a.g.h) continue;
                        double ua[3], va[3], ub[3], vb[3];
                        const bool oka = load_pixel(a, ax, ay, ua, va), okb = load_pixel(a, bx, by, ub, vb);
                        if (!oka || !okb) continue;
                        S += pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
                        C++;
                    }
                if constexpr (GUIDED) acc.template add<true>(S, C, uq, vq, own.distance(a.gd, (size_t)qy * a.g.w + qx));
                else acc.add(S, C, uq, vq);      // (C >= 1: the tap n = 0 counts)
            }
        finish_pixel(a, i, u, v, acc, s);
    }
    leave_partials(a, s, red);
}

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void tiled_kernel(ArgsOf<GUIDED, DEMOD> a) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    const int r = a.r, f = a.f, halo = r + f;
    const int sw = kTile + 2 * halo, sn = sw * sw;      // the stage: the tile and its halo
    const int ew = kTile + 2 * f, en = ew * ew;         // the points the tile's patches touch
    const int ep = e_pitch(f), taps = 2 * f + 1;
    double *const su = lds, *const sv = lds + 3 * sn;   // plane c at su + c sn, sv + c sn
    double *const pe = lds + 6 * sn;                    // e_o of the current offset, pitch ep
    double *const ph = pe + ep * ew;                    // its row sums, pitch 16
    int *const sflag = (int *)(ph + kTile * ew);
    int *const ce = sflag + sn, *const ch = ce + ep * ew;
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
    // the (at most two) pair distances and row sums of an offset that fall to this thread
    int ia[2], ie[2], jrow[2];
    for (int k = 0; k < 2; k++) {
        const int q = tid + k * kBlock;
        const int qy = q / ew, qx = q - qy * ew;
        ia[k] = q < en ? (qy + r) * sw + qx + r : -1;
        ie[k] = qy * ep + qx;
        jrow[k] = q < kTile * ew ? (q / kTile) * ep + (q & (kTile - 1)) : -1;
    }
    const int pc = (ly + halo) * sw + lx + halo;        // the thread's own pixel in the stage
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
            sflag[k] = ok ? 1 : 0;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const bool okp = inside && sflag[pc] != 0;
        OwnFeatures own;
        if constexpr (GUIDED) { if (okp) own.load(a.gd, (size_t)y * a.g.w + x); }
        Accum acc;
        for (int oy = -r; oy <= r; oy++)
            for (int ox = -r; ox <= r; ox++) {
                const int shift = oy * sw + ox;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (ia[k] < 0) continue;
                    const int i0 = ia[k], i1 = i0 + shift;
                    const int both = sflag[i0] & sflag[i1];
                    double e = 0.0;
                    if (both) {
                        double ua[3], va[3], ub[3], vb[3];
#pragma unroll
                        for (int c = 0; c < 3; c++) { ua[c] = su[c * sn + i0]; va[c] = sv[c * sn + i0]; ub[c] = su[c * sn + i1]; vb[c] = sv[c * sn + i1]; }
                        e = pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
                    }
                    pe[ie[k]] = e; ce[ie[k]] = both;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (jrow[k] < 0) continue;
                    double S = 0.0;
                    int C = 0;
                    for (int n = 0; n < taps; n++) { S += pe[jrow[k] + n]; C += ce[jrow[k] + n]; }
                    ph[tid + k * kBlock] = S; ch[tid + k * kBlock] = C;
                }
                __syncthreads();
                const int iq = pc + shift;
                if (okp && sflag[iq] != 0) {
                    double S = 0.0;
                    int C = 0;
                    for (int n = 0; n < taps; n++) { S += ph[tid + n * kTile]; C += ch[tid + n * kTile]; }
                    const double uq[3] = {su[iq], su[sn + iq], su[2 * sn + iq]}, vq[3] = {sv[iq], sv[sn + iq], sv[2 * sn + iq]};
                    if constexpr (GUIDED) acc.template add<true>(S, C, uq, vq, own.distance(a.gd, (size_t)(y + oy) * a.g.w + (x + ox)));
                    else acc.add(S, C, uq, vq);
                }
            }
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        if (okp) {
            const double u[3] = {su[pc], su[sn + pc], su[2 * sn + pc]}, v[3] = {sv[pc], sv[sn + pc], sv[2 * sn + pc]};
            finish_pixel(a, i, u, v, acc, s);
        } else {
            double u[3], v[3];
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlm

namespace gdpt {

namespace {

struct NlmWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;
    DeviceBuffer<film::Estimate> d_est;     // [0] sum var in, sum u^2 in, left out; [1] sum var out, sum u^2 out, left out
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
};

// leaked on purpose: no HIP call is made from a static destructor (as the solver's registry, poisson_kernels.hip); a pair's entry
// goes with forget_stream (device_mem.h)
PerStream<NlmWorkspace> &g_workspaces = *new PerStream<NlmWorkspace>();

// one form of one instantiation, enqueued on `stream`
template <bool GUIDED, bool DEMOD>
void launch_form(const nlm::ArgsOf<GUIDED, DEMOD> &a, bool direct, hipStream_t stream) {
    const int nb = a.g.blocks;
    if (direct) {
        hipLaunchKernelGGL((nlm::direct_kernel<GUIDED, DEMOD>), dim3(nb), dim3(film::kBlock), 0, stream, a);
        return;
    }
    const size_t lds = (size_t)nlm::lds_doubles(a.r, a.f) * sizeof(double) + (size_t)nlm::lds_ints(a.r, a.f) * sizeof(int);
    ck(hipFuncSetAttribute(reinterpret_cast<const void *>(nlm::tiled_kernel<GUIDED, DEMOD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
       "hipFuncSetAttribute(nlm stage)");
    hipLaunchKernelGGL((nlm::tiled_kernel<GUIDED, DEMOD>), dim3(nb), dim3(film::kBlock), lds, stream, a);
}

// Device pointers on the current device; the arguments have been checked. Enqueued on `stream`; waits for it if `stats` is asked for.
// `guide` (nullable): the guided kernels, on `d_feat`, `d_feat_var`. `demod` (nullable): the demodulated kernels, on the same planes.
void denoise_nlm_launch(int w, int h, const double *d_img, const double *d_var, const GdptNlmParams &p, double *d_out, double *d_var_out,
                        hipStream_t stream, GdptNlmStats *stats, const GdptNlmGuide *guide = nullptr, const double *d_feat = nullptr,
                        const double *d_feat_var = nullptr, const GdptNlmDemod *demod = nullptr) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    NlmWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    if (!ws.partials) ws.partials.alloc(6 * film::kMaxBlocks, "hipMalloc(nlm partials)");
    if (!ws.d_est) ws.d_est.alloc(2, "hipMalloc(nlm sums)");
    if (!ws.h_est) ws.h_est.alloc(2, "hipHostMalloc(nlm sums)");
    for (auto &e : ws.ev) if (!e) e.create();

    nlm::GuidedArgs a{};
    a.g = film::tile_grid(w, h, kNlmTile, kNlmTile); a.r = p.window_radius; a.f = p.patch_radius;
    a.k2 = p.k * p.k; a.alpha = p.alpha; a.eps = p.epsilon;
    a.img = d_img; a.var = d_var; a.out = d_out; a.var_out = d_var_out; a.partials = ws.partials;
    const int nb = a.g.blocks;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    if (guide) {
        nlm::Guide &gd = a.gd;
        gd.feat = d_feat; gd.fvar = d_feat_var; gd.plane = (size_t)w * h;
        gd.groups = guide->num_groups; gd.kf2 = guide->k_f * guide->k_f; gd.alpha_f = guide->alpha_f;
        for (int j = 0; j < guide->num_groups; j++) {
            const GdptNlmFeatureGroup &grp = guide->groups[j];
            gd.first[j] = grp.first_channel; gd.count[j] = grp.num_channels; gd.tau[j] = grp.tau;
            for (int c = grp.first_channel; c < grp.first_channel + grp.num_channels; c++) gd.used |= 1u << c;
        }
    }
    const nlm::Args &plain = a;       // (the unguided kernels take the argument block they always took)
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
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    film::launch_finish(nb, ws.partials.data() + 3 * nb, ws.d_est.data() + 1, stream);
    ck(hipGetLastError(), "nlm reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, 2 * sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(nlm sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm)");
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

// what both entry points refuse; `who` names the caller. Returns the parameters in force.
GdptNlmParams check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const GdptNlmParams *params,
                              const double *out, const double *var_out) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (out == img || out == var) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && (var_out == img || var_out == var || var_out == out)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
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

void need_a_device(const std::string &who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }      // (without a device the count itself is an error)
    if (ndev <= 0) throw std::runtime_error(who + ": no HIP device visible (this library has no CPU fallback)");
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
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        const size_t felems = g.num_groups > 0 ? (size_t)width * height * g.num_channels : 0, fbytes = felems * sizeof(double);
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
        gdpt::denoise_nlm_guided_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, g, d_out, d_var_out, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (var_out) ck(hipMemcpy(var_out, d_var_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
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
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        const size_t felems = (size_t)width * height * num_channels, fbytes = felems * sizeof(double);
        gdpt::DeviceBuffer<double> d_img, d_var, d_out, d_var_out, d_feat, d_feat_var;
        d_img.alloc(elems, "hipMalloc(nlm io)"); d_var.alloc(elems, "hipMalloc(nlm io)"); d_out.alloc(elems, "hipMalloc(nlm io)");
        if (var_out) d_var_out.alloc(elems, "hipMalloc(nlm io)");
        d_feat.alloc(felems, "hipMalloc(nlm features)"); d_feat_var.alloc(felems, "hipMalloc(nlm features)");
        ck(hipMemcpy(d_img, img, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_feat, feat, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_feat_var, feat_var, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        gdpt::denoise_nlm_demod_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, guide, d, d_out, d_var_out, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (var_out) ck(hipMemcpy(var_out, d_var_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

int gdpt_denoise_nlm(int width, int height, const double *img, const double *var, const GdptNlmParams *params, double *out, double *var_out,
                     GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm";
        const GdptNlmParams p = check_arguments(who, width, height, img, var, params, out, var_out);
        need_a_device(who);
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        gdpt::DeviceBuffer<double> d_img, d_var, d_out, d_var_out;
        d_img.alloc(elems, "hipMalloc(nlm io)"); d_var.alloc(elems, "hipMalloc(nlm io)"); d_out.alloc(elems, "hipMalloc(nlm io)");
        if (var_out) d_var_out.alloc(elems, "hipMalloc(nlm io)");
        ck(hipMemcpy(d_img, img, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        gdpt::denoise_nlm_launch(width, height, d_img, d_var, p, d_out, d_var_out, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (var_out) ck(hipMemcpy(var_out, d_var_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
