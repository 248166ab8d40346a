// progressive.hip — progressive rendering for gfx950: a session that renders a scene in passes over disjoint sample windows of
// one stream block, folds every pass into running means and sums of weighted squared deviations, and reports per-pixel
// variances and an error estimate (include/gdpt.h: gdpt_progressive_*).
//
// Definition. Pass k is a mean m over its n samples, per buffer component. West's weighted update (1979):
//     W += n;  d = m - mean;  mean += (n / W) d;  M2 += n d (m - mean_new)
// gives mean = sum n_k m_k / sum n_k and M2 = sum n_k (m_k - mean)^2 after any number of passes of any sizes, and
// E[M2] = (K - 1) sigma^2 for per-sample variance sigma^2: var_mean = M2 / ((K - 1) W) estimates the variance of the running
// mean. The error estimate is sqrt(sum var_mean(img) / sum mean(img)^2) over the pixels whose img mean and M2 are finite.
//
// Kernels. A thread owns a PIXEL: its three channels in every buffer (the film is interleaved, [(y*W+x)*3+c], so consecutive
// threads read consecutive 24-byte triples and a wave covers 1536 contiguous bytes per plane).
//   fold_kernel      one pass over the film for all buffers: reads pass, mean, M2, writes mean, M2 (the first pass reads no
//                    mean / M2: they start at 0), and leaves the block partials of the two sums and of the left-out count.
//   finish_kernel    (image_kernels.hip) one block: the partials reduced in a fixed order (xor tree in a wave, waves in index order,
//                    blocks strided in index order), so that the same session gives the same bits and the same stopping pass.
//   variance_kernel  read-out: M2 / ((K-1) W) per buffer and the variances of the assembled cx, cy.
//   merge_kernel     the fold's sibling for two sessions: dst takes in src's (mean, M2) by the pairwise update below.
// The fold is memory bound: 5 doubles of traffic per component (3 read, 2 written), 40 bytes x 15 components per GradPath pixel.
//
// Slices and merges. A session draws its passes from a slice [first, first + own) of the block of `block` streams; sessions over
// disjoint slices hold disjoint samples of the whole film, and their statistics combine exactly (Chan, Golub, LeVeque 1979):
//     W = Wa + Wb;  d = mean_b - mean_a;  mean = mean_a + (Wb / W) d;  M2 = (M2a + M2b) + d d (Wa Wb / W);  K = Ka + Kb
// is the state of one session that folded all the passes of both. The merge is 6 doubles of traffic per component (4 read, 2 written).
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "poisson_kernels.h"
#include "progressive_internal.h"
#include "denoise_nlm.h"
#include "nlm_regress.h"
#include "nlm_collab.h"
#include "denoise_atrous.h"
#include "variance_smooth.h"
#include "nlm_pyramid.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

namespace prg {

using namespace film;             // kBlock, kMaxBlocks, leave_block_sum

struct Planes {
    const double *pass[5];
    double *mean[5], *m2[5];
};

// n: samples of the pass; w_new: samples so far, this pass included; norm = (K - 1) w_new, K passes this one included (0 while K < 2:
// no estimate). FIRST: the running planes are not read (mean = M2 = 0 before the first pass).
// partials: [0] sum var_mean(img), [1] sum mean(img)^2, [2] pixels left out; gridDim.x doubles each.
template <int NBUF, bool FIRST>
__global__ __launch_bounds__(kBlock) void fold_kernel(Planes p, int npix, double n, double w_new, double norm, double *partials) {
    __shared__ double red[kBlock / 64];
    const double f = n / w_new;
    double s_var = 0, s_m2 = 0, s_out = 0;
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < npix; pix += gridDim.x * kBlock) {
        const size_t i = (size_t)3 * pix;
#pragma unroll
        for (int b = 0; b < NBUF; b++) {
            double mu[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double m = p.pass[b][i + c];
                const double mu0 = FIRST ? 0.0 : p.mean[b][i + c], q0 = FIRST ? 0.0 : p.m2[b][i + c];
                const double d = m - mu0;
                mu[c] = mu0 + f * d;
                q[c] = q0 + n * d * (m - mu[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; c++) { p.mean[b][i + c] = mu[c]; p.m2[b][i + c] = q[c]; }
            if (b == 0 && norm > 0.0) {
                const bool ok = isfinite(mu[0]) && isfinite(mu[1]) && isfinite(mu[2]) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
                if (ok) {
                    s_var += (q[0] / norm + q[1] / norm) + q[2] / norm;
                    s_m2 += (mu[0] * mu[0] + mu[1] * mu[1]) + mu[2] * mu[2];
                } else s_out += 1.0;
            }
        }
    }
    leave_block_sum(partials, 0, s_var, red);
    leave_block_sum(partials, 1, s_m2, red);
    leave_block_sum(partials, 2, s_out, red);
}

// dst (mean, m2) takes in src (smean, sm2): f = Wb / W, g = Wa Wb / W for dst's Wa, src's Wb, W = Wa + Wb; norm = (K - 1) W of the
// merged state (0 while K < 2). FIRST: dst holds nothing (Wa = 0) and its planes are not read: src's are copied, bit for bit.
// partials as in fold_kernel.
struct MergePlanes {
    const double *smean[5], *sm2[5];
    double *mean[5], *m2[5];
};
template <int NBUF, bool FIRST>
__global__ __launch_bounds__(kBlock) void merge_kernel(MergePlanes p, int npix, double f, double g, double norm, double *partials) {
    __shared__ double red[kBlock / 64];
    double s_var = 0, s_m2 = 0, s_out = 0;
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < npix; pix += gridDim.x * kBlock) {
        const size_t i = (size_t)3 * pix;
#pragma unroll
        for (int b = 0; b < NBUF; b++) {
            double mu[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double mb = p.smean[b][i + c], qb = p.sm2[b][i + c];
                if (FIRST) { mu[c] = mb; q[c] = qb; }
                else {
                    const double ma = p.mean[b][i + c], qa = p.m2[b][i + c];
                    const double d = mb - ma;
                    mu[c] = ma + f * d;
                    q[c] = (qa + qb) + (d * d) * g;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) { p.mean[b][i + c] = mu[c]; p.m2[b][i + c] = q[c]; }
            if (b == 0 && norm > 0.0) {
                const bool ok = isfinite(mu[0]) && isfinite(mu[1]) && isfinite(mu[2]) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
                if (ok) {
                    s_var += (q[0] / norm + q[1] / norm) + q[2] / norm;
                    s_m2 += (mu[0] * mu[0] + mu[1] * mu[1]) + mu[2] * mu[2];
                } else s_out += 1.0;
            }
        }
    }
    leave_block_sum(partials, 0, s_var, red);
    leave_block_sum(partials, 1, s_m2, red);
    leave_block_sum(partials, 2, s_out, red);
}

// var[b] = M2[b] / norm for b < NBUF; NBUF == 5: vcx(x,y) = var cx0(x,y) + var cx1(x-1,y), vcy(x,y) = var cy0(x,y) + var cy1(x,y-1),
// the second term absent on the film's first column / row (as gdpt_assemble_device assembles cx, cy).
struct VarPlanes { const double *m2[5]; double *var[5], *vcx, *vcy; };
template <int NBUF>
__global__ __launch_bounds__(kBlock) void variance_kernel(VarPlanes p, int w, int h, double norm) {
    const int n3 = 3 * w * h, row = 3 * w;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n3; i += gridDim.x * kBlock) {
#pragma unroll
        for (int b = 0; b < NBUF; b++) p.var[b][i] = p.m2[b][i] / norm;
        if (NBUF == 5) {
            const int y = i / row, x = (i - y * row) / 3;
            const double vx = p.m2[1][i] / norm, vy = p.m2[2][i] / norm;
            p.vcx[i] = x == 0 ? vx : vx + p.m2[3][i - 3] / norm;
            p.vcy[i] = y == 0 ? vy : vy + p.m2[4][i - row] / norm;
        }
    }
}

} // namespace prg

namespace {

using gdpt::ck;

void add_totals(GdptRenderStats &t, const GdptRenderStats &rs) {
    t.samples += rs.samples; t.rays += rs.rays; t.bounces += rs.bounces;
    t.nodes_visited += rs.nodes_visited; t.tris_tested += rs.tris_tested; t.nonfinite_samples += rs.nonfinite_samples;
    t.render_ms += rs.render_ms; t.node_bytes = rs.node_bytes;
    t.wave_node_trips += rs.wave_node_trips; t.wave_leaf_trips += rs.wave_leaf_trips;
    t.wave_steps += rs.wave_steps; t.lane_steps += rs.lane_steps;
}

// the reduction of the partials a fold or merge launch left, the estimate to the host, the launches' device time; waits for the stream
void finish_estimate(GdptProgressive &s, int nb, const char *what) {
    film::launch_finish(nb, s.partials, s.d_est, s.stream);
    ck(hipGetLastError(), what);
    ck(hipEventRecord(s.ev[1], s.stream), "hipEventRecord");
    ck(hipMemcpyAsync(s.h_est, s.d_est, sizeof(film::Estimate), hipMemcpyDeviceToHost, s.stream), "hipMemcpyAsync(estimate)");
    ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(fold)");
    s.est = *s.h_est;
    { float ms = 0; ck(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]), "hipEventElapsedTime"); s.fold_ms = ms; }
}

// every interval of the block whose samples the session holds: its own [first, first + own_done) and the merged ones
std::vector<std::pair<int, int>> intervals_held(const GdptProgressive &s) {
    std::vector<std::pair<int, int>> v = s.merged_intervals;
    if (s.own_done > 0) v.push_back({s.first, s.first + s.own_done});
    return v;
}

} // namespace

namespace prg {

double error_estimate(const GdptProgressive &s) {
    if (s.passes < 2) return std::numeric_limits<double>::quiet_NaN();
    return std::sqrt(s.est.sum_var / s.est.sum_mean2);
}

void fill_status(const GdptProgressive &s, GdptProgressiveStatus *st) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->passes = s.passes; st->spp_done = s.done; st->budget_spp = s.own + s.merged; st->stop_reason = s.stop_reason;
    st->error_estimate = error_estimate(s);
    st->pixels_left_out = s.passes < 2 ? 0 : (uint64_t)s.est.left_out;
    st->fold_ms = s.fold_ms;
    st->totals = s.totals;
}

void add_pass(GdptProgressive &s, int spp, GdptRenderStats *stats) {
    if (spp <= 0) throw std::runtime_error("gdpt_progressive_add_pass: spp must be > 0");
    if ((long long)s.own_done + spp > (long long)s.own)
        throw std::runtime_error("gdpt_progressive_add_pass: the pass exceeds the session's budget (" + std::to_string(s.own_done) + " + " + std::to_string(spp) +
                                 " > " + std::to_string(s.own) + " samples per pixel)");
    ck(hipSetDevice(s.scene->device), "hipSetDevice");
    GdptRenderParams p{};
    p.spp = spp; p.rng_scheme = GDPT_RNG_SAMPLE; p.shift_mode = s.shift; p.max_depth_override = s.max_depth_override;
    const GdptSampleWindow win{s.block, s.first + s.own_done};
    GdptRenderStats rs{};
    const int rc = s.mode == GDPT_PROGRESSIVE_PATH
                       ? gdpt_path_render_window_device(s.scene, &p, &win, s.pass[0], s.stream, &rs)
                       : gdpt_render_window_device(s.scene, &p, &win, s.pass[0], s.pass[1], s.pass[2], s.pass[3], s.pass[4], s.stream, &rs);
    if (rc != 0) throw std::runtime_error(gdpt_last_error());

    prg::Planes pl{};
    for (int k = 0; k < s.nbuf; k++) { pl.pass[k] = s.pass[k]; pl.mean[k] = s.mean[k]; pl.m2[k] = s.m2[k]; }
    const int npix = s.w * s.h, nb = film::stride_grid((size_t)npix, film::kMaxBlocks, 1).blocks, K = s.passes + 1;
    const double n = (double)spp, w_new = (double)(s.done + spp), norm = (double)(K - 1) * w_new;
    const dim3 grid(nb), block(film::kBlock);
    const bool first = s.passes == 0;
    ck(hipEventRecord(s.ev[0], s.stream), "hipEventRecord");
    if (s.nbuf == 5) {
        if (first) hipLaunchKernelGGL((prg::fold_kernel<5, true>), grid, block, 0, s.stream, pl, npix, n, w_new, norm, s.partials);
        else hipLaunchKernelGGL((prg::fold_kernel<5, false>), grid, block, 0, s.stream, pl, npix, n, w_new, norm, s.partials);
    } else {
        if (first) hipLaunchKernelGGL((prg::fold_kernel<1, true>), grid, block, 0, s.stream, pl, npix, n, w_new, norm, s.partials);
        else hipLaunchKernelGGL((prg::fold_kernel<1, false>), grid, block, 0, s.stream, pl, npix, n, w_new, norm, s.partials);
    }
    finish_estimate(s, nb, "progressive fold launch");
    s.done += spp; s.own_done += spp; s.passes = K;
    add_totals(s.totals, rs);
    if (stats) *stats = rs;
}

void merge(GdptProgressive &dst, const GdptProgressive &src) {
    if (&dst == &src) throw std::runtime_error("gdpt_progressive_merge: dst and src are the same session");
    if (dst.w != src.w || dst.h != src.h) throw std::runtime_error("gdpt_progressive_merge: the sessions' films differ");
    if (dst.mode != src.mode) throw std::runtime_error("gdpt_progressive_merge: the sessions' modes differ (GradPath / Integrator::Path)");
    if (dst.shift != src.shift) throw std::runtime_error("gdpt_progressive_merge: the sessions' shift modes differ");
    if (dst.max_depth_override != src.max_depth_override) throw std::runtime_error("gdpt_progressive_merge: the sessions' max_depth_override differ");
    if (dst.block != src.block) throw std::runtime_error("gdpt_progressive_merge: the sessions' stream blocks differ (" + std::to_string(dst.block) + ", " + std::to_string(src.block) + ")");
    // what dst holds, and what its own passes may still draw: src must bring none of it
    std::vector<std::pair<int, int>> mine = dst.merged_intervals;
    if (dst.own > 0) mine.push_back({dst.first, dst.first + dst.own});
    const std::vector<std::pair<int, int>> theirs = intervals_held(src);
    for (const auto &a : theirs)
        for (const auto &b : mine)
            if (a.first < b.second && b.first < a.second)
                throw std::runtime_error("gdpt_progressive_merge: src holds samples [" + std::to_string(a.first) + ", " + std::to_string(a.second) +
                                         ") of the block, which overlap [" + std::to_string(b.first) + ", " + std::to_string(b.second) + ") of dst");
    if (src.passes == 0) return;
    if ((long long)dst.done + src.done > (long long)std::numeric_limits<int>::max() || (long long)dst.passes + src.passes > (long long)std::numeric_limits<int>::max())
        throw std::runtime_error("gdpt_progressive_merge: sample or pass count overflow");
    ck(hipSetDevice(dst.device), "hipSetDevice");
    prg::MergePlanes pl{};
    if (src.device != dst.device) {          // src's planes into staging planes on dst's device, on dst's stream
        int can = 0;
        ck(hipDeviceCanAccessPeer(&can, dst.device, src.device), "hipDeviceCanAccessPeer");
        if (can) {                           // (without peer access the runtime stages the copy through the host)
            const hipError_t e = hipDeviceEnablePeerAccess(src.device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ck(e, "hipDeviceEnablePeerAccess");
            (void)hipGetLastError();
        }
        for (int k = 0; k < 2 * dst.nbuf; k++) if (!dst.stage[k]) dst.stage[k].alloc(dst.elems, "hipMalloc(progressive staging)");
        for (int k = 0; k < dst.nbuf; k++) {
            ck(hipMemcpyPeerAsync(dst.stage[2 * k], dst.device, src.mean[k], src.device, dst.elems * sizeof(double), dst.stream), "hipMemcpyPeerAsync(mean)");
            ck(hipMemcpyPeerAsync(dst.stage[2 * k + 1], dst.device, src.m2[k], src.device, dst.elems * sizeof(double), dst.stream), "hipMemcpyPeerAsync(M2)");
            pl.smean[k] = dst.stage[2 * k]; pl.sm2[k] = dst.stage[2 * k + 1];
        }
    } else
        for (int k = 0; k < dst.nbuf; k++) { pl.smean[k] = src.mean[k]; pl.sm2[k] = src.m2[k]; }
    for (int k = 0; k < dst.nbuf; k++) { pl.mean[k] = dst.mean[k]; pl.m2[k] = dst.m2[k]; }
    const int npix = dst.w * dst.h, nb = film::stride_grid((size_t)npix, film::kMaxBlocks, 1).blocks, K = dst.passes + src.passes;
    const double wa = (double)dst.done, wb = (double)src.done, w = wa + wb;
    const double f = wb / w, g = wa * wb / w, norm = (double)(K - 1) * w;
    const dim3 grid(nb), block(film::kBlock);
    const bool first = dst.passes == 0;
    ck(hipEventRecord(dst.ev[0], dst.stream), "hipEventRecord");
    if (dst.nbuf == 5) {
        if (first) hipLaunchKernelGGL((prg::merge_kernel<5, true>), grid, block, 0, dst.stream, pl, npix, f, g, norm, dst.partials);
        else hipLaunchKernelGGL((prg::merge_kernel<5, false>), grid, block, 0, dst.stream, pl, npix, f, g, norm, dst.partials);
    } else {
        if (first) hipLaunchKernelGGL((prg::merge_kernel<1, true>), grid, block, 0, dst.stream, pl, npix, f, g, norm, dst.partials);
        else hipLaunchKernelGGL((prg::merge_kernel<1, false>), grid, block, 0, dst.stream, pl, npix, f, g, norm, dst.partials);
    }
    finish_estimate(dst, nb, "progressive merge launch");
    dst.done += src.done; dst.merged += src.done; dst.passes = K;
    dst.merged_intervals.insert(dst.merged_intervals.end(), theirs.begin(), theirs.end());
    add_totals(dst.totals, src.totals);
}

void reset(GdptProgressive &s) {
    s.own_done = 0; s.merged = 0; s.done = 0; s.passes = 0; s.stop_reason = GDPT_STOP_NONE;
    s.merged_intervals.clear();
    s.est = film::Estimate{}; s.fold_ms = 0; s.totals = GdptRenderStats{};
}

} // namespace prg

namespace {

using prg::error_estimate;
using prg::fill_status;

void copy_out(const GdptProgressive &s, double *dst, const double *src, int on_device) {
    if (!dst) return;
    ck(hipMemcpyAsync(dst, src, s.elems * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s.stream), "hipMemcpyAsync(progressive read)");
}

// the read-out planes s.var[0..4] and, for a GradPath session, the assembled s.var[5], s.var[6]; enqueued on the session's stream
void compute_variances(GdptProgressive &s) {
    const int nvar = s.nbuf == 5 ? 7 : 1;
    for (int k = 0; k < nvar; k++) if (!s.var[k]) s.var[k].alloc(s.elems, "hipMalloc(progressive variances)");
    prg::VarPlanes vp{};
    for (int k = 0; k < s.nbuf; k++) { vp.m2[k] = s.m2[k]; vp.var[k] = s.var[k]; }
    vp.vcx = s.var[5]; vp.vcy = s.var[6];
    const double norm = (double)(s.passes - 1) * (double)s.done;
    const int nb = film::stride_grid(s.elems, 4 * film::kMaxBlocks, 1).blocks;
    if (s.nbuf == 5) hipLaunchKernelGGL(prg::variance_kernel<5>, dim3(nb), dim3(film::kBlock), 0, s.stream, vp, s.w, s.h, norm);
    else hipLaunchKernelGGL(prg::variance_kernel<1>, dim3(nb), dim3(film::kBlock), 0, s.stream, vp, s.w, s.h, norm);
    ck(hipGetLastError(), "progressive variance launch");
}

// c, cx, cy of the running means into s.asm_buf[0..2] (s.asm_buf[3] takes the reconstruction); enqueued on the session's stream
void assemble_means(GdptProgressive &s) {
    for (auto &b : s.asm_buf) if (!b) b.alloc(s.elems, "hipMalloc(progressive assembly)");
    gdpt::launch_assemble(s.w, s.h, 0, 0, s.mean[0], s.mean[1], s.mean[2], s.mean[3], s.mean[4], s.asm_buf[0], s.asm_buf[1], s.asm_buf[2], s.stream);
}

// whole: the slice is the whole block (gdpt_progressive_create); else [first, first + num) of it
void create_session(const char *fn, GdptScene *scene, const GdptProgressiveConfig *config, bool whole, int first, int num, void *stream, GdptProgressive **out) {
    const std::string who(fn);
    if (!scene || !out) throw std::runtime_error(who + ": null argument");
    GdptProgressiveConfig cfg = config ? *config : GdptProgressiveConfig{};
    if (cfg.mode != GDPT_PROGRESSIVE_GRADPATH && cfg.mode != GDPT_PROGRESSIVE_PATH) throw std::runtime_error(who + ": unknown mode");
    if (cfg.shift_mode != GDPT_SHIFT_REFERENCE && cfg.shift_mode != GDPT_SHIFT_RECONNECT) throw std::runtime_error(who + ": unknown shift_mode");
    if (cfg.mode == GDPT_PROGRESSIVE_PATH && scene->view.num_lights <= 0) throw std::runtime_error(who + ": the scene has no emitter to sample");
    const int budget = cfg.budget_spp > 0 ? cfg.budget_spp : scene->scene_spp;
    if (budget <= 0) throw std::runtime_error(who + ": budget_spp must be > 0");
    if (whole) { first = 0; num = budget; }
    if (first < 0 || num < 0 || (long long)first + num > (long long)budget)
        throw std::runtime_error(who + ": the slice [" + std::to_string(first) + ", " + std::to_string((long long)first + num) + ") leaves the block [0, " +
                                 std::to_string(budget) + ")");
    const int w = scene->view.cam.width, h = scene->view.cam.height;
    if ((unsigned long long)w * (unsigned long long)h > (~0ull >> 1) / (unsigned long long)budget)
        throw std::runtime_error(who + ": width * height * budget_spp does not fit 63 bits");
    if ((long long)w * h > (1LL << 29)) throw std::runtime_error(who + ": film too large");
    ck(hipSetDevice(scene->device), "hipSetDevice");
    std::unique_ptr<GdptProgressive> s(new GdptProgressive());
    s->scene = scene; s->device = scene->device; s->stream = (hipStream_t)stream;
    s->mode = cfg.mode; s->shift = cfg.shift_mode; s->max_depth_override = cfg.max_depth_override;
    s->nbuf = cfg.mode == GDPT_PROGRESSIVE_PATH ? 1 : 5;
    s->w = w; s->h = h; s->block = budget; s->first = first; s->own = num; s->elems = (size_t)w * h * 3;
    for (auto *set : {s->pass, s->mean, s->m2}) {
        if (set == s->pass && num == 0) continue;        // an accumulator renders nothing
        for (int k = 0; k < s->nbuf; k++) set[k].alloc(s->elems, "hipMalloc(progressive planes)");
    }
    s->partials.alloc(3 * film::kMaxBlocks, "hipMalloc(progressive partials)");
    s->d_est.alloc(1, "hipMalloc(progressive estimate)");
    s->h_est.alloc(1, "hipHostMalloc(progressive estimate)");
    for (auto &e : s->ev) e.create();
    *out = s.release();
}

} // namespace

namespace prg {

void reconstruct(GdptProgressive &s, double dataCost, const GdptReconParams *recon, GdptReconStats *stats) {
    if (s.nbuf != 5) throw std::runtime_error("gdpt_progressive_reconstruct: an Integrator::Path session has no gradients (read its mean)");
    if (s.passes < 1) throw std::runtime_error("gdpt_progressive_reconstruct: no pass has been added");
    ck(hipSetDevice(s.scene->device), "hipSetDevice");
    assemble_means(s);
    if (gdpt_reconstruct_device(s.w, s.h, s.asm_buf[0], s.asm_buf[1], s.asm_buf[2], dataCost, recon, s.asm_buf[3], s.stream, stats) != 0)
        throw std::runtime_error(gdpt_last_error());
}

void reconstruct_weighted(GdptProgressive &s, double dataCost, const GdptWeightedReconParams *params, double *const confidence[3],
                          GdptWeightedReconStats *stats) {
    if (s.nbuf != 5) throw std::runtime_error("gdpt_progressive_reconstruct_weighted: an Integrator::Path session has no gradients (read its mean)");
    if (s.passes < 2) throw std::runtime_error("gdpt_progressive_reconstruct_weighted: variances need at least 2 passes");
    ck(hipSetDevice(s.scene->device), "hipSetDevice");
    assemble_means(s);
    compute_variances(s);
    // (the confidence planes go straight to their destination: the copy kind is taken from the pointers, host or device)
    if (gdpt_reconstruct_weighted_device(s.w, s.h, s.asm_buf[0], s.asm_buf[1], s.asm_buf[2], s.var[0], s.var[5], s.var[6], dataCost, params, s.asm_buf[3],
                                         confidence, s.stream, stats) != 0)
        throw std::runtime_error(gdpt_last_error());
}

} // namespace prg

// What the filters that read the session's own features share (gdpt_progressive_denoise_guided, gdpt_progressive_denoise_demod; the
// parameter blocks have been checked): the variances of buffer 0, the feature render on the session's stream, `filter(s, d_out,
// d_var_out, stats)` on it, and the copies out. Blocking.
template <class Filter>
static void filter_with_features(const std::string &who, GdptProgressive &s, int feature_spp, int on_device, double *out, double *var_out,
                                 double *features, double *features_var, GdptNlmStats *stats, Filter filter) {
    if (feature_spp < 2 || feature_spp > s.block) throw std::runtime_error(who + ": feature_spp must be in [2, budget_spp]");
    if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
    ck(hipSetDevice(s.scene->device), "hipSetDevice");
    compute_variances(s);
    const size_t felems = (size_t)s.w * s.h * GDPT_FEATURE_CHANNELS;
    for (auto &b : s.feat_buf) if (!b) b.alloc(felems, "hipMalloc(progressive features)");
    // the camera rays of the session's own first samples: the window {budget_spp, 0}, on the session's stream
    GdptRenderParams rp{};
    rp.spp = feature_spp; rp.rng_scheme = GDPT_RNG_SAMPLE;
    const GdptSampleWindow win{s.block, 0};
    if (!s.feat_current) gdpt::features_launch(s.scene, &rp, &win, s.feat_buf[0], s.feat_buf[1], s.stream, nullptr);
    double *d_out = out, *d_var_out = var_out;
    if (!on_device) {                 // through planes of the session's on the way to host memory
        for (int k = 0; k < (var_out ? 2 : 1); k++) if (!s.nlm_buf[k]) s.nlm_buf[k].alloc(s.elems, "hipMalloc(progressive denoise)");
        d_out = s.nlm_buf[0]; d_var_out = var_out ? s.nlm_buf[1].data() : nullptr;
    }
    GdptNlmStats st{};                // (asked for always: the call is blocking)
    filter(s, d_out, d_var_out, &st);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!on_device) { copy_out(s, out, d_out, 0); copy_out(s, var_out, d_var_out, 0); }
    if (features) ck(hipMemcpyAsync(features, s.feat_buf[0], felems * sizeof(double), kind, s.stream), "hipMemcpyAsync(progressive features)");
    if (features_var) ck(hipMemcpyAsync(features_var, s.feat_buf[1], felems * sizeof(double), kind, s.stream), "hipMemcpyAsync(progressive features)");
    ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise)");
    if (stats) *stats = st;
}

extern "C" {

int gdpt_progressive_create(GdptScene *scene, const GdptProgressiveConfig *config, void *stream, GdptProgressive **out) {
    return gdpt::guarded([&]() { create_session("gdpt_progressive_create", scene, config, true, 0, 0, stream, out); });
}

int gdpt_progressive_create_slice(GdptScene *scene, const GdptProgressiveConfig *config, int first_sample, int num_samples, void *stream,
                                  GdptProgressive **out) {
    return gdpt::guarded([&]() { create_session("gdpt_progressive_create_slice", scene, config, false, first_sample, num_samples, stream, out); });
}

int gdpt_progressive_merge(GdptProgressive *dst, const GdptProgressive *src) {
    return gdpt::guarded([&]() {
        if (!dst || !src) throw std::runtime_error("gdpt_progressive_merge: null argument");
        if (dst->group_half) throw std::runtime_error("gdpt_progressive_merge: dst is a half of a group (its group rebuilds it)");
        if (dst->group_total) throw std::runtime_error("gdpt_progressive_merge: dst is the total of a group (its group rebuilds it)");
        prg::merge(*dst, *src);
    });
}

void gdpt_progressive_free(GdptProgressive *session) {
    if (!session) return;
    hipSetDevice(session->device);
    hipStreamSynchronize(session->stream);
    delete session;
}

int gdpt_progressive_add_pass(GdptProgressive *session, int spp, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        if (!session) throw std::runtime_error("gdpt_progressive_add_pass: null session");
        if (session->group_half) throw std::runtime_error("gdpt_progressive_add_pass: the session is a half of a group (it draws no samples of its own)");
        if (session->group_total) throw std::runtime_error("gdpt_progressive_add_pass: the session is the total of a group (it draws no samples of its own)");
        prg::add_pass(*session, spp, stats);
    });
}

int gdpt_progressive_status(const GdptProgressive *session, GdptProgressiveStatus *status) {
    return gdpt::guarded([&]() {
        if (!session || !status) throw std::runtime_error("gdpt_progressive_status: null argument");
        fill_status(*session, status);
    });
}

int gdpt_progressive_read(GdptProgressive *session, int on_device, double *const means[5], double *const vars[5], double *const assembled_vars[3]) {
    return gdpt::guarded([&]() {
        if (!session) throw std::runtime_error("gdpt_progressive_read: null session");
        GdptProgressive &s = *session;
        if (s.passes < 1) throw std::runtime_error("gdpt_progressive_read: no pass has been added");
        bool want_var = false;
        for (int k = 0; k < 5; k++) {
            if (k >= s.nbuf && ((means && means[k]) || (vars && vars[k]))) throw std::runtime_error("gdpt_progressive_read: an Integrator::Path session has the img plane only");
            if (vars && vars[k]) want_var = true;
        }
        for (int k = 0; k < 3; k++) if (assembled_vars && assembled_vars[k]) {
            if (s.nbuf != 5) throw std::runtime_error("gdpt_progressive_read: assembled variances need a GradPath session");
            want_var = true;
        }
        if (want_var && s.passes < 2) throw std::runtime_error("gdpt_progressive_read: variances need at least 2 passes");
        ck(hipSetDevice(s.scene->device), "hipSetDevice");
        if (want_var) compute_variances(s);
        for (int k = 0; k < s.nbuf; k++) {
            if (means) copy_out(s, means[k], s.mean[k], on_device);
            if (vars) copy_out(s, vars[k], s.var[k], on_device);
        }
        if (assembled_vars) {
            copy_out(s, assembled_vars[0], s.var[0], on_device);
            copy_out(s, assembled_vars[1], s.var[5], on_device);
            copy_out(s, assembled_vars[2], s.var[6], on_device);
        }
        ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive read)");
    });
}

int gdpt_progressive_reconstruct(GdptProgressive *session, double dataCost, const GdptReconParams *recon, int on_device, double *out,
                                 GdptReconStats *stats) {
    return gdpt::guarded([&]() {
        if (!session || !out) throw std::runtime_error("gdpt_progressive_reconstruct: null argument");
        GdptProgressive &s = *session;
        prg::reconstruct(s, dataCost, recon, stats);
        copy_out(s, out, s.asm_buf[3], on_device);
        ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive reconstruct)");
    });
}

int gdpt_progressive_reconstruct_weighted(GdptProgressive *session, double dataCost, const GdptWeightedReconParams *params, int on_device,
                                          double *out, double *const confidence[3], GdptWeightedReconStats *stats) {
    return gdpt::guarded([&]() {
        if (!session || !out) throw std::runtime_error("gdpt_progressive_reconstruct_weighted: null argument");
        GdptProgressive &s = *session;
        prg::reconstruct_weighted(s, dataCost, params, confidence, stats);
        copy_out(s, out, s.asm_buf[3], on_device);
        ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive reconstruct)");
    });
}

int gdpt_progressive_denoise(GdptProgressive *session, const GdptNlmParams *params, int on_device, double *out, double *var_out, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        if (params) gdpt::nlm_check_params(who, *params);
        GdptProgressive &s = *session;
        if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
        ck(hipSetDevice(s.scene->device), "hipSetDevice");
        compute_variances(s);
        double *d_out = out, *d_var_out = var_out;
        if (!on_device) {                 // through planes of the session's on the way to host memory
            for (int k = 0; k < (var_out ? 2 : 1); k++) if (!s.nlm_buf[k]) s.nlm_buf[k].alloc(s.elems, "hipMalloc(progressive denoise)");
            d_out = s.nlm_buf[0]; d_var_out = var_out ? s.nlm_buf[1].data() : nullptr;
        }
        GdptNlmStats st{};                // (asked for always: the call is blocking)
        if (gdpt_denoise_nlm_device(s.w, s.h, s.mean[0], s.var[0], params, d_out, d_var_out, s.stream, &st) != 0) throw std::runtime_error(gdpt_last_error());
        if (!on_device) {
            copy_out(s, out, d_out, 0);
            copy_out(s, var_out, d_var_out, 0);
            ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise)");
        }
        if (stats) *stats = st;
    });
}

int gdpt_progressive_denoise_guided(GdptProgressive *session, const GdptNlmParams *params, const GdptNlmGuide *guide, int feature_spp, int on_device,
                                    double *out, double *var_out, double *features, double *features_var, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_guided";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptNlmParams p;
        if (params) p = *params; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        GdptNlmGuide g;
        if (guide) g = *guide; else gdpt_nlm_default_guide(&g);
        gdpt::nlm_check_guide(who, g);
        if (g.num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, stats,
                             [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *st) {
                                 gdpt::denoise_nlm_guided_launch(s.w, s.h, s.mean[0], s.var[0], s.feat_buf[0], s.feat_buf[1], p, g, d_out, d_var_out, s.stream, st);
                             });
    });
}

int gdpt_progressive_denoise_regress(GdptProgressive *session, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress,
                                     int feature_spp, int on_device, double *out, double *var_out, double *features, double *features_var,
                                     GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_regress";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptNlmParams p;
        if (params) p = *params; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        GdptNlmGuide g;
        if (guide) g = *guide; else gdpt_nlm_default_guide(&g);
        gdpt::nlm_check_guide(who, g);
        if (g.num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        GdptNlmRegress rg;
        if (regress) rg = *regress; else gdpt_nlm_default_regress(&rg);
        gdpt::nlm_check_regress(who, rg, g.num_channels);
        filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, stats,
                             [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *st) {
                                 gdpt::denoise_nlm_regress_launch(s.w, s.h, s.mean[0], s.var[0], s.feat_buf[0], s.feat_buf[1], p, g, rg, d_out, d_var_out,
                                                                  s.stream, st);
                             });
    });
}

int gdpt_progressive_denoise_collab(GdptProgressive *session, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress,
                                    int feature_spp, int on_device, double *out, double *features, double *features_var, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_collab";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptNlmParams p;
        if (params) p = *params; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        GdptNlmGuide g;
        if (guide) g = *guide; else gdpt_nlm_default_guide(&g);
        gdpt::nlm_check_guide(who, g);
        if (g.num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        GdptNlmRegress rg;
        if (regress) rg = *regress; else gdpt_nlm_default_regress(&rg);
        gdpt::nlm_check_regress(who, rg, g.num_channels);
        filter_with_features(who, *session, feature_spp, on_device, out, nullptr, features, features_var, stats,
                             [&](GdptProgressive &s, double *d_out, double *, GdptNlmStats *st) {
                                 gdpt::denoise_nlm_collab_launch(s.w, s.h, s.mean[0], s.var[0], s.feat_buf[0], s.feat_buf[1], p, g, rg, d_out, nullptr,
                                                                 s.stream, st);
                             });
    });
}

int gdpt_progressive_denoise_demod(GdptProgressive *session, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod,
                                   int feature_spp, int on_device, double *out, double *var_out, double *features, double *features_var,
                                   GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_demod";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptNlmParams p;
        if (params) p = *params; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        if (guide) {                      // (NULL: no feature term)
            gdpt::nlm_check_guide(who, *guide);
            if (guide->num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        }
        GdptNlmDemod d;
        if (demod) d = *demod; else gdpt_nlm_default_demod(&d);
        gdpt::nlm_check_demod(who, d, GDPT_FEATURE_CHANNELS);
        filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, stats,
                             [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *st) {
                                 gdpt::denoise_nlm_demod_launch(s.w, s.h, s.mean[0], s.var[0], s.feat_buf[0], s.feat_buf[1], p, guide, d, d_out, d_var_out, s.stream, st);
                             });
    });
}

int gdpt_progressive_denoise_atrous(GdptProgressive *session, const GdptAtrousParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod,
                                    int feature_spp, int on_device, double *out, double *var_out, double *features, double *features_var,
                                    GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_atrous";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptAtrousParams p;
        if (params) p = *params; else gdpt_atrous_default_params(&p);
        gdpt::atrous_check_params(who, p);
        if (guide) {                      // (NULL: no feature term)
            gdpt::nlm_check_guide(who, *guide);
            if (guide->num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        }
        if (demod) gdpt::nlm_check_demod(who, *demod, GDPT_FEATURE_CHANNELS);
        if ((guide && guide->num_groups > 0) || demod) {
            filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, stats,
                                 [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *st) {
                                     gdpt::denoise_atrous_launch(s.w, s.h, s.mean[0], s.var[0], s.feat_buf[0], s.feat_buf[1], p, guide, demod, d_out, d_var_out, s.stream, st);
                                 });
            return;
        }
        // neither a group nor a demod block: no features are rendered (as gdpt_progressive_denoise)
        if (features || features_var) throw std::runtime_error(who + ": features need a group or a demod block (none are rendered without)");
        GdptProgressive &s = *session;
        if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
        ck(hipSetDevice(s.scene->device), "hipSetDevice");
        compute_variances(s);
        double *d_out = out, *d_var_out = var_out;
        if (!on_device) {                 // through planes of the session's on the way to host memory
            for (int k = 0; k < (var_out ? 2 : 1); k++) if (!s.nlm_buf[k]) s.nlm_buf[k].alloc(s.elems, "hipMalloc(progressive denoise)");
            d_out = s.nlm_buf[0]; d_var_out = var_out ? s.nlm_buf[1].data() : nullptr;
        }
        GdptNlmStats st{};                // (asked for always: the call is blocking)
        gdpt::denoise_atrous_launch(s.w, s.h, s.mean[0], s.var[0], nullptr, nullptr, p, nullptr, nullptr, d_out, d_var_out, s.stream, &st);
        if (!on_device) {
            copy_out(s, out, d_out, 0);
            copy_out(s, var_out, d_var_out, 0);
            ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise)");
        }
        if (stats) *stats = st;
    });
}

int gdpt_progressive_denoise_smoothed(GdptProgressive *session, int kind,const GdptVarSmoothParams *smooth, const GdptNlmParams *nlm,
                                      const GdptNlmGuide *guide, const GdptNlmDemod *demod, int feature_spp, int on_device, double *out,
                                      double *var_out, double *smoothed_var, double *features, double *features_var, GdptNlmStats *stats,
                                      GdptVarSmoothStats *smooth_stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_smoothed";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        if (kind != GDPT_DENOISE_PLAIN && kind != GDPT_DENOISE_GUIDED && kind != GDPT_DENOISE_DEMOD)
            throw std::runtime_error(who + ": kind must be GDPT_DENOISE_PLAIN, GDPT_DENOISE_GUIDED or GDPT_DENOISE_DEMOD");
        GdptVarSmoothParams sp;
        if (smooth) sp = *smooth; else gdpt_var_smooth_default_params(&sp);
        gdpt::var_smooth_check_params(who, sp);
        GdptNlmParams p;
        if (nlm) p = *nlm; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        if (kind == GDPT_DENOISE_PLAIN && guide) throw std::runtime_error(who + ": guide must be null for GDPT_DENOISE_PLAIN");
        if (kind != GDPT_DENOISE_DEMOD && demod) throw std::runtime_error(who + ": demod must be null unless kind is GDPT_DENOISE_DEMOD");
        if (kind == GDPT_DENOISE_PLAIN && (features || features_var))
            throw std::runtime_error(who + ": features and features_var must be null for GDPT_DENOISE_PLAIN (it renders none)");
        GdptNlmGuide g;                   // GUIDED: the guide in force
        if (guide) g = *guide; else gdpt_nlm_default_guide(&g);
        if (kind == GDPT_DENOISE_GUIDED || guide) {
            gdpt::nlm_check_guide(who, g);
            if (g.num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        }
        GdptNlmDemod d;
        if (demod) d = *demod; else gdpt_nlm_default_demod(&d);
        if (kind == GDPT_DENOISE_DEMOD) gdpt::nlm_check_demod(who, d, GDPT_FEATURE_CHANNELS);
        GdptVarSmoothStats sst{};         // (asked for always: the call is blocking)
        // the variance of buffer 0 into s.smooth_buf, on the planes of `dm` (nullable) in s.feat_buf, and its copy out
        auto smoothed = [&](GdptProgressive &s, const GdptNlmDemod *dm) {
            if (!s.smooth_buf) s.smooth_buf.alloc(s.elems, "hipMalloc(progressive smoothed variance)");
            gdpt::variance_smooth_launch(s.w, s.h, s.mean[0], s.var[0], dm ? s.feat_buf[0].data() : nullptr, dm ? s.feat_buf[1].data() : nullptr, sp, dm,
                                         s.smooth_buf, s.stream, &sst);
            copy_out(s, smoothed_var, s.smooth_buf, on_device);
        };
        if (kind == GDPT_DENOISE_PLAIN) {
            GdptProgressive &s = *session;
            if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
            ck(hipSetDevice(s.scene->device), "hipSetDevice");
            compute_variances(s);
            double *d_out = out, *d_var_out = var_out;
            if (!on_device) {                 // through planes of the session's on the way to host memory
                for (int k = 0; k < (var_out ? 2 : 1); k++) if (!s.nlm_buf[k]) s.nlm_buf[k].alloc(s.elems, "hipMalloc(progressive denoise)");
                d_out = s.nlm_buf[0]; d_var_out = var_out ? s.nlm_buf[1].data() : nullptr;
            }
            smoothed(s, nullptr);
            GdptNlmStats st{};
            if (gdpt_denoise_nlm_device(s.w, s.h, s.mean[0], s.smooth_buf, &p, d_out, d_var_out, s.stream, &st) != 0) throw std::runtime_error(gdpt_last_error());
            if (!on_device) { copy_out(s, out, d_out, 0); copy_out(s, var_out, d_var_out, 0); }
            ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise)");
            if (stats) *stats = st;
        } else {
            filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, stats,
                                 [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *st) {
                                     if (kind == GDPT_DENOISE_DEMOD) {
                                         smoothed(s, &d);
                                         gdpt::denoise_nlm_demod_launch(s.w, s.h, s.mean[0], s.smooth_buf, s.feat_buf[0], s.feat_buf[1], p, guide ? &g : nullptr, d,
                                                                        d_out, d_var_out, s.stream, st);
                                     } else {
                                         smoothed(s, nullptr);
                                         gdpt::denoise_nlm_guided_launch(s.w, s.h, s.mean[0], s.smooth_buf, s.feat_buf[0], s.feat_buf[1], p, g, d_out, d_var_out,
                                                                         s.stream, st);
                                     }
                                 });
        }
        if (smooth_stats) *smooth_stats = sst;
    });
}

int gdpt_progressive_denoise_reconstruct(GdptProgressive *session, const GdptNlmParams *nlm, const GdptNlmGuide *guide, int feature_spp,
                                         const GdptVarSmoothParams *var_smooth, double dataCost, const GdptWeightedReconParams *weighted_recon,
                                         int on_device, double *out, double *const filtered[3], double *const filtered_var[3],
                                         GdptNlmJointStats *stats, GdptWeightedReconStats *recon_stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_reconstruct";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        GdptNlmParams p;
        if (nlm) p = *nlm; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        GdptNlmGuide g;                   // guide == NULL: no group, so no feature term and no planes
        if (guide) g = *guide; else { gdpt_nlm_default_guide(&g); g.num_groups = 0; }
        gdpt::nlm_check_guide(who, g);
        if (guide && g.num_channels != GDPT_FEATURE_CHANNELS) throw std::runtime_error(who + ": num_channels must be GDPT_FEATURE_CHANNELS (the session renders its own features)");
        if (var_smooth) gdpt::var_smooth_check_params(who, *var_smooth);
        GdptProgressive &s = *session;
        if (s.nbuf != 5) throw std::runtime_error(who + ": an Integrator::Path session has no gradients (filter its mean with gdpt_progressive_denoise*)");
        if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
        if (guide && (feature_spp < 2 || feature_spp > s.block)) throw std::runtime_error(who + ": feature_spp must be in [2, budget_spp]");
        ck(hipSetDevice(s.scene->device), "hipSetDevice");
        assemble_means(s);
        compute_variances(s);
        const double *d_var_c = s.var[0];
        if (var_smooth) {                 // the guide film's variance only: the companions' and the reconstruction's stay the session's
            if (!s.smooth_buf) s.smooth_buf.alloc(s.elems, "hipMalloc(progressive smoothed variance)");
            gdpt::variance_smooth_launch(s.w, s.h, s.asm_buf[0], s.var[0], nullptr, nullptr, *var_smooth, nullptr, s.smooth_buf, s.stream, nullptr);
            d_var_c = s.smooth_buf;
        }
        if (guide) {                      // the feature render of gdpt_progressive_denoise_guided (filter_with_features)
            const size_t felems = (size_t)s.w * s.h * GDPT_FEATURE_CHANNELS;
            for (auto &b : s.feat_buf) if (!b) b.alloc(felems, "hipMalloc(progressive features)");
            GdptRenderParams rp{};
            rp.spp = feature_spp; rp.rng_scheme = GDPT_RNG_SAMPLE;
            const GdptSampleWindow win{s.block, 0};
            if (!s.feat_current) gdpt::features_launch(s.scene, &rp, &win, s.feat_buf[0], s.feat_buf[1], s.stream, nullptr);
        }
        for (auto &b : s.joint_buf) if (!b) b.alloc(s.elems, "hipMalloc(progressive joint filter)");
        const double *comp[2] = {s.asm_buf[1], s.asm_buf[2]}, *comp_var[2] = {s.var[5], s.var[6]};
        double *comp_out[2] = {s.joint_buf[1], s.joint_buf[2]}, *comp_var_out[2] = {s.joint_buf[4], s.joint_buf[5]};
        GdptNlmJointStats st{};           // (asked for always: the call is blocking)
        gdpt::denoise_nlm_joint_launch(s.w, s.h, s.asm_buf[0], d_var_c, guide ? s.feat_buf[0].data() : nullptr, guide ? s.feat_buf[1].data() : nullptr, 2,
                                       comp, comp_var, p, g, s.joint_buf[0], s.joint_buf[3], comp_out, comp_var_out, s.stream, &st);
        GdptWeightedReconStats rs{};
        if (weighted_recon) {
            if (gdpt_reconstruct_weighted_device(s.w, s.h, s.joint_buf[0], s.joint_buf[1], s.joint_buf[2], s.joint_buf[3], s.joint_buf[4], s.joint_buf[5],
                                                 dataCost, weighted_recon, s.asm_buf[3], nullptr, s.stream, &rs) != 0)
                throw std::runtime_error(gdpt_last_error());
        } else if (gdpt_reconstruct_device(s.w, s.h, s.joint_buf[0], s.joint_buf[1], s.joint_buf[2], dataCost, nullptr, s.asm_buf[3], s.stream, &rs.recon) != 0)
            throw std::runtime_error(gdpt_last_error());
        copy_out(s, out, s.asm_buf[3], on_device);
        for (int k = 0; k < 3; k++) {
            if (filtered) copy_out(s, filtered[k], s.joint_buf[k], on_device);
            if (filtered_var) copy_out(s, filtered_var[k], s.joint_buf[3 + k], on_device);
        }
        ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise reconstruct)");
        if (stats) *stats = st;
        if (recon_stats) *recon_stats = rs;
    });
}

int gdpt_progressive_denoise_multiscale(GdptProgressive *session, int kind, int levels, const GdptVarSmoothParams *smooth, const GdptNlmParams *nlm,
                                        const GdptNlmGuide *guide, const GdptNlmDemod *demod, int feature_spp, int on_device, double *out,
                                        double *var_out, double *features, double *features_var, GdptNlmPyramidStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_denoise_multiscale";
        if (!session) throw std::runtime_error(who + ": null session");
        if (!out) throw std::runtime_error(who + ": out is null");
        // (the session renders its own planes: a guide must be over GDPT_FEATURE_CHANNELS of them)
        const gdpt::NlmKindBlocks kb = gdpt::nlm_pyramid_check_kind(who, kind, guide, demod, GDPT_FEATURE_CHANNELS, kind == GDPT_DENOISE_GUIDED || kind == GDPT_DENOISE_DEMOD);
        gdpt::nlm_pyramid_check_levels(who, levels);
        if (smooth) gdpt::var_smooth_check_params(who, *smooth);
        GdptNlmParams p;
        if (nlm) p = *nlm; else gdpt_nlm_default_params(&p);
        gdpt::nlm_check_params(who, p);
        if (kind == GDPT_DENOISE_PLAIN && (features || features_var))
            throw std::runtime_error(who + ": features and features_var must be null for GDPT_DENOISE_PLAIN (it renders none)");
        GdptNlmPyramidStats pst{};        // (asked for always: the call is blocking)
        // the variance the levels start from: buffer 0's as estimated, or smoothed into s.smooth_buf as gdpt_progressive_denoise_smoothed does
        auto variance = [&](GdptProgressive &s) -> const double * {
            if (!smooth) return s.var[0];
            if (!s.smooth_buf) s.smooth_buf.alloc(s.elems, "hipMalloc(progressive smoothed variance)");
            const bool dm = kind == GDPT_DENOISE_DEMOD;
            gdpt::variance_smooth_launch(s.w, s.h, s.mean[0], s.var[0], dm ? s.feat_buf[0].data() : nullptr, dm ? s.feat_buf[1].data() : nullptr, *smooth,
                                         dm ? &kb.demod : nullptr, s.smooth_buf, s.stream, nullptr);
            return s.smooth_buf;
        };
        if (kind == GDPT_DENOISE_PLAIN) {
            GdptProgressive &s = *session;
            if (s.passes < 2) throw std::runtime_error(who + ": variances need at least 2 passes");
            ck(hipSetDevice(s.scene->device), "hipSetDevice");
            compute_variances(s);
            double *d_out = out, *d_var_out = var_out;
            if (!on_device) {                 // through planes of the session's on the way to host memory
                for (int k = 0; k < (var_out ? 2 : 1); k++) if (!s.nlm_buf[k]) s.nlm_buf[k].alloc(s.elems, "hipMalloc(progressive denoise)");
                d_out = s.nlm_buf[0]; d_var_out = var_out ? s.nlm_buf[1].data() : nullptr;
            }
            gdpt::denoise_nlm_multiscale_launch(s.w, s.h, s.mean[0], variance(s), nullptr, nullptr, kb, levels, p, d_out, d_var_out, s.stream, &pst);
            if (!on_device) { copy_out(s, out, d_out, 0); copy_out(s, var_out, d_var_out, 0); }
            ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(progressive denoise)");
        } else {
            filter_with_features(who, *session, feature_spp, on_device, out, var_out, features, features_var, nullptr,
                                 [&](GdptProgressive &s, double *d_out, double *d_var_out, GdptNlmStats *) {
                                     gdpt::denoise_nlm_multiscale_launch(s.w, s.h, s.mean[0], variance(s), s.feat_buf[0], s.feat_buf[1], kb, levels, p, d_out,
                                                                         d_var_out, s.stream, &pst);
                                 });
        }
        if (stats) *stats = pst;
    });
}

int gdpt_progressive_run(GdptProgressive *session, double target_error, int pass_spp, int max_passes, GdptProgressiveStatus *status) {
    return gdpt::guarded([&]() {
        if (!session) throw std::runtime_error("gdpt_progressive_run: null session");
        if (pass_spp <= 0) throw std::runtime_error("gdpt_progressive_run: pass_spp must be > 0");
        if (std::isnan(target_error)) throw std::runtime_error("gdpt_progressive_run: target_error is NaN");
        GdptProgressive &s = *session;
        if (s.group_half) throw std::runtime_error("gdpt_progressive_run: the session is a half of a group (run the group)");
        if (s.group_total) throw std::runtime_error("gdpt_progressive_run: the session is the total of a group (run the group)");
        auto reached = [&]() { return target_error > 0 && s.passes >= 2 && error_estimate(s) <= target_error; };
        int added = 0;
        for (;;) {
            if (reached()) { s.stop_reason = GDPT_STOP_TARGET; break; }
            if (s.own_done >= s.own) { s.stop_reason = GDPT_STOP_BUDGET; break; }
            if (max_passes > 0 && added >= max_passes) { s.stop_reason = GDPT_STOP_MAX_PASSES; break; }
            prg::add_pass(s, std::min(pass_spp, s.own - s.own_done), nullptr);
            added++;
        }
        fill_status(s, status);
    });
}

} // extern "C"
