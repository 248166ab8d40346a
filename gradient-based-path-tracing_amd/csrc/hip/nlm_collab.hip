// nlm_collab.hip — the collaborative form of the first-order feature regression, for gfx950 (include/gdpt.h: gdpt_denoise_nlm_collab*,
// where the definition stands; Bitterli et al. 2016, section 4.3 "collaborative filtering").
//
// Two passes with a coefficient film between them: 3 d channel-planar planes of W H doubles, plane c d + j holding beta_c,j.
//   collab_fit_*      the first sweep of the regression kernels (nlm_regress.hip) and the LDL^T solve of the three right-hand sides: the
//                     same Stage::sweep, Fit::add and Ldlt, so plane c d + 0 is gdpt_denoise_nlm_regress's out channel c bit for bit.
//                     There is no second sweep; the thread stores its 3 d coefficients.
//   collab_gather_*   every valid q averages the fits of the valid p = q + t, |t|_inf <= r, at its own regressor values, under the
//                     weight the fit centred at p gave its partner q: w_{-t}(p). Neither distance is symmetric in its variances, so
//                     the pair distances are taken with p's triple first and the feature distance with p in the centre's place.
// Each in two forms chosen by the test knob nlm_direct (include/gdpt_debug.h), built as the regression's: 16 x 16 tiles, a thread on
// a pixel, the nlm grid rule of image_kernels.h, block partials through leave_block_sum for finish_kernel. The tiled gather runs the
// regression's LDS stage with the roles of an offset's two pixels swapped; p's feature values and its coefficients come from global
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
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = ga.num[c] / ga.den;
        k.a.out[i + c] = o[c];
    }
    s.var_in += (v[0] + v[1]) + v[2];
    s.sq_in += (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
}

__global__ __launch_bounds__(kBlock) void collab_fit_direct_kernel(Args k) {
    const nlmr::Args &a = k.a;
    const int r = a.r;
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
                patch_distance(a, x, y, ox, oy, S, C);      // (C >= 1: the tap n = 0 counts)
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
                patch_distance(a, px, py, -tx, -ty, S, C);     // the fit centred at p, its offset o = -t
                const size_t ip = (size_t)py * a.g.w + px;
                ga.add(k, reg, ip, pair_weight(S, C, distance_from(a.gd, own, ip)));
            }
        finish_pixel(k, i, u, v, ga, s);
    }
    leave_partials(a, s, red);
}

// the regression's stage in the block's LDS (regress_tiled_kernel's layout)
__device__ __forceinline__ void lay_out(Stage &st, const nlmr::Args &a, double *lds) {
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
}

// the tile at (x0, y0) with its halo into the stage; the caller's barriers stand before and after
__device__ __forceinline__ void fill(const Stage &st, const nlmr::Args &a, int x0, int y0) {
    const int halo = a.r + a.f;
    for (int k = st.tid; k < st.sn; k += kBlock) {
        const int ry = k / st.sw, rx = k - ry * st.sw;
        const int gx = x0 - halo + rx, gy = y0 - halo + ry;
        double u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
        bool ok = false;
        if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) ok = load_pixel(a, gx, gy, u, v);
#pragma unroll
        for (int c = 0; c < 3; c++) { st.su[c * st.sn + k] = ok ? u[c] : 0.0; st.sv[c * st.sn + k] = ok ? v[c] : 0.0; }
        st.sflag[k] = ok ? 1 : 0;
    }
}

// Stage::sweep with the roles of an offset's two pixels swapped: tap(ip, S, C, ty, tx) is called for the thread's own pixel q and every
// valid p = q + t, with S and C of the fit centred at p for its offset -t, that is the pair distances e(p + n, q + n) with p's triple
// first, over the same patch taps n and summed in the same separable order as the fit's.
template <class Tap>
__device__ __forceinline__ void sweep_from_partner(const Stage &st, const nlmr::Args &a, bool okq, Tap tap) {
    const int r = st.r, sw = st.sw, sn = st.sn, taps = st.taps, tid = st.tid;
    for (int ty = -r; ty <= r; ty++)
        for (int tx = -r; tx <= r; tx++) {
            const int shift = ty * sw + tx;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (st.ia[k] < 0) continue;
                const int i0 = st.ia[k], i1 = i0 + shift;
                const int both = st.sflag[i0] & st.sflag[i1];
                double e = 0.0;
                if (both) {
                    double ua[3], va[3], ub[3], vb[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) { ua[c] = st.su[c * sn + i1]; va[c] = st.sv[c * sn + i1]; ub[c] = st.su[c * sn + i0]; vb[c] = st.sv[c * sn + i0]; }
                    e = pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
                }
                st.pe[st.ie[k]] = e; st.ce[st.ie[k]] = both;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (st.jrow[k] < 0) continue;
                double S = 0.0;
                int C = 0;
                for (int n = 0; n < taps; n++) { S += st.pe[st.jrow[k] + n]; C += st.ce[st.jrow[k] + n]; }
                st.ph[tid + k * kBlock] = S; st.ch[tid + k * kBlock] = C;
            }
            __syncthreads();
            const int ip = st.pc + shift;
            if (okq && st.sflag[ip] != 0) {
                double S = 0.0;
                int C = 0;
                for (int n = 0; n < taps; n++) { S += st.ph[tid + n * kTile]; C += st.ch[tid + n * kTile]; }
                tap(ip, S, C, ty, tx);
            }
        }
}

__global__ __launch_bounds__(kBlock) void collab_fit_tiled_kernel(Args k) {
    extern __shared__ double lds[];
    const nlmr::Args &a = k.a;
    Stage st;
    lay_out(st, a, lds);
    const int sn = st.sn, pc = st.pc;
    double *const su = st.su;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage has been read
        fill(st, a, tp.x0, tp.y0);
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
        st.sweep(a, okp, [&](int iq, double S, int C, int oy, int ox) {
            const size_t gq = (size_t)(y + oy) * a.g.w + (x + ox);
            const double w = pair_weight(S, C, own.distance(a.gd, gq));
            const double uq[3] = {su[iq], su[sn + iq], su[2 * sn + iq]};
            double z[kD];
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
    lay_out(st, a, lds);
    const int sn = st.sn, pc = st.pc;
    double *const su = st.su, *const sv = st.sv;
    Sums s;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage has been read
        fill(st, a, tp.x0, tp.y0);
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const bool okq = inside && st.sflag[pc] != 0;
        OwnFeatures own;
        OwnRegressors reg;
        if (okq) { own.load(a.gd, (size_t)y * a.g.w + x); reg.load(a.rg, a.gd, (size_t)y * a.g.w + x); }
        Gather ga;
        sweep_from_partner(st, a, okq, [&](int, double S, int C, int ty, int tx) {
            const size_t gp = (size_t)(y + ty) * a.g.w + (x + tx);
            ga.add(k, reg, gp, pair_weight(S, C, distance_from(a.gd, own, gp)));
        });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        if (okq) {
            const double u[3] = {su[pc], su[sn + pc], su[2 * sn + pc]}, v[3] = {sv[pc], sv[sn + pc], sv[2 * sn + pc]};
            finish_pixel(k, i, u, v, ga, s);
        } else {
            double u[3], v[3];
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
        }
    }
    leave_partials(a, s, red);
}

} // namespace nlmc

namespace gdpt {

namespace {

struct CollabWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;
    DeviceBuffer<double> coef;        // the coefficient film of a call that brings none; grown on demand
    DeviceBuffer<film::Estimate> d_est;     // [0] sum var in, sum u^2 in, left out; [1] (unused), sum u^2 out, left out
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
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
    if (!ws.partials) ws.partials.alloc(6 * film::kMaxBlocks, "hipMalloc(nlm collab partials)");
    if (!ws.d_est) ws.d_est.alloc(2, "hipMalloc(nlm collab sums)");
    if (!ws.h_est) ws.h_est.alloc(2, "hipHostMalloc(nlm collab sums)");
    for (auto &e : ws.ev) if (!e) e.create();
    const int d = 1 + rg.num_regressors;
    if (!d_coef) {
        ws.coef.grow((size_t)3 * d * w * h, stream, "hipMalloc(nlm collab coefficients)");
        d_coef = ws.coef;
    }

    nlmc::Args k{};
    nlmr::Args &a = k.a;
    a.g = film::tile_grid(w, h, kNlmTile, kNlmTile); a.r = p.window_radius; a.f = p.patch_radius;
    a.k2 = p.k * p.k; a.alpha = p.alpha; a.eps = p.epsilon;
    a.img = d_img; a.var = d_var; a.out = d_out; a.var_out = nullptr; a.partials = ws.partials;
    a.second = 0;
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
    k.coef = d_coef; k.d = d;
    const int nb = a.g.blocks;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    const int pass = debug_knob_int("nlm_collab_pass", 0);      // measurements: 1 the fit alone, 2 the gather alone
    const bool fit = pass != 2, gather = pass != 1;
    if (debug_knob("nlm_direct", 0) != 0) {
        if (fit) hipLaunchKernelGGL(nlmc::collab_fit_direct_kernel, dim3(nb), dim3(film::kBlock), 0, stream, k);
        if (gather) hipLaunchKernelGGL(nlmc::collab_gather_direct_kernel, dim3(nb), dim3(film::kBlock), 0, stream, k);
    } else {
        const size_t lds = (size_t)nlm::lds_doubles(a.r, a.f) * sizeof(double) + (size_t)nlm::lds_ints(a.r, a.f) * sizeof(int);
        ck(hipFuncSetAttribute(reinterpret_cast<const void *>(nlmc::collab_fit_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "hipFuncSetAttribute(nlm collab stage)");
        ck(hipFuncSetAttribute(reinterpret_cast<const void *>(nlmc::collab_gather_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "hipFuncSetAttribute(nlm collab stage)");
        if (fit) hipLaunchKernelGGL(nlmc::collab_fit_tiled_kernel, dim3(nb), dim3(film::kBlock), lds, stream, k);
        if (gather) hipLaunchKernelGGL(nlmc::collab_gather_tiled_kernel, dim3(nb), dim3(film::kBlock), lds, stream, k);
    }
    ck(hipGetLastError(), "nlm collab launch");
    if (!stats) return;
    if (!gather) ck(hipMemsetAsync(ws.partials, 0, 6 * film::kMaxBlocks * sizeof(double), stream), "hipMemsetAsync(nlm collab partials)");      // (no sums)
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    film::launch_finish(nb, ws.partials.data() + 3 * nb, ws.d_est.data() + 1, stream);
    ck(hipGetLastError(), "nlm collab reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, 2 * sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(nlm collab sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm collab)");
    *stats = GdptNlmStats{};
    const film::Estimate &in = ws.h_est.data()[0], &out = ws.h_est.data()[1];
    const double not_estimated = std::numeric_limits<double>::quiet_NaN();
    stats->pixels_left_out = (uint64_t)in.left_out;
    stats->sum_var_in = in.sum_var; stats->sum_sq_in = in.sum_mean2;
    stats->sum_var_out = not_estimated; stats->sum_sq_out = out.sum_mean2;
    stats->error_in = std::sqrt(in.sum_var / in.sum_mean2);
    stats->error_out = not_estimated;
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->filter_ms = ms; }
    stats->window_radius = p.window_radius; stats->patch_radius = p.patch_radius;
}

} // namespace gdpt

namespace {

using gdpt::ck;

// whether [a, a + na) and [b, b + nb) doubles share an address; a null range shares none
bool overlap(const double *a, size_t na, const double *b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(double), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(double);
    return a0 < b1 && b0 < a1;
}

// The blocks in force of a call, every argument checked: what the regression's entry points refuse, and a coefficient film that
// overlaps an input or out. `who` names the caller.
struct Blocks { GdptNlmParams p; GdptNlmGuide g; GdptNlmRegress rg; };
Blocks check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                       const double *feat_var, const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress,
                       const double *out, const double *coef) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (out == img || out == var) throw std::runtime_error(who + ": out must not alias an input");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    Blocks b;
    if (params) b.p = *params; else gdpt_nlm_default_params(&b.p);
    gdpt::nlm_check_params(who, b.p);
    if (guide) b.g = *guide; else gdpt_nlm_default_guide(&b.g);
    gdpt::nlm_check_guide(who, b.g);
    if (regress) b.rg = *regress; else gdpt_nlm_default_regress(&b.rg);
    gdpt::nlm_check_regress(who, b.rg, b.g.num_channels);
    const bool planes = b.g.num_groups > 0 || b.rg.num_regressors > 0;
    if (planes) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    if (feat && (out == feat || out == feat_var)) throw std::runtime_error(who + ": out must not alias an input");
    const size_t px = (size_t)width * height, nc = 3 * (size_t)(1 + b.rg.num_regressors) * px, nf = planes ? px * b.g.num_channels : 0;
    if (overlap(coef, nc, img, 3 * px) || overlap(coef, nc, var, 3 * px) || overlap(coef, nc, out, 3 * px) || overlap(coef, nc, feat, nf) ||
        overlap(coef, nc, feat_var, nf))
        throw std::runtime_error(who + ": coef must not overlap an input or out");
    return b;
}

void need_a_device(const std::string &who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }      // (without a device the count itself is an error)
    if (ndev <= 0) throw std::runtime_error(who + ": no HIP device visible (this library has no CPU fallback)");
}

} // namespace

extern "C" {

int gdpt_denoise_nlm_collab_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *d_out,
                                   double *d_coef, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_collab_device";
        const Blocks b = check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, params, guide, regress, d_out, d_coef);
        need_a_device(who);
        gdpt::denoise_nlm_collab_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_coef, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_collab(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                            const GdptNlmParams *params, const GdptNlmGuide *guide, const GdptNlmRegress *regress, double *out, double *coef,
                            GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_collab";
        const Blocks b = check_arguments(who, width, height, img, var, feat, feat_var, params, guide, regress, out, coef);
        need_a_device(who);
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        const bool planes = b.g.num_groups > 0 || b.rg.num_regressors > 0;
        const size_t felems = planes ? (size_t)width * height * b.g.num_channels : 0, fbytes = felems * sizeof(double);
        const size_t celems = coef ? elems * (size_t)(1 + b.rg.num_regressors) : 0;
        gdpt::DeviceBuffer<double> d_img, d_var, d_out, d_coef, d_feat, d_feat_var;
        d_img.alloc(elems, "hipMalloc(nlm io)"); d_var.alloc(elems, "hipMalloc(nlm io)"); d_out.alloc(elems, "hipMalloc(nlm io)");
        d_coef.alloc(celems, "hipMalloc(nlm io)");
        d_feat.alloc(felems, "hipMalloc(nlm features)"); d_feat_var.alloc(felems, "hipMalloc(nlm features)");
        ck(hipMemcpy(d_img, img, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        if (felems) {
            ck(hipMemcpy(d_feat, feat, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            ck(hipMemcpy(d_feat_var, feat_var, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        }
        gdpt::denoise_nlm_collab_launch(width, height, d_img, d_var, d_feat, d_feat_var, b.p, b.g, b.rg, d_out, d_coef, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (coef) ck(hipMemcpy(coef, d_coef, celems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
