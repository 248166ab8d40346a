// temporal.hip — temporal reprojection: the accumulated mean, its variance of the mean and the history length carried across a camera
// move, for gfx950 (include/gdpt.h: gdpt_temporal_*, where the definition stands; Schied et al. 2017, the temporal half).
//
// One kernel per push, a thread on a pixel, 16 x 16 tiles under the "nlm" grid rule (film::tile_grid: a film past the block cap takes
// further trips). The pixel's world point comes from the camera code of the render kernels (gd::camera_ray, device_trace.h) and its
// own depth; the previous frame's matrix M, both camera positions and the current camera are kernel arguments, so they are
// wave-uniform and stay in SGPRs. The four bilinear taps are gathered from global memory: the reprojected footprint of a tile is
// arbitrary (a rotation shears it, a dolly scales it), so there is no LDS stage. A tap reads N first, then coverage, depth and the
// normal, and the six doubles of U and V only if it is valid.
//   Layout. U and V are interleaved (3 doubles a pixel) like the films they are blended with: under a coherent reprojection the 16
//   lanes of a tile row read 16 neighbouring history pixels, 384 contiguous bytes over the three channel loads, so every line
//   fetched is used whole. N and the geometry (unit normal, depth, coverage) are planar like the feature planes they are copied
//   from: a lane row reads 128 contiguous bytes a plane, and a tap that fails on N or coverage touches no other plane.
// The handle owns two history sets that alternate: a push reads one and writes the other, so no launch writes a plane it reads. The
// four sums (three counts and the sum of N') leave through leave_block_sum and finish_runs_kernel (image_kernels.h): a fixed order.
//   Gradients (gdpt_temporal_push_gradients*). push_kernel_t<GradArgs> is the same body and the same gather under a template
//   parameter: the plain kernel, push_kernel_t<>, is the instantiation without it and keeps its argument and its code. A valid tap
//   reads, after U and V, its 12 gradient doubles (G_x, G_y, VG_x, VG_y by channel, interleaved: one pixel's 96 bytes are contiguous, so a lane row reads 16 x 96 contiguous
//   bytes) and N_g. The Jacobian of the reprojection costs two more camera rays and two more products with M(prev) a pixel, all on
//   kernel arguments: no memory traffic. Two more sums (gradient resets, the sum of N_g') leave by the same route.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "../host/host_math.h"
#include "../host/scene_prepare.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "device_trace.h"
#include "nlm_host.h"
#include "temporal.h"

#include <cmath>
#include <memory>
#include <mutex>

namespace temporal {

using film::kBlock;
constexpr int kTile = gdpt::kNlmTile;
constexpr int kGeomPlanes = 5;        // of a history set: unit normal x, y, z; depth / coverage; coverage
constexpr int kRuns = 4;              // left out, background, reset, sum of N'
constexpr int kGradRuns = 6;          // and: gradient resets, sum of N_g'
constexpr int kGradDoubles = 12;      // of a pixel of the gradient history: G_x, G_y, VG_x, VG_y, three channels each

struct Args {
    film::TileGrid g;
    DevCamera cam;                    // the frame's camera
    double Mprev[16], org_prev[3];    // M and the position of the previous frame's camera
    double tau_z, tau_n, s_min, max_history;
    int first;                        // the first push after create or reset: no history is read
    const double *img, *var, *feat;   // the frame
    const double *pU, *pV, *pN, *pG;  // the history read
    double *nU, *nV, *nN, *nG;        // the history written
    double *out, *var_out, *len;      // len nullable
    double *partials;                 // kRuns runs of gridDim.x partials
};

// what the gradient kernel takes beside Args
struct GradArgs {
    double j_max, cos_min;
    int stale;                        // the gradient history holds nothing: every gradient restarts, and pH, pNg are not read
    const double *gx, *gx_var, *gy, *gy_var;      // the frame's
    const double *pH, *pNg;           // the gradient history read: kGradDoubles a pixel, and N_g
    double *nH, *nNg;                 // and written
    double *gx_out, *gx_var_out, *gy_out, *gy_var_out, *glen;      // glen nullable
};

struct History { double U[3], V[3], N; };
// the gathered gradients (k = 0: x, 1: y), and what the Jacobian needs of the pixel's own reprojection
struct GradHistory { double G[2][3], VG[2][3], N, qx, qy, c0; };

// the history of the surface pixel (x, y) with depth d and unit normal n; false: reset. kGrad: the gradient history by the same taps
template <bool kGrad>
__device__ __forceinline__ bool gather(const Args &a, const GradArgs &ga, int x, int y, double d, gd::D3 n, History &h, GradHistory &gh) {
    const int W = a.g.w, H = a.g.h;
    const size_t plane = (size_t)W * H;
    const gd::Ray r = gd::camera_ray(a.cam, (x + 0.5) / a.cam.width, (y + 0.5) / a.cam.height);
    const gd::D3 X = r.org + d * r.dir;
    const double *M = a.Mprev;
    const double sx = M[0] * X.x + M[1] * X.y + M[2] * X.z + M[3];
    const double sy = M[4] * X.x + M[5] * X.y + M[6] * X.z + M[7];
    const double w = M[12] * X.x + M[13] * X.y + M[14] * X.z + M[15];
    if (!(w > 0.0)) return false;
    const double qx = sx / w * W - 0.5, qy = sy / w * H - 0.5;
    if (!(qx >= -1.0 && qx <= (double)W && qy >= -1.0 && qy <= (double)H)) return false;     // (a NaN ends here)
    const double flx = floor(qx), fly = floor(qy);
    const int i0 = (int)flx, j0 = (int)fly;
    const double fx = qx - flx, fy = qy - fly;
    const double e = gd::length(X - gd::mk(a.org_prev[0], a.org_prev[1], a.org_prev[2]));
    double S = 0.0, Us[3] = {0.0, 0.0, 0.0}, Vs[3] = {0.0, 0.0, 0.0}, Ns = 0.0;
    double Gs[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, VGs[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, Ngs = 0.0;
#pragma unroll
    for (int tb = 0; tb < 2; tb++)
#pragma unroll
        for (int ta = 0; ta < 2; ta++) {
            const int tx = i0 + ta, ty = j0 + tb;
            if (tx < 0 || ty < 0 || tx >= W || ty >= H) continue;
            const size_t q = (size_t)ty * W + tx;
            const double Nq = a.pN[q];
            if (!(Nq >= 1.0)) continue;
            if (!(a.pG[4 * plane + q] > 0.0)) continue;
            if (!(fabs(a.pG[3 * plane + q] - e) <= a.tau_z * e)) continue;
            const gd::D3 nq = gd::mk(a.pG[q], a.pG[plane + q], a.pG[2 * plane + q]);
            if (nq.x == 0.0 && nq.y == 0.0 && nq.z == 0.0) continue;      // (a pixel without a normal: no tap at any tau_n)
            if (!(gd::dot(n, nq) >= a.tau_n)) continue;
            const double bt = (ta ? fx : 1.0 - fx) * (tb ? fy : 1.0 - fy);
            S += bt;
#pragma unroll
            for (int c = 0; c < 3; c++) { Us[c] += bt * a.pU[3 * q + c]; Vs[c] += (bt * bt) * a.pV[3 * q + c]; }
            Ns += bt * Nq;
            if constexpr (kGrad) {
                if (!ga.stale) {
                    const double *hq = ga.pH + (size_t)kGradDoubles * q;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        Gs[0][c] += bt * hq[c]; Gs[1][c] += bt * hq[3 + c];
                        VGs[0][c] += (bt * bt) * hq[6 + c]; VGs[1][c] += (bt * bt) * hq[9 + c];
                    }
                    Ngs += bt * ga.pNg[q];
                }
            }
        }
    if (!(S >= a.s_min)) return false;
    const double S2 = S * S;
#pragma unroll
    for (int c = 0; c < 3; c++) { h.U[c] = Us[c] / S; h.V[c] = Vs[c] / S2; }
    h.N = Ns / S;
    if constexpr (kGrad) {
#pragma unroll
        for (int k = 0; k < 2; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) { gh.G[k][c] = Gs[k][c] / S; gh.VG[k][c] = VGs[k][c] / S2; }
        gh.N = Ngs / S; gh.qx = qx; gh.qy = qy; gh.c0 = gd::dot(n, r.dir);
    }
    return true;
}

// The Jacobian of the reprojection at the blending surface pixel (x, y), by backward differences along the plane through its world
// point with normal n: J = {Jxx, Jyx, Jxy, Jyy}. false: GRADIENT RESET.
__device__ __forceinline__ bool jacobian(const Args &a, const GradArgs &ga, int x, int y, double d, gd::D3 n, const GradHistory &gh, double J[4]) {
    const double *M = a.Mprev;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const gd::Ray r = gd::camera_ray(a.cam, (x + (k == 0 ? -0.5 : 0.5)) / a.cam.width, (y + (k == 1 ? -0.5 : 0.5)) / a.cam.height);
        const double ck = gd::dot(n, r.dir);
        if (fabs(ck) < ga.cos_min) return false;
        const double ratio = gh.c0 / ck;
        if (!(ratio > 0.0)) return false;
        const gd::D3 X = r.org + (d * ratio) * r.dir;
        const double sx = M[0] * X.x + M[1] * X.y + M[2] * X.z + M[3];
        const double sy = M[4] * X.x + M[5] * X.y + M[6] * X.z + M[7];
        const double w = M[12] * X.x + M[13] * X.y + M[14] * X.z + M[15];
        if (!(w > 0.0)) return false;
        const double jx = gh.qx - (sx / w * a.g.w - 0.5), jy = gh.qy - (sy / w * a.g.h - 0.5);
        if (!(fabs(jx) <= ga.j_max && fabs(jy) <= ga.j_max)) return false;      // (a non-finite entry ends here)
        J[2 * k] = jx; J[2 * k + 1] = jy;
    }
    return true;
}

__device__ __forceinline__ GradArgs grad_of() { return GradArgs{}; }
__device__ __forceinline__ const GradArgs &grad_of(const GradArgs &ga) { return ga; }

// push_kernel_t<> is the plain kernel, its one argument and its code; push_kernel_t<GradArgs> carries the gradients along
template <class... GA>
__global__ __launch_bounds__(kBlock) void push_kernel_t(Args a, GA... grad) {
    constexpr bool kGrad = sizeof...(GA) > 0;
    __shared__ double red[kBlock / 64];
    const GradArgs &ga = grad_of(grad...);
    const size_t plane = (size_t)a.g.w * a.g.h;
    double n_left = 0.0, n_bg = 0.0, n_reset = 0.0, n_len = 0.0, n_greset = 0.0, n_glen = 0.0;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const film::TilePixel tp = film::tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t p = (size_t)y * a.g.w + x;
        double u[3], v[3], o[3], vo[3];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            u[c] = a.img[3 * p + c]; v[c] = a.var[3 * p + c];
            o[c] = u[c]; vo[c] = v[c];
            ok = ok && isfinite(u[c]) && isfinite(v[c]) && v[c] >= 0.0;
        }
        double g[2][3], gv[2][3], go[2][3], gvo[2][3], Ngp = 1.0;
        if constexpr (kGrad) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                g[0][c] = ga.gx[3 * p + c]; gv[0][c] = ga.gx_var[3 * p + c]; g[1][c] = ga.gy[3 * p + c]; gv[1][c] = ga.gy_var[3 * p + c];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    go[k][c] = g[k][c]; gvo[k][c] = gv[k][c];
                    ok = ok && isfinite(g[k][c]) && isfinite(gv[k][c]) && gv[k][c] >= 0.0;
                }
            }
        }
        double Np = 1.0, hd = 0.0, hc = 0.0;
        gd::D3 hn = gd::mk(0.0, 0.0, 0.0);
        const double cov = ok ? a.feat[7 * plane + p] : 0.0;
        if (!ok) { Np = 0.0; Ngp = 0.0; n_left += 1.0; }
        else if (!(cov > 0.0)) n_bg += 1.0;
        else {
            hd = a.feat[6 * plane + p] / cov; hc = cov;
            hn = gd::normalize(gd::mk(a.feat[3 * plane + p], a.feat[4 * plane + p], a.feat[5 * plane + p]));
            History h;
            GradHistory gh;
            const bool facing = hn.x != 0.0 || hn.y != 0.0 || hn.z != 0.0;
            if (a.first || !facing || !gather<kGrad>(a, ga, x, y, hd, hn, h, gh)) n_reset += 1.0;
            else {
                if constexpr (kGrad) {
                    double J[4];
                    if (ga.stale || !jacobian(a, ga, x, y, hd, hn, gh, J)) n_greset += 1.0;
                    else {
                        Ngp = fmin(gh.N + 1.0, a.max_history);
                        if (Ngp > 1.0) {      // (N_g' = 1: the input's bits)
                            const double alpha = 1.0 / Ngp, keep = 1.0 - alpha;
#pragma unroll
                            for (int k = 0; k < 2; k++)
#pragma unroll
                                for (int c = 0; c < 3; c++) {
                                    const double Hk = J[2 * k] * gh.G[0][c] + J[2 * k + 1] * gh.G[1][c];
                                    const double VHk = (J[2 * k] * J[2 * k]) * gh.VG[0][c] + (J[2 * k + 1] * J[2 * k + 1]) * gh.VG[1][c];
                                    go[k][c] = Hk + alpha * (g[k][c] - Hk);
                                    gvo[k][c] = (keep * keep) * VHk + (alpha * alpha) * gv[k][c];
                                }
                        }
                    }
                }
                Np = fmin(h.N + 1.0, a.max_history);
                if (Np > 1.0) {       // (N' = 1: alpha = 1, the input's bits)
                    const double alpha = 1.0 / Np, keep = 1.0 - alpha;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        o[c] = h.U[c] + alpha * (u[c] - h.U[c]);
                        vo[c] = (keep * keep) * h.V[c] + (alpha * alpha) * v[c];
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a.out[3 * p + c] = o[c]; a.var_out[3 * p + c] = vo[c];
            a.nU[3 * p + c] = o[c]; a.nV[3 * p + c] = vo[c];
        }
        a.nN[p] = Np;
        if (a.len) a.len[p] = Np;
        a.nG[p] = hn.x; a.nG[plane + p] = hn.y; a.nG[2 * plane + p] = hn.z;
        a.nG[3 * plane + p] = hd; a.nG[4 * plane + p] = hc;
        n_len += Np;
        if constexpr (kGrad) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                ga.gx_out[3 * p + c] = go[0][c]; ga.gx_var_out[3 * p + c] = gvo[0][c];
                ga.gy_out[3 * p + c] = go[1][c]; ga.gy_var_out[3 * p + c] = gvo[1][c];
                double *hp = ga.nH + (size_t)kGradDoubles * p;
                hp[c] = go[0][c]; hp[3 + c] = go[1][c]; hp[6 + c] = gvo[0][c]; hp[9 + c] = gvo[1][c];
            }
            ga.nNg[p] = Ngp;
            if (ga.glen) ga.glen[p] = Ngp;
            n_glen += Ngp;
        }
    }
    film::leave_block_sum(a.partials, 0, n_left, red);
    film::leave_block_sum(a.partials, 1, n_bg, red);
    film::leave_block_sum(a.partials, 2, n_reset, red);
    film::leave_block_sum(a.partials, 3, n_len, red);
    if constexpr (kGrad) {
        film::leave_block_sum(a.partials, 4, n_greset, red);
        film::leave_block_sum(a.partials, 5, n_glen, red);
    }
}

} // namespace temporal

struct GdptTemporal {
    int width = 0, height = 0, device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;                               // held while a call uses the handle
    struct Set { gdpt::DeviceBuffer<double> U, V, N, G, H, Ng; } set[2];      // H, Ng: the gradient history, from the first gradient push on
    int cur = 0;                                 // the set that holds the history
    bool have = false;                           // a push has been made since create or reset
    bool have_grad = false;                      // and it was a gradient push: the set holds the gradient history too (else it is stale)
    double Mprev[16] = {}, org_prev[3] = {};
    gdpt::DeviceBuffer<double> partials, d_sums;
    gdpt::PinnedBuffer<double> h_sums;
    gdpt::Event ev[2];

    ~GdptTemporal() {                            // the members free themselves on the device, after what the stream still holds
        if (!partials) return;                   // (no push was made: nothing is on a device)
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
    }
};

namespace gdpt {

void temporal_check_params(const std::string &who, const GdptTemporalParams &p) {
    if (!std::isfinite(p.tau_z) || !(p.tau_z >= 0)) throw std::runtime_error(who + ": tau_z must be finite and >= 0");
    if (!(p.tau_n >= -1 && p.tau_n <= 1)) throw std::runtime_error(who + ": tau_n must be in [-1, 1]");
    if (!(p.s_min > 0 && p.s_min <= 1)) throw std::runtime_error(who + ": s_min must be in (0, 1]");
    if (p.max_history < 1) throw std::runtime_error(who + ": max_history must be >= 1");
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) throw std::runtime_error(who + ": temporal reserved must be 0");
}

void temporal_world_to_sample(const std::string &who, const GdptCamera &cam, double M[16]) {
    M4 s2c, c2w;
    for (int i = 0; i < 16; i++) {
        if (!std::isfinite(cam.sample_to_cam[i])) throw std::runtime_error(who + ": sample_to_cam has a non-finite entry");
        if (!std::isfinite(cam.cam_to_world[i])) throw std::runtime_error(who + ": cam_to_world has a non-finite entry");
        s2c.m[i / 4][i % 4] = cam.sample_to_cam[i]; c2w.m[i / 4][i % 4] = cam.cam_to_world[i];
    }
    const M4 is = inverse(s2c), ic = inverse(c2w), m = is * ic;
    bool zs = true, zc = true, fin = true;
    for (int i = 0; i < 16; i++) {
        zs = zs && is.m[i / 4][i % 4] == 0; zc = zc && ic.m[i / 4][i % 4] == 0;
        fin = fin && std::isfinite(m.m[i / 4][i % 4]);
    }
    if (zs) throw std::runtime_error(who + ": sample_to_cam is singular");
    if (zc) throw std::runtime_error(who + ": cam_to_world is singular");
    if (!fin) throw std::runtime_error(who + ": sample_to_cam, cam_to_world: the world-to-sample matrix is not finite");
    for (int i = 0; i < 16; i++) M[i] = m.m[i / 4][i % 4];
}

void temporal_check_grad_params(const std::string &who, const GdptTemporalGradParams &p) {
    if (!std::isfinite(p.j_max) || !(p.j_max >= 1)) throw std::runtime_error(who + ": j_max must be finite and >= 1");
    if (!(p.cos_min > 0 && p.cos_min <= 1)) throw std::runtime_error(who + ": cos_min must be in (0, 1]");
    for (int r : p.reserved) if (r != 0) throw std::runtime_error(who + ": temporal gradient reserved must be 0");
}

// one push: the plain kernel, or with io and gp the gradient kernel; stats or gstats (at most one) waits for the stream
static void temporal_launch(GdptTemporal *t, const GdptCamera &cam, const double *d_img, const double *d_var, const double *d_feat,
                            const GdptTemporalParams &p, double *d_out, double *d_var_out, double *d_len, const TemporalGradIO *io,
                            const GdptTemporalGradParams *gp, GdptTemporalStats *stats, GdptTemporalGradStats *gstats) {
    if (gstats) stats = &gstats->base;
    double M[16];
    temporal_world_to_sample("gdpt_temporal_push", cam, M);      // (checked by the caller: cannot throw here)
    std::lock_guard<std::mutex> lk(t->mu);
    ck(hipSetDevice(t->device), "hipSetDevice");
    const size_t pixels = (size_t)t->width * t->height;
    for (auto &s : t->set) {
        if (!s.U) s.U.alloc(3 * pixels, "hipMalloc(temporal history)");
        if (!s.V) s.V.alloc(3 * pixels, "hipMalloc(temporal history)");
        if (!s.N) s.N.alloc(pixels, "hipMalloc(temporal history)");
        if (!s.G) s.G.alloc(temporal::kGeomPlanes * pixels, "hipMalloc(temporal history)");
        if (io && !s.H) s.H.alloc(temporal::kGradDoubles * pixels, "hipMalloc(temporal gradient history)");
        if (io && !s.Ng) s.Ng.alloc(pixels, "hipMalloc(temporal gradient history)");
    }
    if (!t->partials) t->partials.alloc(temporal::kGradRuns * film::kMaxBlocks, "hipMalloc(temporal partials)");
    if (!t->d_sums) t->d_sums.alloc(temporal::kGradRuns, "hipMalloc(temporal sums)");
    if (!t->h_sums) t->h_sums.alloc(temporal::kGradRuns, "hipHostMalloc(temporal sums)");
    for (auto &e : t->ev) if (!e) e.create();

    temporal::Args a{};
    a.g = film::tile_grid(t->width, t->height, kNlmTile, kNlmTile);
    fill_camera(cam, &a.cam);
    for (int i = 0; i < 16; i++) a.Mprev[i] = t->Mprev[i];
    for (int k = 0; k < 3; k++) a.org_prev[k] = t->org_prev[k];
    a.tau_z = p.tau_z; a.tau_n = p.tau_n; a.s_min = p.s_min; a.max_history = (double)p.max_history;
    a.first = t->have ? 0 : 1;
    a.img = d_img; a.var = d_var; a.feat = d_feat;
    const GdptTemporal::Set &rd = t->set[t->cur], &wr = t->set[t->cur ^ 1];
    a.pU = rd.U; a.pV = rd.V; a.pN = rd.N; a.pG = rd.G;
    a.nU = wr.U; a.nV = wr.V; a.nN = wr.N; a.nG = wr.G;
    a.out = d_out; a.var_out = d_var_out; a.len = d_len;
    a.partials = t->partials;
    const hipStream_t stream = t->stream;
    if (stats) ck(hipEventRecord(t->ev[0], stream), "hipEventRecord");
    const int runs = io ? temporal::kGradRuns : temporal::kRuns;
    if (io) {
        temporal::GradArgs ga{};
        ga.j_max = gp->j_max; ga.cos_min = gp->cos_min;
        ga.stale = (t->have && t->have_grad) ? 0 : 1;
        ga.gx = io->gx; ga.gx_var = io->gx_var; ga.gy = io->gy; ga.gy_var = io->gy_var;
        ga.pH = rd.H; ga.pNg = rd.Ng; ga.nH = wr.H; ga.nNg = wr.Ng;
        ga.gx_out = io->gx_out; ga.gx_var_out = io->gx_var_out; ga.gy_out = io->gy_out; ga.gy_var_out = io->gy_var_out; ga.glen = io->glen;
        hipLaunchKernelGGL(temporal::push_kernel_t<temporal::GradArgs>, dim3(a.g.blocks), dim3(film::kBlock), 0, stream, a, ga);
    } else hipLaunchKernelGGL(temporal::push_kernel_t<>, dim3(a.g.blocks), dim3(film::kBlock), 0, stream, a);
    ck(hipGetLastError(), "temporal launch");
    // the handle's state follows the enqueue: later pushes on the stream are ordered behind this one
    t->cur ^= 1; t->have = true; t->have_grad = io != nullptr;
    for (int i = 0; i < 16; i++) t->Mprev[i] = M[i];
    for (int k = 0; k < 3; k++) t->org_prev[k] = a.cam.org[k];
    if (!stats) return;
    ck(hipEventRecord(t->ev[1], stream), "hipEventRecord");
    film::launch_finish_runs(a.g.blocks, runs, t->partials, t->d_sums, stream);
    ck(hipGetLastError(), "temporal reduction launch");
    ck(hipMemcpyAsync(t->h_sums, t->d_sums, runs * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(temporal sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(temporal)");
    *stats = GdptTemporalStats{};
    const double *s = t->h_sums.data();
    stats->pixels_left_out = (uint64_t)s[0]; stats->pixels_background = (uint64_t)s[1]; stats->pixels_reset = (uint64_t)s[2];
    stats->sum_history = s[3];
    { float ms = 0; ck(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]), "hipEventElapsedTime"); stats->push_ms = ms; }
    if (gstats) { gstats->pixels_gradient_reset = (uint64_t)s[4]; gstats->sum_gradient_history = s[5]; }
}

void temporal_push_launch(GdptTemporal *t, const GdptCamera &cam, const double *d_img, const double *d_var, const double *d_feat,
                          const GdptTemporalParams &p, double *d_out, double *d_var_out, double *d_len, GdptTemporalStats *stats) {
    temporal_launch(t, cam, d_img, d_var, d_feat, p, d_out, d_var_out, d_len, nullptr, nullptr, stats, nullptr);
}

void temporal_push_gradients_launch(GdptTemporal *t, const GdptCamera &cam, const double *d_img, const double *d_var, const double *d_feat,
                                    const TemporalGradIO &io, const GdptTemporalParams &p, const GdptTemporalGradParams &gp, double *d_out,
                                    double *d_var_out, double *d_len, GdptTemporalGradStats *stats) {
    temporal_launch(t, cam, d_img, d_var, d_feat, p, d_out, d_var_out, d_len, &io, &gp, nullptr, stats);
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// What both push entry points refuse; `who` names the caller. Returns the parameters in force.
GdptTemporalParams check_push(const std::string &who, const GdptTemporal *t, const GdptCamera *camera, const double *img, const double *var,
                              const double *feat, const GdptTemporalParams *params, const double *out, const double *var_out,
                              const double *len) {
    if (!t) throw std::runtime_error(who + ": handle is null");
    if (!camera) throw std::runtime_error(who + ": camera is null");
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!feat) throw std::runtime_error(who + ": feat is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (!var_out) throw std::runtime_error(who + ": var_out is null");
    if (out == img || out == var || out == feat) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out == img || var_out == var || var_out == feat || var_out == out) throw std::runtime_error(who + ": var_out must not alias an input or out");
    if (len && (len == img || len == var || len == feat || len == out || len == var_out))
        throw std::runtime_error(who + ": len must not alias an input or another output");
    if (camera->width != t->width) throw std::runtime_error(who + ": camera width differs from the handle's");
    if (camera->height != t->height) throw std::runtime_error(who + ": camera height differs from the handle's");
    double M[16];
    gdpt::temporal_world_to_sample(who, *camera, M);
    GdptTemporalParams p;
    if (params) p = *params;
    else gdpt_temporal_default_params(&p);
    gdpt::temporal_check_params(who, p);
    return p;
}

// What both gradient push entry points refuse beyond check_push; returns the gradient parameters in force.
GdptTemporalGradParams check_push_gradients(const std::string &who, const double *img, const double *var, const double *feat,
                                            const gdpt::TemporalGradIO &io, const GdptTemporalGradParams *grad_params, const double *out,
                                            const double *var_out, const double *len) {
    struct Named { const char *name; const double *p; };
    const Named in_new[4] = {{"gx", io.gx}, {"gx_var", io.gx_var}, {"gy", io.gy}, {"gy_var", io.gy_var}};
    const Named out_new[5] = {{"gx_out", io.gx_out}, {"gx_var_out", io.gx_var_out}, {"gy_out", io.gy_out}, {"gy_var_out", io.gy_var_out}, {"glen", io.glen}};
    for (const Named &n : in_new) if (!n.p) throw std::runtime_error(who + ": " + n.name + " is null");
    for (int i = 0; i < 4; i++) if (!out_new[i].p) throw std::runtime_error(who + ": " + out_new[i].name + " is null");
    const Named ins[7] = {{"img", img}, {"var", var}, {"feat", feat}, in_new[0], in_new[1], in_new[2], in_new[3]};
    const Named outs[8] = {{"out", out}, {"var_out", var_out}, {"len", len}, out_new[0], out_new[1], out_new[2], out_new[3], out_new[4]};
    for (int i = 0; i < 8; i++) {
        if (!outs[i].p) continue;     // (len, glen: nullable)
        for (const Named &n : ins) if (outs[i].p == n.p) throw std::runtime_error(who + ": " + outs[i].name + " must not alias an input");
        for (int j = 0; j < i; j++) if (outs[i].p == outs[j].p) throw std::runtime_error(who + ": " + outs[i].name + " must not alias another output");
    }
    GdptTemporalGradParams gp;
    if (grad_params) gp = *grad_params;
    else gdpt_temporal_default_grad_params(&gp);
    gdpt::temporal_check_grad_params(who, gp);
    return gp;
}

} // namespace

extern "C" {

void gdpt_temporal_default_grad_params(GdptTemporalGradParams *p) {
    if (!p) return;
    *p = GdptTemporalGradParams{};
    p->j_max = 4.0; p->cos_min = 0.02;
}

int gdpt_temporal_push_gradients_device(GdptTemporal *t, const GdptCamera *camera, const double *d_img, const double *d_var,
                                        const double *d_feat, const double *d_gx, const double *d_gx_var, const double *d_gy,
                                        const double *d_gy_var, const GdptTemporalParams *params, const GdptTemporalGradParams *grad_params,
                                        double *d_out, double *d_var_out, double *d_len, double *d_gx_out, double *d_gx_var_out,
                                        double *d_gy_out, double *d_gy_var_out, double *d_glen, GdptTemporalGradStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_push_gradients_device";
        const GdptTemporalParams p = check_push(who, t, camera, d_img, d_var, d_feat, params, d_out, d_var_out, d_len);
        const gdpt::TemporalGradIO io{d_gx, d_gx_var, d_gy, d_gy_var, d_gx_out, d_gx_var_out, d_gy_out, d_gy_var_out, d_glen};
        const GdptTemporalGradParams gp = check_push_gradients(who, d_img, d_var, d_feat, io, grad_params, d_out, d_var_out, d_len);
        need_a_device(who);
        gdpt::temporal_push_gradients_launch(t, *camera, d_img, d_var, d_feat, io, p, gp, d_out, d_var_out, d_len, stats);
    });
}

int gdpt_temporal_push_gradients(GdptTemporal *t, const GdptCamera *camera, const double *img, const double *var, const double *feat,
                                 const double *gx, const double *gx_var, const double *gy, const double *gy_var,
                                 const GdptTemporalParams *params, const GdptTemporalGradParams *grad_params, double *out, double *var_out,
                                 double *len, double *gx_out, double *gx_var_out, double *gy_out, double *gy_var_out, double *glen,
                                 GdptTemporalGradStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_push_gradients";
        const GdptTemporalParams p = check_push(who, t, camera, img, var, feat, params, out, var_out, len);
        const gdpt::TemporalGradIO host{gx, gx_var, gy, gy_var, gx_out, gx_var_out, gy_out, gy_var_out, glen};
        const GdptTemporalGradParams gp = check_push_gradients(who, img, var, feat, host, grad_params, out, var_out, len);
        need_a_device(who);
        ck(hipSetDevice(t->device), "hipSetDevice");
        const size_t pixels = (size_t)t->width * t->height, n = 3 * pixels;
        gdpt::Mirror m_img, m_var, m_feat, m_out, m_vout, m_len, m_in[4], m_o[4], m_glen;
        m_img.up(img, n); m_var.up(var, n); m_feat.up(feat, GDPT_FEATURE_CHANNELS * pixels);
        const double *ins[4] = {gx, gx_var, gy, gy_var};
        double *outs[4] = {gx_out, gx_var_out, gy_out, gy_var_out};
        for (int i = 0; i < 4; i++) { m_in[i].up(ins[i], n); m_o[i].make(outs[i], n); }
        m_out.make(out, n); m_vout.make(var_out, n); m_len.make(len, pixels); m_glen.make(glen, pixels);
        const gdpt::TemporalGradIO io{m_in[0].d, m_in[1].d, m_in[2].d, m_in[3].d, m_o[0].d, m_o[1].d, m_o[2].d, m_o[3].d, m_glen.d};
        gdpt::temporal_push_gradients_launch(t, *camera, m_img.d, m_var.d, m_feat.d, io, p, gp, m_out.d, m_vout.d, m_len.d, stats);
        ck(hipStreamSynchronize(t->stream), "hipStreamSynchronize(temporal)");
        m_out.down(out, n); m_vout.down(var_out, n); m_len.down(len, pixels); m_glen.down(glen, pixels);
        for (int i = 0; i < 4; i++) m_o[i].down(outs[i], n);
    });
}

void gdpt_temporal_default_params(GdptTemporalParams *p) {
    if (!p) return;
    *p = GdptTemporalParams{};
    p->tau_z = 0.05; p->tau_n = 0.9; p->s_min = 1e-3; p->max_history = 32;
}

int gdpt_temporal_create(int width, int height, int device, void *stream, GdptTemporal **out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_create";
        if (!out) throw std::runtime_error(who + ": out is null");
        if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
        if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
        if (device < 0) throw std::runtime_error(who + ": bad device index");
        // (no device call: the planes are allocated by the first push, which fails on a device that does not exist)
        std::unique_ptr<GdptTemporal> t(new GdptTemporal());
        t->width = width; t->height = height; t->device = device; t->stream = (hipStream_t)stream;
        *out = t.release();
    });
}

void gdpt_temporal_free(GdptTemporal *t) {
    if (!t) return;
    delete t;
}

int gdpt_temporal_reset(GdptTemporal *t) {
    return gdpt::guarded([&]() {
        if (!t) throw std::runtime_error("gdpt_temporal_reset: handle is null");
        std::lock_guard<std::mutex> lk(t->mu);
        t->have = false; t->have_grad = false;
    });
}

int gdpt_temporal_world_to_sample(const GdptCamera *camera, double M[16]) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_world_to_sample";
        if (!camera) throw std::runtime_error(who + ": camera is null");
        if (!M) throw std::runtime_error(who + ": M is null");
        gdpt::temporal_world_to_sample(who, *camera, M);
    });
}

int gdpt_temporal_push_device(GdptTemporal *t, const GdptCamera *camera, const double *d_img, const double *d_var, const double *d_feat,
                              const GdptTemporalParams *params, double *d_out, double *d_var_out, double *d_len, GdptTemporalStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_push_device";
        const GdptTemporalParams p = check_push(who, t, camera, d_img, d_var, d_feat, params, d_out, d_var_out, d_len);
        need_a_device(who);
        gdpt::temporal_push_launch(t, *camera, d_img, d_var, d_feat, p, d_out, d_var_out, d_len, stats);
    });
}

int gdpt_temporal_push(GdptTemporal *t, const GdptCamera *camera, const double *img, const double *var, const double *feat,
                       const GdptTemporalParams *params, double *out, double *var_out, double *len, GdptTemporalStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_temporal_push";
        const GdptTemporalParams p = check_push(who, t, camera, img, var, feat, params, out, var_out, len);
        need_a_device(who);
        ck(hipSetDevice(t->device), "hipSetDevice");
        const size_t pixels = (size_t)t->width * t->height;
        gdpt::Mirror m_img, m_var, m_feat, m_out, m_vout, m_len;
        m_img.up(img, 3 * pixels); m_var.up(var, 3 * pixels); m_feat.up(feat, GDPT_FEATURE_CHANNELS * pixels);
        m_out.make(out, 3 * pixels); m_vout.make(var_out, 3 * pixels); m_len.make(len, pixels);
        gdpt::temporal_push_launch(t, *camera, m_img.d, m_var.d, m_feat.d, p, m_out.d, m_vout.d, m_len.d, stats);
        ck(hipStreamSynchronize(t->stream), "hipStreamSynchronize(temporal)");
        m_out.down(out, 3 * pixels); m_vout.down(var_out, 3 * pixels); m_len.down(len, pixels);
    });
}

} // extern "C"
