// recon_spread.hip — how far N independent estimates of one film lie apart, for gfx950 (include/gdpt.h: gdpt_recon_spread*).
//
// Definition. Images f_1..f_N with weights W_i > 0 (the samples per pixel behind each). Per component, West's weighted update in
// member order, the arithmetic of fold_kernel (progressive.hip) with an image in the place of a pass and W_i in the place of n:
//     W += W_i;  d = f_i - mean;  mean += (W_i / W) d;  M2 += W_i d (f_i - mean_new)
// leaves mean = sum W_i f_i / W and M2 = sum W_i (f_i - mean)^2, and var = M2 / ((N - 1) W) estimates the variance of the mean when
// every f_i has variance sigma^2 / W_i. The film sums are sum var and sum f_tot^2 over the pixels whose members' triples, f_tot
// triple and var triple are all finite; the others are counted. The map is var summed over the three channels, per pixel.
//
// Kernels.
//   spread_kernel   a thread owns a PIXEL (consecutive threads on consecutive 24-byte triples, as fold_kernel): the running
//                   (mean, M2) of its three channels stay in registers while the N images stream by; the image pointers and
//                   weights come by value in the kernel arguments. Memory bound: (N + 1) x 24 bytes read, 32 written per pixel.
//                   Block partials through leave_block_sum, then finish_kernel (image_kernels.h): a fixed order, the same bits every time.
//   box_kernel      the map's window mean for radius r >= 1: 32 x 8 pixel tiles with an r-wide halo staged in LDS (48 x 24 doubles
//                   at r = 8), staged as pcg_step_a stages its tile; a finite count travels beside every sum; separable inside the
//                   tile: row sums of 2r + 1 taps, then column sums of the row sums. Out-of-film and non-finite entries count 0.
//                   LDS banking: a half-wave is one tile row, and its 32 lanes read 32 consecutive doubles (256 bytes, every bank of
//                   the 64-dword bank row once) in both passes, whatever the pitch: no padding is needed for the 8-byte reads.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "recon_spread.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

namespace rsp {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, leave_block_sum

constexpr int kMaxN = GDPT_MULTI_MAX_DEVICES, kMaxRadius = 8;
constexpr int kTileW = gdpt::kSpreadTileW, kTileH = gdpt::kSpreadTileH;
constexpr int kStageW = kTileW + 2 * kMaxRadius, kStageH = kTileH + 2 * kMaxRadius;      // 48 x 24
static_assert(kTileW * kTileH == kBlock, "one thread per tile pixel");

// frac[i] = W_i / (W_1 + .. + W_i), as fold_kernel's n / w_new
struct Members {
    const double *img[kMaxN];
    double w[kMaxN], frac[kMaxN];
};

// norm = (N - 1) W. total == nullptr: the mean is the total. var (3 npix) and pixsum (npix) are optional.
// partials: [0] sum var, [1] sum total^2, [2] pixels left out; gridDim.x doubles each.
__global__ __launch_bounds__(kBlock) void spread_kernel(Members m, int n, int npix, double norm, const double *total, double *var,
                                                        double *pixsum, double *partials) {
    __shared__ double red[kBlock / 64];
    double s_var = 0, s_sq = 0, s_out = 0;
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < npix; pix += gridDim.x * kBlock) {
        const size_t i = (size_t)3 * pix;
        double mu[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
        bool ok = true;
        for (int k = 0; k < n; k++) {
            const double *f = m.img[k];
            const double wk = m.w[k], fr = m.frac[k];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double x = f[i + c];
                ok = ok && isfinite(x);
                const double d = x - mu[c];
                mu[c] = mu[c] + fr * d;
                q[c] = q[c] + wk * d * (x - mu[c]);
            }
        }
        double v[3], t[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[c] = q[c] / norm;
            t[c] = total ? total[i + c] : mu[c];
            ok = ok && isfinite(v[c]) && isfinite(t[c]);
        }
        const double sum = (v[0] + v[1]) + v[2];
        if (var) {
#pragma unroll
            for (int c = 0; c < 3; c++) var[i + c] = v[c];
        }
        if (pixsum) pixsum[pix] = sum;
        if (ok) {
            s_var += sum;
            s_sq += (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
        } else s_out += 1.0;
    }
    leave_block_sum(partials, 0, s_var, red);
    leave_block_sum(partials, 1, s_sq, red);
    leave_block_sum(partials, 2, s_out, red);
}

// out(x, y) = mean of the finite entries of `in` in the window [x - r, x + r] x [y - r, y + r] clipped to the film; NaN without one.
// 1 <= r <= kMaxRadius.
__global__ __launch_bounds__(kBlock) void box_kernel(TileGrid g, int r, const double *in, double *out) {
    __shared__ double sv[kStageH][kStageW];      // the tile and its halo: the value, 0 where it does not count
    __shared__ int sc[kStageH][kStageW];         // ... 1 where it counts
    __shared__ double hv[kStageH][kTileW];       // row sums of 2r + 1 taps
    __shared__ int hc[kStageH][kTileW];
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    const int sw = kTileW + 2 * r, sh = kTileH + 2 * r, taps = 2 * r + 1;
    const int w = g.w, h = g.h;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTileW, kTileH>(g, t);
        const int x0 = tp.x0, y0 = tp.y0;
        __syncthreads();                                   // the previous tile's sums have been read
        for (int k = threadIdx.x; k < sw * sh; k += kBlock) {
            const int ry = k / sw, rx = k - ry * sw;
            const int gx = x0 - r + rx, gy = y0 - r + ry;
            double val = 0.0;
            int cnt = 0;
            if (gx >= 0 && gy >= 0 && gx < w && gy < h) {
                const double a = in[gy * w + gx];
                if (isfinite(a)) { val = a; cnt = 1; }
            }
            sv[ry][rx] = val; sc[ry][rx] = cnt;
        }
        __syncthreads();
        for (int row = ly; row < sh; row += kTileH) {
            double s = 0.0;
            int c = 0;
            for (int k = 0; k < taps; k++) { s += sv[row][lx + k]; c += sc[row][lx + k]; }
            hv[row][lx] = s; hc[row][lx] = c;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        if (x < w && y < h) {
            double s = 0.0;
            int c = 0;
            for (int k = 0; k < taps; k++) { s += hv[ly + k][lx]; c += hc[ly + k][lx]; }
            out[y * w + x] = c > 0 ? s / (double)c : __builtin_nan("");
        }
    }
}

} // namespace rsp

namespace gdpt {

namespace {

struct SpreadWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials, pixsum;
    DeviceBuffer<film::Estimate> d_est;
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
};

// leaked on purpose: no HIP call is made from a static destructor (as the solver's registry, poisson_kernels.hip); a pair's entry
// goes with forget_stream (device_mem.h)
PerStream<SpreadWorkspace> &g_workspaces = *new PerStream<SpreadWorkspace>();

} // namespace

ReconSpreadResult recon_spread_device(int w, int h, int n, const double *const *d_images, const double *weights, const double *d_total,
                                      int radius, double *d_var, double *d_map, hipStream_t stream) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    SpreadWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    const int npix = w * h;
    if (!ws.partials) ws.partials.alloc(3 * film::kMaxBlocks, "hipMalloc(spread partials)");
    if (!ws.d_est) ws.d_est.alloc(1, "hipMalloc(spread sums)");
    if (!ws.h_est) ws.h_est.alloc(1, "hipHostMalloc(spread sums)");
    for (auto &e : ws.ev) if (!e) e.create();
    const bool windowed = d_map && radius >= 1;
    if (windowed) ws.pixsum.grow((size_t)npix, stream, "hipMalloc(spread map)");

    rsp::Members m{};
    double wsum = 0;
    for (int i = 0; i < n; i++) {
        wsum += weights[i];
        m.img[i] = d_images[i]; m.w[i] = weights[i]; m.frac[i] = weights[i] / wsum;
    }
    const double norm = (double)(n - 1) * wsum;
    const int nb = film::stride_grid((size_t)npix, film::kMaxBlocks, 1).blocks;
    ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    hipLaunchKernelGGL(rsp::spread_kernel, dim3(nb), dim3(film::kBlock), 0, stream, m, n, npix, norm, d_total, d_var,
                       windowed ? ws.pixsum.data() : d_map, ws.partials.data());
    ck(hipGetLastError(), "spread launch");
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    ck(hipGetLastError(), "spread reduction launch");
    if (windowed) {
        const film::TileGrid bg = film::tile_grid(w, h, kSpreadTileW, kSpreadTileH);
        hipLaunchKernelGGL(rsp::box_kernel, dim3(bg.blocks), dim3(film::kBlock), 0, stream, bg, radius, ws.pixsum.data(), d_map);
        ck(hipGetLastError(), "spread window launch");
    }
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(spread sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(spread)");
    ReconSpreadResult res;
    res.sum_var = ws.h_est->sum_var; res.sum_sq = ws.h_est->sum_mean2; res.left_out = ws.h_est->left_out;
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); res.ms = ms; }
    return res;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// what both entry points refuse; `who` names the caller
void check_arguments(const std::string &who, int width, int height, int n, const double *const *images, const double *weights, const double *total,
                     int radius, const double *var, const double *map) {
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": film too large");
    if (n < 2 || n > GDPT_MULTI_MAX_DEVICES)
        throw std::runtime_error(who + ": the number of images must be in [2, " + std::to_string(GDPT_MULTI_MAX_DEVICES) + "] (one image has no spread)");
    if (radius < 0 || radius > rsp::kMaxRadius) throw std::runtime_error(who + ": radius must be in [0, " + std::to_string(rsp::kMaxRadius) + "]");
    if (!images || !weights) throw std::runtime_error(who + ": null images or weights");
    for (int i = 0; i < n; i++) {
        if (!images[i]) throw std::runtime_error(who + ": image " + std::to_string(i) + " is null");
        if (!(weights[i] > 0) || !std::isfinite(weights[i])) throw std::runtime_error(who + ": weight " + std::to_string(i) + " must be finite and > 0");
    }
    for (const double *out : {var, map}) {
        if (!out) continue;
        bool alias = out == total || (var && var == map);
        for (int i = 0; i < n; i++) alias = alias || out == images[i];
        if (alias) throw std::runtime_error(who + ": an output must not alias an input or the other output");
    }
}

} // namespace

namespace gdpt {

void fill_spread_stats(GdptReconSpreadStats *st, int n, int radius, const ReconSpreadResult &r) {
    if (!st) return;
    *st = GdptReconSpreadStats{};
    st->members = n; st->radius = radius;
    st->sum_var = r.sum_var; st->sum_sq = r.sum_sq;
    st->error_estimate = std::sqrt(r.sum_var / r.sum_sq);
    st->pixels_left_out = (uint64_t)r.left_out;
    st->spread_ms = r.ms;
}

} // namespace gdpt

extern "C" {

int gdpt_recon_spread_device(int width, int height, int n, const double *const *d_images, const double *weights, const double *d_total,
                             int radius, double *d_var, double *d_map, void *stream, GdptReconSpreadStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_recon_spread_device";
        check_arguments(who, width, height, n, d_images, weights, d_total, radius, d_var, d_map);
        need_a_device(who);
        gdpt::fill_spread_stats(stats, n, radius, gdpt::recon_spread_device(width, height, n, d_images, weights, d_total, radius, d_var, d_map, (hipStream_t)stream));
    });
}

int gdpt_recon_spread(int width, int height, int n, const double *const *images, const double *weights, const double *total, int radius,
                      double *var, double *map, GdptReconSpreadStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_recon_spread";
        check_arguments(who, width, height, n, images, weights, total, radius, var, map);
        need_a_device(who);
        const size_t npix = (size_t)width * height, elems = 3 * npix;
        std::vector<gdpt::DeviceBuffer<double>> d_in((size_t)n + 1);
        gdpt::DeviceBuffer<double> d_var, d_map;
        std::vector<const double *> ptrs((size_t)n);
        for (int i = 0; i <= n; i++) {
            const double *src = i < n ? images[i] : total;
            if (!src) continue;
            d_in[(size_t)i].alloc(elems, "hipMalloc(spread io)");
            ck(hipMemcpy(d_in[(size_t)i], src, elems * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            if (i < n) ptrs[(size_t)i] = d_in[(size_t)i];
        }
        if (var) d_var.alloc(elems, "hipMalloc(spread io)");
        if (map) d_map.alloc(npix, "hipMalloc(spread io)");
        gdpt::fill_spread_stats(stats, n, radius, gdpt::recon_spread_device(width, height, n, ptrs.data(), weights, d_in[(size_t)n], radius, d_var, d_map, nullptr));
        if (var) ck(hipMemcpy(var, d_var, elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (map) ck(hipMemcpy(map, d_map, npix * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
