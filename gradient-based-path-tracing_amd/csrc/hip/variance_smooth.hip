// variance_smooth.hip — the box mean of a film's per-pixel variance of the mean, for gfx950 (include/gdpt.h: gdpt_variance_smooth*,
// where the definition stands). A session estimates that variance from K pass means, with K - 1 degrees of freedom; the non-local-means
// filters (denoise_nlm.hip) take their weights from it, and run unchanged on what this pre-pass writes.
//
// Kernel: smooth_kernel, a template on DEMOD (whether an effective albedo a~ is divided out before the mean and multiplied back
// after it). Blocks loop over 16 x 16 tiles as the filters' kernels do, a thread on a pixel of the tile, and leave block partials
// through leave_block_sum for finish_kernel (image_kernels.h): a fixed order, the same bits every time.
//   stage   the tile with a halo of `radius` pixels, plane by plane: three planes of doubles n_c = v_c / a~_c^2 and a plane of int
//           validity flags; out-of-film and invalid entries are 0 / 0. (16 + 2s) rows of pitch 16 (s = 0) or 48.
//   rows    sums of 2s + 1 taps in increasing x for the 16 columns of every staged row, into three planes of doubles and a plane of
//           int counts, (16 + 2s) rows of pitch 16. At most 24 x 16 = 384 outputs a plane: a thread takes at most two.
//   columns each thread sums 2s + 1 row sums of its own column in increasing y, divides by the count and multiplies its own a~_c^2
//           back (recomputed from the planar planes, as finish_pixel of denoise_nlm.hip does).
// LDS is sized by the call's radius: 14 336 bytes at s = 0, 43 008 at s = 4.
// LDS banking: every plane is a plane of doubles or of ints, so consecutive lanes read consecutive elements in both passes. In the
// row pass a half-wave covers two rows of 16 outputs; the stage's pitch of 48 doubles, = 16 mod 32, puts the second row's 16 doubles
// on the other half of the 64 banks for every tap (the pitch 16 + 2s itself would overlap them by 2s doubles). In the column pass a
// half-wave reads 32 consecutive doubles of the row sums (pitch 16). The staging stores walk the stage row by row, (16 + 2s) points a
// row: a group of 16 lanes that wraps from one row to the next stores two-way on part of the banks, once per staged point and plane.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "variance_smooth.h"

#include <cmath>
#include <mutex>
#include <type_traits>

namespace vsm {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, leave_block_sum

constexpr int kTile = gdpt::kVarSmoothTile;
constexpr int kMaxS = GDPT_VAR_SMOOTH_MAX_RADIUS;
static_assert(kTile * kTile == kBlock, "one thread per tile pixel");
static_assert((kTile + 2 * kMaxS) * kTile <= 2 * kBlock, "a thread computes at most two row sums per plane");

struct Args {
    static constexpr bool kDemod = false;
    TileGrid g;                  // 16 x 16 tiles
    int s;
    const double *img, *var;
    double *var_out;
    double *partials;            // [0] sum var in, [1] sum var out, [2] pixels left out; gridDim.x doubles each
};
// the divisor of a call with a demod block (denoise_nlm.hip's): planes `feat`, `fvar` of `plane` doubles each; the albedo is planes
// albedo .. albedo + 2, the coverage plane `coverage` (< 0: none)
struct Demod {
    const double *feat, *fvar;
    size_t plane;
    int albedo, coverage;
    double floor;
};
struct DemodArgs : Args {
    static constexpr bool kDemod = true;
    Demod dm;
};
template <bool DEMOD>
using ArgsOf = typename std::conditional<DEMOD, DemodArgs, Args>::type;

// pitch of the stage for rows of 16 + 2s points
__host__ __device__ inline int stage_pitch(int s) { return s == 0 ? kTile : 48; }
// doubles, then ints, of the kernel's LDS
__host__ __device__ inline int lds_doubles(int s) { return 3 * (stage_pitch(s) + kTile) * (kTile + 2 * s); }
__host__ __device__ inline int lds_ints(int s) { return (stage_pitch(s) + kTile) * (kTile + 2 * s); }

// a~_c^2 of pixel p (film index y w + x), in the operations of include/gdpt.h; returns whether its albedo and coverage values are valid
__device__ __forceinline__ bool albedo_squared(const Demod &dm, size_t p, double al2[3]) {
    bool ok = true;
    double miss = 0.0;               // 1 - cov; without a coverage plane cov = 1
    if (dm.coverage >= 0) {
        const double cov = dm.feat[dm.coverage * dm.plane + p], sc = dm.fvar[dm.coverage * dm.plane + p];
        ok = isfinite(cov) && isfinite(sc) && sc >= 0.0;
        miss = 1.0 - cov;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double g = dm.feat[(dm.albedo + c) * dm.plane + p], sg = dm.fvar[(dm.albedo + c) * dm.plane + p];
        ok = ok && isfinite(g) && isfinite(sg) && sg >= 0.0;
        const double al = fmax(dm.floor, g + miss);
        al2[c] = al * al;
    }
    return ok;
}

// n_c of film pixel (x, y), which is inside the film; returns whether it is valid (n is not to be used otherwise)
template <class A>
__device__ __forceinline__ bool load_pixel(const A &a, int x, int y, double n[3]) {
    const size_t p = (size_t)y * a.g.w + x;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double u = a.img[3 * p + c];
        n[c] = a.var[3 * p + c];
        ok = ok && isfinite(u) && isfinite(n[c]) && n[c] >= 0.0;
    }
    if constexpr (A::kDemod) {
        double al2[3];
        const bool oka = albedo_squared(a.dm, p, al2);
        ok = ok && oka;
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = n[c] / al2[c];
    }
    return ok;
}

template <bool DEMOD>
__global__ __launch_bounds__(kBlock) void smooth_kernel(ArgsOf<DEMOD> a) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    const int s = a.s, taps = 2 * s + 1;
    const int sw = kTile + 2 * s, sp = stage_pitch(s), sn = sp * sw;      // the stage: sw rows of sw points, pitch sp
    const int hn = kTile * sw;                                           // the row sums: sw rows of 16
    double *const pn = lds;                             // plane c at pn + c sn
    double *const ph = lds + 3 * sn;                    // plane c at ph + c hn
    int *const sflag = (int *)(ph + 3 * hn);
    int *const ch = sflag + sn;
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
    const int pc = (ly + s) * sp + lx + s;              // the thread's own pixel in the stage
    double var_in = 0.0, var_sum = 0.0, left_out = 0.0;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage and row sums have been read
        for (int k = tid; k < sw * sw; k += kBlock) {
            const int ry = k / sw, rx = k - ry * sw;
            const int gx = tp.x0 - s + rx, gy = tp.y0 - s + ry;
            double n[3] = {0.0, 0.0, 0.0};
            bool ok = false;
            if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) ok = load_pixel(a, gx, gy, n);
            const int j = ry * sp + rx;
#pragma unroll
            for (int c = 0; c < 3; c++) pn[c * sn + j] = ok ? n[c] : 0.0;
            sflag[j] = ok ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int q = tid + k * kBlock;             // row q / 16 of the stage, column q % 16 of the tile
            if (q >= hn) continue;
            const int j = (q / kTile) * sp + (q & (kTile - 1));
            double S[3] = {0.0, 0.0, 0.0};
            int C = 0;
            for (int m = 0; m < taps; m++) {
#pragma unroll
                for (int c = 0; c < 3; c++) S[c] += pn[c * sn + j + m];
                C += sflag[j + m];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) ph[c * hn + q] = S[c];
            ch[q] = C;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t p = (size_t)y * a.g.w + x;
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = a.var[3 * p + c];
        if (sflag[pc] == 0) {                           // kept as it came
#pragma unroll
            for (int c = 0; c < 3; c++) a.var_out[3 * p + c] = v[c];
            left_out += 1.0;
            continue;
        }
        double S[3] = {0.0, 0.0, 0.0};
        int C = 0;
        for (int m = 0; m < taps; m++) {
#pragma unroll
            for (int c = 0; c < 3; c++) S[c] += ph[c * hn + tid + m * kTile];
            C += ch[tid + m * kTile];
        }
        double o[3];                                    // (C >= 1: the pixel itself counts)
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = S[c] / (double)C;
        if constexpr (DEMOD) {
            double al2[3];
            albedo_squared(a.dm, p, al2);
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = o[c] * al2[c];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) a.var_out[3 * p + c] = o[c];
        var_in += (v[0] + v[1]) + v[2];
        var_sum += (o[0] + o[1]) + o[2];
    }
    leave_block_sum(a.partials, 0, var_in, red);
    leave_block_sum(a.partials, 1, var_sum, red);
    leave_block_sum(a.partials, 2, left_out, red);
}

} // namespace vsm

namespace gdpt {

namespace {

struct SmoothWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;
    DeviceBuffer<film::Estimate> d_est;     // sum var in, sum var out, left out
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<SmoothWorkspace> &g_workspaces = *new PerStream<SmoothWorkspace>();

template <bool DEMOD>
void launch_kernel(const vsm::ArgsOf<DEMOD> &a, hipStream_t stream) {
    const size_t lds = (size_t)vsm::lds_doubles(a.s) * sizeof(double) + (size_t)vsm::lds_ints(a.s) * sizeof(int);
    hipLaunchKernelGGL((vsm::smooth_kernel<DEMOD>), dim3(a.g.blocks), dim3(film::kBlock), lds, stream, a);
}

} // namespace

void var_smooth_check_params(const std::string &who, const GdptVarSmoothParams &p) {
    if (p.radius < 0 || p.radius > vsm::kMaxS) throw std::runtime_error(who + ": radius must be in [0, " + std::to_string(vsm::kMaxS) + "]");
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) throw std::runtime_error(who + ": smooth reserved must be 0");
}

void variance_smooth_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                            const GdptVarSmoothParams &p, const GdptNlmDemod *demod, double *d_var_out, hipStream_t stream,
                            GdptVarSmoothStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    SmoothWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    if (!ws.partials) ws.partials.alloc(3 * film::kMaxBlocks, "hipMalloc(variance smooth partials)");
    if (!ws.d_est) ws.d_est.alloc(1, "hipMalloc(variance smooth sums)");
    if (!ws.h_est) ws.h_est.alloc(1, "hipHostMalloc(variance smooth sums)");
    for (auto &e : ws.ev) if (!e) e.create();

    vsm::DemodArgs a{};
    a.g = film::tile_grid(w, h, kVarSmoothTile, kVarSmoothTile); a.s = p.radius;
    a.img = d_img; a.var = d_var; a.var_out = d_var_out; a.partials = ws.partials;
    const int nb = a.g.blocks;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    if (demod) {
        a.dm = vsm::Demod{d_feat, d_feat_var, (size_t)w * h, demod->albedo_channel, demod->coverage_channel, demod->floor};
        launch_kernel<true>(a, stream);
    } else launch_kernel<false>(static_cast<const vsm::Args &>(a), stream);
    ck(hipGetLastError(), "variance smooth launch");
    if (!stats) return;
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    ck(hipGetLastError(), "variance smooth reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(variance smooth sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(variance smooth)");
    *stats = GdptVarSmoothStats{};
    const film::Estimate &est = ws.h_est.data()[0];
    stats->pixels_left_out = (uint64_t)est.left_out;
    stats->sum_var_in = est.sum_var; stats->sum_var_out = est.sum_mean2;
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->smooth_ms = ms; }
    stats->radius = p.radius;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// what both entry points refuse; `who` names the caller. Returns the parameters in force.
GdptVarSmoothParams check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                    const double *feat_var, int num_channels, const GdptVarSmoothParams *params, const GdptNlmDemod *demod,
                                    const double *var_out) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!var_out) throw std::runtime_error(who + ": var_out is null");
    if (var_out == img || var_out == var || (feat && var_out == feat) || (feat_var && var_out == feat_var))
        throw std::runtime_error(who + ": var_out must not alias an input");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    GdptVarSmoothParams p;
    if (params) p = *params;
    else gdpt_var_smooth_default_params(&p);
    gdpt::var_smooth_check_params(who, p);
    if (demod) {
        if (!feat) throw std::runtime_error(who + ": feat is null (a demod block needs its planes)");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null (a demod block needs its planes)");
        gdpt::nlm_check_demod(who, *demod, num_channels);
    } else if (feat || feat_var) throw std::runtime_error(who + ": demod is null (feature planes need a demod block)");
    return p;
}

} // namespace

extern "C" {

void gdpt_var_smooth_default_params(GdptVarSmoothParams *p) {
    if (!p) return;
    *p = GdptVarSmoothParams{};
    p->radius = 2;
}

int gdpt_variance_smooth_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                int num_channels, const GdptVarSmoothParams *params, const GdptNlmDemod *demod, double *d_var_out, void *stream,
                                GdptVarSmoothStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_variance_smooth_device";
        const GdptVarSmoothParams p = check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, num_channels, params, demod, d_var_out);
        need_a_device(who);
        gdpt::variance_smooth_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, demod, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_variance_smooth(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int num_channels,
                         const GdptVarSmoothParams *params, const GdptNlmDemod *demod, double *var_out, GdptVarSmoothStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_variance_smooth";
        const GdptVarSmoothParams p = check_arguments(who, width, height, img, var, feat, feat_var, num_channels, params, demod, var_out);
        need_a_device(who);
        const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
        const size_t felems = demod ? (size_t)width * height * num_channels : 0, fbytes = felems * sizeof(double);
        gdpt::DeviceBuffer<double> d_img, d_var, d_var_out, d_feat, d_feat_var;
        d_img.alloc(elems, "hipMalloc(variance smooth io)"); d_var.alloc(elems, "hipMalloc(variance smooth io)");
        d_var_out.alloc(elems, "hipMalloc(variance smooth io)");
        d_feat.alloc(felems, "hipMalloc(variance smooth features)"); d_feat_var.alloc(felems, "hipMalloc(variance smooth features)");
        ck(hipMemcpy(d_img, img, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        if (felems) {
            ck(hipMemcpy(d_feat, feat, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            ck(hipMemcpy(d_feat_var, feat_var, fbytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        }
        gdpt::variance_smooth_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, demod, d_var_out, nullptr, stats);
        ck(hipMemcpy(var_out, d_var_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
