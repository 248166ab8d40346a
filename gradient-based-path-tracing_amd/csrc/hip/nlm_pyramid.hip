// nlm_pyramid.hip — the multi-scale (pyramid) form of the non-local-means filters, for gfx950 (include/gdpt.h: gdpt_nlm_pyramid_down*,
// gdpt_nlm_pyramid_up*, gdpt_denoise_nlm_multiscale*, where the definition stands). The filters of denoise_nlm.hip run unchanged on
// every level; the two kernels here make the next level (down) and put a filtered coarser level back into a filtered finer one (up).
//
// Kernels: templates on KIND, which decides what makes a pixel valid (valid_pixel restates the predicates of denoise_nlm.hip:
// valid_triples, valid_features, the checks of effective_albedo). Blocks loop over 16 x 16 tiles as the filters' kernels do and leave
// block partials through leave_block_sum for finish_kernel (image_kernels.h): a fixed order, the same bits every time.
//   down_kernel  a thread on a pixel of a tile of the COARSE level: the validity of its (at most) four fine pixels, then every value
//                summed over the valid ones in the order (0,0), (1,0), (0,1), (1,1) and divided. No LDS but the reduction's.
//   up_kernel    a thread on a pixel of a tile of the FINE level. The tile's 8 x 8 coarse cells and a ring of one cell around them
//                (the taps X*, Y* of the tile's border pixels) are 10 x 10 cells, 20 x 20 fine pixels:
//     stage      F_l and the validity of those 400 pixels (0.0 and 0 outside the film and on invalid pixels), split by the pixel's
//                place (dx, dy) in its cell into four sub-planes of 10 x 10 cells, per channel
//     cells      R of the 100 cells and 3 channels from the four sub-planes and out_{l+1}, into LDS: 300 items over 256 threads
//     combine    each thread reads its own F_l and four R per channel and adds them, products and sums apart (no contraction).
// LDS: 3 x 4 sub-planes and 3 planes of R of 104 doubles, 4 sub-planes of 104 ints: 14 144 bytes, static (and the reduction's 32).
// LDS banking: a half-wave's 32 doubles are conflict-free when they fall on 32 distinct double-slots mod 32 (64 banks of 4 bytes). In
// the cells pass consecutive lanes take consecutive cells of one channel, so each of the four reads is 32 consecutive doubles of one
// sub-plane: that is why the stage is split by (dx, dy); kept as a 20 x 20 plane the four reads would have stride 2 and could reach
// only the 16 even slots. A sub-plane's pitch is 104 doubles, = 8 mod 32: in the combine pass a half-wave is two rows of 16 pixels,
// which read 8 consecutive cells of each of the four sub-planes of a channel, at 0, 8, 16 and 24 mod 32. The reads of R are at most 10
// consecutive doubles of one row of cells (X, X*; two lanes of a cell read one address), and for Y* of two rows 20 doubles apart.
// The staging stores walk the 20 x 20 pixels row by row for the sake of the global reads. A store of doubles is served in groups of
// 16 lanes over 32 banks: a group's 8 even and 8 odd pixels go to two sub-planes 104 doubles = 16 banks mod 32 apart, 16 banks each,
// which is conflict-free but for a group that wraps from one row of the stage (20 pixels) to the next.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_pyramid.h"
#include "nlm_host.h"

#include <cmath>
#include <initializer_list>
#include <mutex>
#include <string>

namespace pyr {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, leave_block_sum

constexpr int kTile = gdpt::kNlmPyramidTile;
constexpr int kMaxChannels = GDPT_NLM_MAX_CHANNELS;
constexpr int kCells = kTile / 2 + 2;              // cells a side of the stage: the tile's and a ring of one
constexpr int kStage = 2 * kCells;                 // fine pixels a side
constexpr int kSub = 104;                          // pitch of a sub-plane of kCells^2 cells: = 8 mod 32
static_assert(kTile * kTile == kBlock, "one thread per tile pixel");
static_assert(kSub >= kCells * kCells && kSub % 32 == 8, "four sub-planes a quarter of the banks apart");
static_assert(kMaxChannels <= 32, "Level::used holds a bit per channel");

// a level's arrays and what decides a pixel's validity there
struct Level {
    const double *img, *var, *feat, *fvar;
    size_t plane;                // w h
    unsigned used;               // bit c: some group of the guide names channel c
    int albedo, coverage;        // GDPT_DENOISE_DEMOD: the planes of the block (coverage < 0: none)
};

struct DownArgs {
    TileGrid g;                  // 16 x 16 tiles of the COARSE level
    int w, h, nc;                // the fine level; feature planes to carry (0: none)
    Level lv;
    double *img_out, *var_out, *feat_out, *fvar_out;
    double *partials;            // [0] invalid fine pixels, [1] coarse pixels with n = 0, [2] 0; gridDim.x doubles each
};

struct UpArgs {
    TileGrid g;                  // 16 x 16 tiles of the FINE level
    int wc, hc;                  // the coarse level
    Level lv;
    const double *filtered, *coarse;
    double *out;
    double *partials;            // [0] invalid fine pixels, [1] 0, [2] 0
};

// whether pixel p (film index y w + x) of the level is valid for the kind's filter
template <int KIND>
__device__ __forceinline__ bool valid_pixel(const Level &lv, size_t p) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double u = lv.img[3 * p + c], v = lv.var[3 * p + c];
        ok = ok && isfinite(u) && isfinite(v) && v >= 0.0;
    }
    if constexpr (KIND != GDPT_DENOISE_PLAIN) {
        for (unsigned m = lv.used; m != 0; m &= m - 1) {      // (wave-uniform; no register array is indexed by c, so nothing is unrolled)
            const int c = __ffs(m) - 1;
            const double g = lv.feat[c * lv.plane + p], s = lv.fvar[c * lv.plane + p];
            ok = ok && isfinite(g) && isfinite(s) && s >= 0.0;
        }
    }
    if constexpr (KIND == GDPT_DENOISE_DEMOD) {
        if (lv.coverage >= 0) {
            const double cov = lv.feat[lv.coverage * lv.plane + p], sc = lv.fvar[lv.coverage * lv.plane + p];
            ok = ok && isfinite(cov) && isfinite(sc) && sc >= 0.0;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double g = lv.feat[(lv.albedo + c) * lv.plane + p], sg = lv.fvar[(lv.albedo + c) * lv.plane + p];
            ok = ok && isfinite(g) && isfinite(sg) && sg >= 0.0;
        }
    }
    return ok;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void down_kernel(DownArgs a) {
    __shared__ double red[kBlock / 64];
    const size_t cplane = (size_t)a.g.w * a.g.h;
    const double nan = __builtin_nan("");
    double left_out = 0.0, empty = 0.0;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int X = tp.x, Y = tp.y;
        if (X >= a.g.w || Y >= a.g.h) continue;
        size_t p[4];
        bool ok[4];
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {                   // (dx, dy) = (0,0), (1,0), (0,1), (1,1)
            const int x = 2 * X + (k & 1), y = 2 * Y + (k >> 1);
            const bool in = x < a.w && y < a.h;
            p[k] = in ? (size_t)y * a.w + x : 0;
            ok[k] = in && valid_pixel<KIND>(a.lv, p[k]);
            n += ok[k] ? 1 : 0;
            if (in && !ok[k]) left_out += 1.0;
        }
        const size_t q = (size_t)Y * a.g.w + X;
        const double dn = (double)n, dn2 = (double)(n * n);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (ok[k]) { su += a.lv.img[3 * p[k] + c]; sv += a.lv.var[3 * p[k] + c]; }
            a.img_out[3 * q + c] = n ? su / dn : nan;
            a.var_out[3 * q + c] = n ? sv / dn2 : nan;
        }
        for (int c = 0; c < a.nc; c++) {
            double sg = 0.0, ss = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (ok[k]) { sg += a.lv.feat[c * a.lv.plane + p[k]]; ss += a.lv.fvar[c * a.lv.plane + p[k]]; }
            a.feat_out[c * cplane + q] = n ? sg / dn : nan;
            a.fvar_out[c * cplane + q] = n ? ss / dn2 : nan;
        }
        if (n == 0) empty += 1.0;
    }
    leave_block_sum(a.partials, 0, left_out, red);
    leave_block_sum(a.partials, 1, empty, red);
    leave_block_sum(a.partials, 2, 0.0, red);
}

// F plus the interpolated correction, every product and sum rounded on its own, in the order of include/gdpt.h
__device__ __forceinline__ double combine(double F, double r00, double r10, double r01, double r11) {
#pragma clang fp contract(off)
    const double a = 0.5625 * r00, b = 0.1875 * r10, c = 0.1875 * r01, d = 0.0625 * r11;
    const double t = ((a + b) + c) + d;
    return F + t;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void up_kernel(UpArgs a) {
    __shared__ double sf[3 * 4 * kSub];                 // F_l: channel c, sub-plane s = 2 dy + dx, cell (cx, cy) at (4 c + s) kSub + cy kCells + cx
    __shared__ double sr[3 * kSub];                     // R: channel c, cell (cx, cy) at c kSub + cy kCells + cx
    __shared__ int sflag[4 * kSub];                     // validity, as one channel of sf
    __shared__ double red[kBlock / 64];
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
    const int own_cell = ((ly >> 1) + 1) * kCells + (lx >> 1) + 1, own_sub = (ly & 1) * 2 + (lx & 1);
    double left_out = 0.0;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int cx0 = tp.x0 / 2 - 1, cy0 = tp.y0 / 2 - 1;      // the stage's first cell (-1 at the film's left and top)
        __syncthreads();                                // the previous tile's stage and R have been read
        for (int k = tid; k < kStage * kStage; k += kBlock) {
            const int ry = k / kStage, rx = k - ry * kStage;
            const int gx = 2 * cx0 + rx, gy = 2 * cy0 + ry;
            double F[3] = {0.0, 0.0, 0.0};
            bool ok = false;
            if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) {
                const size_t p = (size_t)gy * a.g.w + gx;
                ok = valid_pixel<KIND>(a.lv, p);
                if (ok) {
#pragma unroll
                    for (int c = 0; c < 3; c++) F[c] = a.filtered[3 * p + c];
                }
            }
            const int j = ((ry & 1) * 2 + (rx & 1)) * kSub + (ry >> 1) * kCells + (rx >> 1);
#pragma unroll
            for (int c = 0; c < 3; c++) sf[c * 4 * kSub + j] = F[c];
            sflag[j] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int k = tid; k < 3 * kCells * kCells; k += kBlock) {
            const int c = k / (kCells * kCells), cell = k - c * (kCells * kCells);
            double s = 0.0;
            int n = 0;
#pragma unroll
            for (int sub = 0; sub < 4; sub++)           // (dx, dy) = (0,0), (1,0), (0,1), (1,1)
                if (sflag[sub * kSub + cell]) { s += sf[(4 * c + sub) * kSub + cell]; n++; }
            double R = 0.0;
            if (n > 0) {                                // (a valid fine pixel lies in the film, so its cell lies in the coarse film)
                const int cy = cell / kCells, cx = cell - cy * kCells;
                const size_t q = (size_t)(cy0 + cy) * a.wc + (cx0 + cx);
                R = a.coarse[3 * q + c] - s / (double)n;
            }
            sr[c * kSub + cell] = R;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t p = (size_t)y * a.g.w + x;
        if (sflag[own_sub * kSub + own_cell] == 0) {    // kept as it came
#pragma unroll
            for (int c = 0; c < 3; c++) a.out[3 * p + c] = a.lv.img[3 * p + c];
            left_out += 1.0;
            continue;
        }
        const int X = x >> 1, Y = y >> 1;
        const int Xs = min(max(X + ((x & 1) ? 1 : -1), 0), a.wc - 1), Ys = min(max(Y + ((y & 1) ? 1 : -1), 0), a.hc - 1);
        const int cx = X - cx0, cy = Y - cy0, cxs = Xs - cx0, cys = Ys - cy0;      // within [0, kCells): X, Y are the tile's own cells
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double *r = sr + c * kSub;
            a.out[3 * p + c] = combine(sf[(4 * c + own_sub) * kSub + own_cell], r[cy * kCells + cx], r[cy * kCells + cxs], r[cys * kCells + cx],
                                       r[cys * kCells + cxs]);
        }
    }
    leave_block_sum(a.partials, 0, left_out, red);
    leave_block_sum(a.partials, 1, 0.0, red);
    leave_block_sum(a.partials, 2, 0.0, red);
}

} // namespace pyr

namespace gdpt {

namespace {

// the scratch of one operator launch
struct OpWorkspace {
    std::mutex mu;                    // held while a down or an up runs on this (device, stream) pair
    DeviceBuffer<double> partials;
    DeviceBuffer<film::Estimate> d_est;     // invalid fine pixels, empty cells, 0
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];
};
// the pyramid of a multi-scale call: levels 1 .. of the inputs, every level's filtered mean, the combined outputs of the levels between
struct PyramidStorage {
    std::mutex mu;                    // held while a multi-scale call runs on this (device, stream) pair
    DeviceBuffer<double> img[GDPT_NLM_MAX_LEVELS], var[GDPT_NLM_MAX_LEVELS], feat[GDPT_NLM_MAX_LEVELS], fvar[GDPT_NLM_MAX_LEVELS];
    DeviceBuffer<double> filtered[GDPT_NLM_MAX_LEVELS], out[GDPT_NLM_MAX_LEVELS];
    Event ev[2];
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entries go with forget_stream (device_mem.h)
PerStream<OpWorkspace> &g_ops = *new PerStream<OpWorkspace>();
PerStream<PyramidStorage> &g_pyramids = *new PerStream<PyramidStorage>();

pyr::Level make_level(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, const NlmKindBlocks &kb) {
    pyr::Level lv{d_img, d_var, d_feat, d_feat_var, (size_t)w * h, 0u, 0, -1};
    if (kb.has_guide)
        for (int j = 0; j < kb.guide.num_groups; j++)
            for (int c = kb.guide.groups[j].first_channel; c < kb.guide.groups[j].first_channel + kb.guide.groups[j].num_channels; c++) lv.used |= 1u << c;
    if (kb.has_demod) { lv.albedo = kb.demod.albedo_channel; lv.coverage = kb.demod.coverage_channel; }
    return lv;
}

OpWorkspace &op_workspace(hipStream_t stream) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    return g_ops.get(dev, stream);
}
void prepare(OpWorkspace &ws) {
    if (!ws.partials) ws.partials.alloc(3 * film::kMaxBlocks, "hipMalloc(nlm pyramid partials)");
    if (!ws.d_est) ws.d_est.alloc(1, "hipMalloc(nlm pyramid sums)");
    if (!ws.h_est) ws.h_est.alloc(1, "hipHostMalloc(nlm pyramid sums)");
    for (auto &e : ws.ev) if (!e) e.create();
}
// the counts of a launch that has left its partials, after waiting for `stream`
void read_stats(OpWorkspace &ws, int nb, int wc, int hc, hipStream_t stream, GdptNlmPyramidOpStats *stats) {
    film::launch_finish(nb, ws.partials, ws.d_est, stream);
    ck(hipGetLastError(), "nlm pyramid reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_est, ws.d_est, sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(nlm pyramid sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm pyramid)");
    *stats = GdptNlmPyramidOpStats{};
    const film::Estimate &est = ws.h_est.data()[0];
    stats->pixels_left_out = (uint64_t)est.sum_var; stats->cells_empty = (uint64_t)est.sum_mean2;
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->op_ms = ms; }
    stats->coarse_width = wc; stats->coarse_height = hc;
}

// Device pointers on the current device; the arguments have been checked. Enqueued on `stream`; waits for it if `stats` is asked for.
void down_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, const NlmKindBlocks &kb,
                 double *d_img_out, double *d_var_out, double *d_feat_out, double *d_feat_var_out, hipStream_t stream, GdptNlmPyramidOpStats *stats) {
    OpWorkspace &ws = op_workspace(stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    prepare(ws);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2;
    pyr::DownArgs a{};
    a.g = film::tile_grid(wc, hc, kNlmPyramidTile, kNlmPyramidTile);
    a.w = w; a.h = h; a.nc = d_feat_out ? kb.num_channels : 0;
    a.lv = make_level(w, h, d_img, d_var, d_feat, d_feat_var, kb);
    a.img_out = d_img_out; a.var_out = d_var_out; a.feat_out = d_feat_out; a.fvar_out = d_feat_var_out; a.partials = ws.partials;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    const dim3 grid(a.g.blocks), block(film::kBlock);
    if (kb.kind == GDPT_DENOISE_DEMOD) hipLaunchKernelGGL((pyr::down_kernel<GDPT_DENOISE_DEMOD>), grid, block, 0, stream, a);
    else if (kb.kind == GDPT_DENOISE_GUIDED) hipLaunchKernelGGL((pyr::down_kernel<GDPT_DENOISE_GUIDED>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pyr::down_kernel<GDPT_DENOISE_PLAIN>), grid, block, 0, stream, a);
    ck(hipGetLastError(), "nlm pyramid down launch");
    if (stats) read_stats(ws, a.g.blocks, wc, hc, stream, stats);
}

void up_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, const NlmKindBlocks &kb,
               const double *d_filtered, const double *d_coarse_out, double *d_out, hipStream_t stream, GdptNlmPyramidOpStats *stats) {
    OpWorkspace &ws = op_workspace(stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    prepare(ws);
    pyr::UpArgs a{};
    a.g = film::tile_grid(w, h, kNlmPyramidTile, kNlmPyramidTile);
    a.wc = (w + 1) / 2; a.hc = (h + 1) / 2;
    a.lv = make_level(w, h, d_img, d_var, d_feat, d_feat_var, kb);
    a.filtered = d_filtered; a.coarse = d_coarse_out; a.out = d_out; a.partials = ws.partials;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    const dim3 grid(a.g.blocks), block(film::kBlock);
    if (kb.kind == GDPT_DENOISE_DEMOD) hipLaunchKernelGGL((pyr::up_kernel<GDPT_DENOISE_DEMOD>), grid, block, 0, stream, a);
    else if (kb.kind == GDPT_DENOISE_GUIDED) hipLaunchKernelGGL((pyr::up_kernel<GDPT_DENOISE_GUIDED>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pyr::up_kernel<GDPT_DENOISE_PLAIN>), grid, block, 0, stream, a);
    ck(hipGetLastError(), "nlm pyramid up launch");
    if (stats) read_stats(ws, a.g.blocks, a.wc, a.hc, stream, stats);
}

// the kind's existing device filter on one level, through its own entry point
void filter_level(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, const NlmKindBlocks &kb,
                  const GdptNlmParams &p, double *d_out, double *d_var_out, hipStream_t stream, GdptNlmStats *stats) {
    int rc;
    if (kb.kind == GDPT_DENOISE_DEMOD)
        rc = gdpt_denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_feat_var, kb.num_channels, &p, kb.has_guide ? &kb.guide : nullptr, &kb.demod,
                                           d_out, d_var_out, stream, stats);
    else if (kb.kind == GDPT_DENOISE_GUIDED)
        rc = gdpt_denoise_nlm_guided_device(w, h, d_img, d_var, d_feat, d_feat_var, &p, &kb.guide, d_out, d_var_out, stream, stats);
    else rc = gdpt_denoise_nlm_device(w, h, d_img, d_var, &p, d_out, d_var_out, stream, stats);
    if (rc != 0) throw std::runtime_error(gdpt_last_error());
}

} // namespace

NlmKindBlocks nlm_pyramid_check_kind(const std::string &who, int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, int num_channels,
                                     bool planes) {
    if (kind != GDPT_DENOISE_PLAIN && kind != GDPT_DENOISE_GUIDED && kind != GDPT_DENOISE_DEMOD)
        throw std::runtime_error(who + ": kind must be GDPT_DENOISE_PLAIN, GDPT_DENOISE_GUIDED or GDPT_DENOISE_DEMOD");
    if (kind == GDPT_DENOISE_PLAIN && guide) throw std::runtime_error(who + ": guide must be null for GDPT_DENOISE_PLAIN");
    if (kind != GDPT_DENOISE_DEMOD && demod) throw std::runtime_error(who + ": demod must be null unless kind is GDPT_DENOISE_DEMOD");
    if (kind == GDPT_DENOISE_PLAIN && planes) throw std::runtime_error(who + ": feat and feat_var must be null for GDPT_DENOISE_PLAIN (it reads none)");
    NlmKindBlocks kb;
    kb.kind = kind;
    kb.num_channels = planes ? num_channels : 0;
    if (kind == GDPT_DENOISE_GUIDED || guide) {
        kb.has_guide = true;
        if (guide) kb.guide = *guide; else gdpt_nlm_default_guide(&kb.guide);
        nlm_check_guide(who, kb.guide);
        if (planes && kb.guide.num_channels != num_channels) throw std::runtime_error(who + ": guide num_channels must equal num_channels");
        if (!planes && kb.guide.num_groups > 0) throw std::runtime_error(who + ": feat and feat_var are null (the guide's groups need their planes)");
    }
    if (kind == GDPT_DENOISE_DEMOD) {
        kb.has_demod = true;
        if (demod) kb.demod = *demod; else gdpt_nlm_default_demod(&kb.demod);
        if (!planes) throw std::runtime_error(who + ": feat and feat_var are null (a demod block needs its planes)");
        nlm_check_demod(who, kb.demod, num_channels);
    }
    return kb;
}

void nlm_pyramid_check_levels(const std::string &who, int levels) {
    if (levels < 1 || levels > GDPT_NLM_MAX_LEVELS) throw std::runtime_error(who + ": levels must be in [1, " + std::to_string(GDPT_NLM_MAX_LEVELS) + "]");
}

void denoise_nlm_multiscale_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const NlmKindBlocks &kb, int levels, const GdptNlmParams &p, double *d_out, double *d_var_out,
                                   hipStream_t stream, GdptNlmPyramidStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    PyramidStorage &ps = g_pyramids.get(dev, stream);
    std::lock_guard<std::mutex> lk(ps.mu);
    for (auto &e : ps.ev) if (!e) e.create();
    int lw[GDPT_NLM_MAX_LEVELS] = {w}, lh[GDPT_NLM_MAX_LEVELS] = {h}, made = 1;
    while (made < levels && (long long)lw[made - 1] * lh[made - 1] > 1) {
        lw[made] = (lw[made - 1] + 1) / 2; lh[made] = (lh[made - 1] + 1) / 2;
        made++;
    }
    GdptNlmPyramidStats st{};
    st.levels = made;
    for (int l = 0; l < made; l++) { st.width[l] = lw[l]; st.height[l] = lh[l]; }
    if (stats) ck(hipEventRecord(ps.ev[0], stream), "hipEventRecord");
    const bool planes = kb.num_channels > 0 && d_feat;
    const double *img[GDPT_NLM_MAX_LEVELS] = {d_img}, *var[GDPT_NLM_MAX_LEVELS] = {d_var}, *feat[GDPT_NLM_MAX_LEVELS] = {d_feat},
                 *fvar[GDPT_NLM_MAX_LEVELS] = {d_feat_var};
    for (int l = 1; l < made; l++) {                    // the pyramid of the inputs
        const size_t n = (size_t)lw[l] * lh[l];
        ps.img[l].grow(3 * n, stream, "hipMalloc(nlm pyramid level)"); ps.var[l].grow(3 * n, stream, "hipMalloc(nlm pyramid level)");
        if (planes) {
            ps.feat[l].grow(kb.num_channels * n, stream, "hipMalloc(nlm pyramid features)");
            ps.fvar[l].grow(kb.num_channels * n, stream, "hipMalloc(nlm pyramid features)");
        }
        down_launch(lw[l - 1], lh[l - 1], img[l - 1], var[l - 1], feat[l - 1], fvar[l - 1], kb, ps.img[l], ps.var[l], planes ? ps.feat[l].data() : nullptr,
                    planes ? ps.fvar[l].data() : nullptr, stream, nullptr);
        img[l] = ps.img[l]; var[l] = ps.var[l];
        feat[l] = planes ? ps.feat[l].data() : nullptr; fvar[l] = planes ? ps.fvar[l].data() : nullptr;
    }
    const double *filtered[GDPT_NLM_MAX_LEVELS] = {};
    for (int l = 0; l < made; l++) {                    // F_l; a single level goes straight to the call's outputs
        double *F = d_out;
        if (made > 1) { ps.filtered[l].grow(3 * (size_t)lw[l] * lh[l], stream, "hipMalloc(nlm pyramid filtered)"); F = ps.filtered[l]; }
        filter_level(lw[l], lh[l], img[l], var[l], feat[l], fvar[l], kb, p, F, l == 0 ? d_var_out : nullptr, stream, stats ? &st.level[l] : nullptr);
        filtered[l] = F;
    }
    const double *coarse = filtered[made - 1];           // out_L = F_L
    for (int l = made - 2; l >= 0; l--) {
        double *o = d_out;
        if (l > 0) { ps.out[l].grow(3 * (size_t)lw[l] * lh[l], stream, "hipMalloc(nlm pyramid combined)"); o = ps.out[l]; }
        up_launch(lw[l], lh[l], img[l], var[l], feat[l], fvar[l], kb, filtered[l], coarse, o, stream, nullptr);
        coarse = o;
    }
    if (!stats) return;
    ck(hipEventRecord(ps.ev[1], stream), "hipEventRecord");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm multiscale)");
    { float ms = 0; ck(hipEventElapsedTime(&ms, ps.ev[0], ps.ev[1]), "hipEventElapsedTime"); st.total_ms = ms; }
    *stats = st;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;
using gdpt::Mirror;

// what every entry point here refuses in a level's inputs; `who` names the caller. Returns the kind's blocks in force.
gdpt::NlmKindBlocks check_level(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                const double *feat_var, int num_channels, int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    if (feat && !feat_var) throw std::runtime_error(who + ": feat_var is null (feat and feat_var go together)");
    if (feat_var && !feat) throw std::runtime_error(who + ": feat is null (feat and feat_var go together)");
    return gdpt::nlm_pyramid_check_kind(who, kind, guide, demod, num_channels, feat != nullptr);
}

// `out` (named `name`) against the inputs `in`
void check_alias(const std::string &who, const char *name, const double *out, std::initializer_list<const double *> in) {
    if (!out) return;
    for (const double *q : in) if (q && q == out) throw std::runtime_error(who + ": " + name + " must not alias an input or another output");
}

void check_down(const std::string &who, const double *img, const double *var, const double *feat, const double *feat_var, double *img_out,
                double *var_out, double *feat_out, double *feat_var_out) {
    if (!img_out) throw std::runtime_error(who + ": img_out is null");
    if (!var_out) throw std::runtime_error(who + ": var_out is null");
    if (feat && !feat_out) throw std::runtime_error(who + ": feat_out is null (the planes of the next level go with feat)");
    if (feat && !feat_var_out) throw std::runtime_error(who + ": feat_var_out is null (the planes of the next level go with feat)");
    if (!feat && (feat_out || feat_var_out)) throw std::runtime_error(who + ": feat_out and feat_var_out must be null without feat");
    check_alias(who, "img_out", img_out, {img, var, feat, feat_var});
    check_alias(who, "var_out", var_out, {img, var, feat, feat_var, img_out});
    check_alias(who, "feat_out", feat_out, {img, var, feat, feat_var, img_out, var_out});
    check_alias(who, "feat_var_out", feat_var_out, {img, var, feat, feat_var, img_out, var_out, feat_out});
}

void check_up(const std::string &who, const double *img, const double *var, const double *feat, const double *feat_var, const double *filtered,
              const double *coarse_out, double *out) {
    if (!filtered) throw std::runtime_error(who + ": filtered is null");
    if (!coarse_out) throw std::runtime_error(who + ": coarse_out is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    check_alias(who, "out", out, {img, var, feat, feat_var, filtered, coarse_out});
}

GdptNlmParams check_multiscale(const std::string &who, const double *img, const double *var, const double *feat, const double *feat_var, int levels,
                               const GdptNlmParams *params, double *out, double *var_out) {
    gdpt::nlm_pyramid_check_levels(who, levels);
    GdptNlmParams p;
    if (params) p = *params;
    else gdpt_nlm_default_params(&p);
    gdpt::nlm_check_params(who, p);
    if (!out) throw std::runtime_error(who + ": out is null");
    check_alias(who, "out", out, {img, var, feat, feat_var});
    check_alias(who, "var_out", var_out, {img, var, feat, feat_var, out});
    return p;
}

} // namespace

extern "C" {

int gdpt_nlm_pyramid_down_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                 int num_channels, int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *d_img_out,
                                 double *d_var_out, double *d_feat_out, double *d_feat_var_out, void *stream, GdptNlmPyramidOpStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_nlm_pyramid_down_device";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, d_img, d_var, d_feat, d_feat_var, num_channels, kind, guide, demod);
        check_down(who, d_img, d_var, d_feat, d_feat_var, d_img_out, d_var_out, d_feat_out, d_feat_var_out);
        need_a_device(who);
        gdpt::down_launch(width, height, d_img, d_var, d_feat, d_feat_var, kb, d_img_out, d_var_out, d_feat_out, d_feat_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_nlm_pyramid_down(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int num_channels,
                          int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *img_out, double *var_out, double *feat_out,
                          double *feat_var_out, GdptNlmPyramidOpStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_nlm_pyramid_down";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, img, var, feat, feat_var, num_channels, kind, guide, demod);
        check_down(who, img, var, feat, feat_var, img_out, var_out, feat_out, feat_var_out);
        need_a_device(who);
        const size_t n = (size_t)width * height, nc = (size_t)((width + 1) / 2) * ((height + 1) / 2), ch = (size_t)kb.num_channels;
        Mirror m_img, m_var, m_feat, m_fvar, o_img, o_var, o_feat, o_fvar;
        m_img.up(img, 3 * n); m_var.up(var, 3 * n); m_feat.up(feat, ch * n); m_fvar.up(feat_var, ch * n);
        o_img.make(img_out, 3 * nc); o_var.make(var_out, 3 * nc); o_feat.make(feat_out, ch * nc); o_fvar.make(feat_var_out, ch * nc);
        gdpt::down_launch(width, height, m_img.d, m_var.d, m_feat.d, m_fvar.d, kb, o_img.d, o_var.d, o_feat.d, o_fvar.d, nullptr, stats);
        o_img.down(img_out, 3 * nc); o_var.down(var_out, 3 * nc); o_feat.down(feat_out, ch * nc); o_fvar.down(feat_var_out, ch * nc);
    });
}

int gdpt_nlm_pyramid_up_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               int num_channels, int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, const double *d_filtered,
                               const double *d_coarse_out, double *d_out, void *stream, GdptNlmPyramidOpStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_nlm_pyramid_up_device";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, d_img, d_var, d_feat, d_feat_var, num_channels, kind, guide, demod);
        check_up(who, d_img, d_var, d_feat, d_feat_var, d_filtered, d_coarse_out, d_out);
        need_a_device(who);
        gdpt::up_launch(width, height, d_img, d_var, d_feat, d_feat_var, kb, d_filtered, d_coarse_out, d_out, (hipStream_t)stream, stats);
    });
}

int gdpt_nlm_pyramid_up(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int num_channels,
                        int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, const double *filtered, const double *coarse_out, double *out,
                        GdptNlmPyramidOpStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_nlm_pyramid_up";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, img, var, feat, feat_var, num_channels, kind, guide, demod);
        check_up(who, img, var, feat, feat_var, filtered, coarse_out, out);
        need_a_device(who);
        const size_t n = (size_t)width * height, nc = (size_t)((width + 1) / 2) * ((height + 1) / 2), ch = (size_t)kb.num_channels;
        Mirror m_img, m_var, m_feat, m_fvar, m_fil, m_coarse, o_out;
        m_img.up(img, 3 * n); m_var.up(var, 3 * n); m_feat.up(feat, ch * n); m_fvar.up(feat_var, ch * n);
        m_fil.up(filtered, 3 * n); m_coarse.up(coarse_out, 3 * nc); o_out.make(out, 3 * n);
        gdpt::up_launch(width, height, m_img.d, m_var.d, m_feat.d, m_fvar.d, kb, m_fil.d, m_coarse.d, o_out.d, nullptr, stats);
        o_out.down(out, 3 * n);
    });
}

int gdpt_denoise_nlm_multiscale_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                       int num_channels, int kind, int levels, const GdptNlmParams *params, const GdptNlmGuide *guide,
                                       const GdptNlmDemod *demod, double *d_out, double *d_var_out, void *stream, GdptNlmPyramidStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_multiscale_device";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, d_img, d_var, d_feat, d_feat_var, num_channels, kind, guide, demod);
        const GdptNlmParams p = check_multiscale(who, d_img, d_var, d_feat, d_feat_var, levels, params, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_nlm_multiscale_launch(width, height, d_img, d_var, d_feat, d_feat_var, kb, levels, p, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_multiscale(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                                int num_channels, int kind, int levels, const GdptNlmParams *params, const GdptNlmGuide *guide,
                                const GdptNlmDemod *demod, double *out, double *var_out, GdptNlmPyramidStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_multiscale";
        const gdpt::NlmKindBlocks kb = check_level(who, width, height, img, var, feat, feat_var, num_channels, kind, guide, demod);
        const GdptNlmParams p = check_multiscale(who, img, var, feat, feat_var, levels, params, out, var_out);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, (size_t)width * height * kb.num_channels, out, var_out);
        gdpt::denoise_nlm_multiscale_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, kb, levels, p, m.out.d, m.var_out.d, nullptr, stats);
        ck(hipStreamSynchronize(nullptr), "hipStreamSynchronize(nlm multiscale)");
        m.down(out, var_out);
    });
}

} // extern "C"
