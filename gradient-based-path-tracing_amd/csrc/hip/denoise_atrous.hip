// denoise_atrous.hip — the edge-avoiding a-trous wavelet filter with variance-guided weights on (mean, variance of the mean), for
// gfx950 (include/gdpt.h: gdpt_denoise_atrous*, where the definition stands; Dammertz et al. 2010, Schied et al. 2017).
//
// One launch per level. A level reads the previous level's planes and writes its own: the first level reads the caller's planes
// (load_pixel of nlm_device.h: validity from the inputs, and with a demod block the quotients), the levels between ping-pong over two
// (u, v) film pairs of the workspace, the last level writes the caller's out / var_out, multiplies the albedo back and leaves the
// film sums through leave_block_sum for finish_kernel (image_kernels.h): a fixed order, the same bits every time. The first level
// also leaves the valid set, a byte per pixel, which the later levels read in the place of the inputs: the set is fixed by the inputs,
// and a value between the levels is never asked whether it is finite. No launch writes a plane that the same launch reads.
//
// Kernels: two forms of the one definition, both over 16 x 16 tiles under the "nlm" grid rule, a thread on a pixel of the tile.
//   direct_kernel   the literal definition: every tap is read from global memory.
//   staged_kernel   the tile with a halo of 2 step pixels staged in LDS, plane by plane (three u, three v, a validity flag;
//                   out-of-film and invalid entries are u = v = 0, flag 0): (16 + 4 step)^2 entries of 52 bytes, 20.8 KB at step 1,
//                   30.0 KB at 2, 53.2 KB at 4, 119.8 KB at 8; at step 16 it would be 332.8 KB and does not exist. The 25 taps then
//                   come from LDS with no barrier between them. Every plane is a plane of doubles (or ints), so consecutive lanes
//                   read consecutive elements; a half-wave covers two rows of 16 pixels whose distance is the pitch 16 + 4 step, which
//                   is never 16 mod 32 doubles below step 8, so the two rows share 8 - 32 of the 64 banks: the tap reads are
//                   two-way conflicted at steps 1, 2, 4 and free at 8. A pitch of 48 frees them at 2.4 x the LDS of step 1 and was
//                   measured to change no level's time (profiles/atrous_times.txt): the tap is three fp64 divisions and an exp (and
//                   a division per guide channel) against seven LDS reads. The pitch stays dense.
// atrous_staged below says which form a step takes: staged up to step 4, where its worst run beats the direct form's best
// (profiles/atrous_times.txt), direct beyond; the knob nlm_direct (include/gdpt_debug.h) forces the direct form.
// Both are templates on GUIDED and DEMOD, as the kernels of denoise_nlm.hip: a guided kernel keeps its own pixel's features in
// registers (OwnFeatures) and reads those of the tap from the planar planes in global memory.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "denoise_atrous.h"
#include "nlm_device.h"
#include "nlm_host.h"

#include <cmath>
#include <mutex>
#include <type_traits>

namespace atrous {

using namespace nlm;

constexpr int kMaxLevels = GDPT_ATROUS_MAX_LEVELS;
constexpr int kStagedCap = 8;         // the largest step at which the stage fits a CU's LDS
constexpr int kStagedProduct = 4;     // the largest step at which the staged form is the product route (profiles/atrous_times.txt)

struct Args {
    static constexpr bool kGuided = false, kDemod = false;
    TileGrid g;                       // 16 x 16 tiles
    int step, first, last;            // first: reads the caller's planes; last: writes the caller's planes and leaves the sums
    double k2, alpha, eps;
    const double *img, *var;          // the caller's planes
    const double *pu, *pv;            // the previous level's planes (not first)
    unsigned char *mask;              // the valid set: written by the first level, read by the later ones; null in a call of one level
    double *out, *var_out;            // this level's planes; var_out nullable on the last level
    double *partials;                 // as nlm::Args (denoise_nlm.hip); left by the last level
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

// h_a of tap a = -2 .. 2
__device__ __forceinline__ double spline(int a) { return a == 0 ? 0.375 : (a == 1 || a == -1) ? 0.25 : 0.0625; }

struct Accum {
    double num[3] = {0.0, 0.0, 0.0}, vnum[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
    // e: the pair distance; Df: the pair's feature distance, >= 0; h: h_a h_b
    __device__ __forceinline__ void add(double h, double e, double Df, const double u[3], const double v[3]) {
        double D = e > 0.0 ? e : 0.0;
        D = fmax(D, Df);
        const double wgt = h * exp(-D);
        wsum += wgt;
#pragma unroll
        for (int c = 0; c < 3; c++) { num[c] += wgt * u[c]; vnum[c] += (wgt * wgt) * v[c]; }
    }
};

// this level's triples of film pixel (x, y), which is inside the film; returns whether it is valid
template <class A>
__device__ __forceinline__ bool load_level(const A &a, int x, int y, double u[3], double v[3]) {
    if (a.first) return load_pixel(a, x, y, u, v);
    const size_t p = (size_t)y * a.g.w + x;
    if (a.mask[p] == 0) return false;
#pragma unroll
    for (int c = 0; c < 3; c++) { u[c] = a.pu[3 * p + c]; v[c] = a.pv[3 * p + c]; }
    return true;
}

// an invalid pixel p: its place in the valid set, and on the last level its input bits
template <class A>
__device__ __forceinline__ void leave_out(const A &a, size_t p, Sums &s) {
    if (a.first && a.mask) a.mask[p] = 0;
    if (!a.last) return;
    const double u[3] = {a.img[3 * p], a.img[3 * p + 1], a.img[3 * p + 2]}, v[3] = {a.var[3 * p], a.var[3 * p + 1], a.var[3 * p + 2]};
    keep_pixel(a, 3 * p, u, v, s);
}

// a valid pixel p: the level's outputs; the last level multiplies the pixel's own a~ back and takes its terms of the film sums, the
// input terms from the caller's triples
template <class A>
__device__ __forceinline__ void finish_level(const A &a, size_t p, const Accum &acc, Sums &s) {
    const size_t i = 3 * p;
    const double w2 = acc.wsum * acc.wsum;
    double o[3], vo[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { o[c] = acc.num[c] / acc.wsum; vo[c] = acc.vnum[c] / w2; }
    if (a.first && a.mask) a.mask[p] = 1;
    if (!a.last) {
#pragma unroll
        for (int c = 0; c < 3; c++) { a.out[i + c] = o[c]; a.var_out[i + c] = vo[c]; }
        return;
    }
    if constexpr (A::kDemod) {
        double al[3];
        effective_albedo(a.dm, p, al);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double al2 = al[c] * al[c];
            o[c] = o[c] * al[c];
            vo[c] = vo[c] * al2;
        }
    }
    double ui[3], vi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.out[i + c] = o[c];
        if (a.var_out) a.var_out[i + c] = vo[c];
        ui[c] = a.img[i + c]; vi[c] = a.var[i + c];
    }
    s.var_in += (vi[0] + vi[1]) + vi[2];
    s.sq_in += (ui[0] * ui[0] + ui[1] * ui[1]) + ui[2] * ui[2];
    s.var_out += (vo[0] + vo[1]) + vo[2];
    s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
}

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void direct_kernel(ArgsOf<GUIDED, DEMOD> a) {
    __shared__ double red[kBlock / 64];
    const int step = a.step;
    Sums s;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t p = (size_t)y * a.g.w + x;
        double u[3], v[3];
        if (!load_level(a, x, y, u, v)) { leave_out(a, p, s); continue; }
        OwnFeatures own;
        if constexpr (GUIDED) own.load(a.gd, p);
        Accum acc;
        for (int ta = -2; ta <= 2; ta++)
            for (int tb = -2; tb <= 2; tb++) {
                const int qx = x + tb * step, qy = y + ta * step;
                if (qx < 0 || qy < 0 || qx >= a.g.w || qy >= a.g.h) continue;
                double uq[3], vq[3];
                if (!load_level(a, qx, qy, uq, vq)) continue;
                const double e = pair_distance(u, v, uq, vq, a.k2, a.alpha, a.eps);
                double Df = 0.0;
                if constexpr (GUIDED) Df = own.distance(a.gd, (size_t)qy * a.g.w + qx);
                acc.add(spline(ta) * spline(tb), e, Df, uq, vq);
            }
        finish_level(a, p, acc, s);
    }
    if (a.last) leave_partials(a, s, red);
}

// doubles, then ints, of the stage at `step`
__host__ __device__ inline int stage_width(int step) { return kTile + 4 * step; }
__host__ __device__ inline size_t stage_bytes(int step) {
    const size_t sn = (size_t)stage_width(step) * stage_width(step);
    return 6 * sn * sizeof(double) + sn * sizeof(int);
}

template <bool GUIDED, bool DEMOD>
__global__ __launch_bounds__(kBlock) void staged_kernel(ArgsOf<GUIDED, DEMOD> a) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    const int step = a.step, halo = 2 * step;
    const int sw = stage_width(step), sn = sw * sw;     // the stage: the tile and its halo
    double *const su = lds, *const sv = lds + 3 * sn;   // plane c at su + c sn, sv + c sn
    int *const sflag = (int *)(lds + 6 * sn);
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
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
            if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) ok = load_level(a, gx, gy, u, v);
#pragma unroll
            for (int c = 0; c < 3; c++) { su[c * sn + k] = ok ? u[c] : 0.0; sv[c * sn + k] = ok ? v[c] : 0.0; }
            sflag[k] = ok ? 1 : 0;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;         // (no barrier stands behind this point of the trip)
        const size_t p = (size_t)y * a.g.w + x;
        if (sflag[pc] == 0) { leave_out(a, p, s); continue; }
        OwnFeatures own;
        if constexpr (GUIDED) own.load(a.gd, p);
        const double u[3] = {su[pc], su[sn + pc], su[2 * sn + pc]}, v[3] = {sv[pc], sv[sn + pc], sv[2 * sn + pc]};
        Accum acc;
        for (int ta = -2; ta <= 2; ta++)
            for (int tb = -2; tb <= 2; tb++) {
                const int iq = pc + (ta * sw + tb) * step;
                if (sflag[iq] == 0) continue;
                const double uq[3] = {su[iq], su[sn + iq], su[2 * sn + iq]}, vq[3] = {sv[iq], sv[sn + iq], sv[2 * sn + iq]};
                const double e = pair_distance(u, v, uq, vq, a.k2, a.alpha, a.eps);
                double Df = 0.0;
                if constexpr (GUIDED) Df = own.distance(a.gd, (size_t)(y + ta * step) * a.g.w + (x + tb * step));
                acc.add(spline(ta) * spline(tb), e, Df, uq, vq);
            }
        finish_level(a, p, acc, s);
    }
    if (a.last) leave_partials(a, s, red);
}

} // namespace atrous

namespace gdpt {

namespace {

// the sums', and what the levels keep between them
struct AtrousWorkspace : SumsWorkspace {
    DeviceBuffer<double> plane[4];    // the two (u, v) film pairs between the levels
    DeviceBuffer<unsigned char> mask; // the valid set
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<AtrousWorkspace> &g_workspaces = *new PerStream<AtrousWorkspace>();

// one level of one instantiation, enqueued on `stream`
template <bool GUIDED, bool DEMOD>
void launch_level(const atrous::ArgsOf<GUIDED, DEMOD> &a, bool staged, hipStream_t stream) {
    const int nb = a.g.blocks;
    if (!staged) {
        hipLaunchKernelGGL((atrous::direct_kernel<GUIDED, DEMOD>), dim3(nb), dim3(film::kBlock), 0, stream, a);
        return;
    }
    const size_t lds = atrous::stage_bytes(a.step);
    ck(hipFuncSetAttribute(reinterpret_cast<const void *>(atrous::staged_kernel<GUIDED, DEMOD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
       "hipFuncSetAttribute(atrous stage)");
    hipLaunchKernelGGL((atrous::staged_kernel<GUIDED, DEMOD>), dim3(nb), dim3(film::kBlock), lds, stream, a);
}

// Whether the level of step `step` takes the staged kernel under the value `knob` of nlm_direct: 0 the product routes, 1 the direct
// form at every step, 2 the staged form wherever it exists (for measurements).
bool atrous_staged(int step, long knob) {
    if (knob == 1) return false;
    return step <= (knob == 2 ? atrous::kStagedCap : atrous::kStagedProduct);
}

} // namespace

void atrous_check_params(const std::string &who, const GdptAtrousParams &p) {
    const std::string cap = std::to_string(atrous::kMaxLevels);
    if (p.levels < 1 || p.levels > atrous::kMaxLevels) throw std::runtime_error(who + ": levels must be in [1, " + cap + "]");
    if (p.first_level < 0 || p.first_level >= atrous::kMaxLevels) throw std::runtime_error(who + ": first_level must be in [0, " + cap + ")");
    if (p.first_level + p.levels > atrous::kMaxLevels) throw std::runtime_error(who + ": first_level + levels must be <= " + cap);
    if (!std::isfinite(p.k) || !(p.k > 0)) throw std::runtime_error(who + ": k must be finite and > 0");
    if (!std::isfinite(p.alpha) || !(p.alpha >= 0)) throw std::runtime_error(who + ": alpha must be finite and >= 0");
    if (!std::isfinite(p.epsilon) || !(p.epsilon > 0)) throw std::runtime_error(who + ": epsilon must be finite and > 0");
    if (p.reserved[0] != 0 || p.reserved[1] != 0) throw std::runtime_error(who + ": atrous reserved must be 0");
}

void denoise_atrous_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                           const GdptAtrousParams &p, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *d_out, double *d_var_out,
                           hipStream_t stream, GdptNlmStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    AtrousWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    ws.prepare("atrous");
    const size_t pixels = (size_t)w * h;
    if (p.levels > 1) {               // (a call of one level reads and writes the caller's planes alone)
        for (int k = 0; k < (p.levels > 2 ? 4 : 2); k++) ws.plane[k].grow(3 * pixels, stream, "hipMalloc(atrous planes)");
        ws.mask.grow(pixels, stream, "hipMalloc(atrous valid set)");
    }
    if (guide && guide->num_groups == 0) guide = nullptr;      // no group: no feature term, the unguided kernels

    atrous::GuidedArgs a{};
    a.g = film::tile_grid(w, h, kNlmTile, kNlmTile);
    a.k2 = p.k * p.k; a.alpha = p.alpha; a.eps = p.epsilon;
    a.img = d_img; a.var = d_var; a.partials = ws.partials;
    a.mask = p.levels > 1 ? ws.mask.data() : nullptr;
    if (guide) fill_guide(a.gd, *guide, d_feat, d_feat_var, pixels);
    nlm::Demod dm{};
    if (demod) dm = nlm::Demod{d_feat, d_feat_var, pixels, demod->albedo_channel, demod->coverage_channel, demod->floor};
    const int nb = a.g.blocks;
    const long knob = (long)debug_knob("nlm_direct", 0);
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    for (int i = 0; i < p.levels; i++) {
        a.step = 1 << (p.first_level + i);
        a.first = i == 0; a.last = i == p.levels - 1;
        // level i writes pair i mod 2 and reads pair (i - 1) mod 2
        a.pu = i > 0 ? ws.plane[2 * ((i - 1) & 1)].data() : nullptr;
        a.pv = i > 0 ? ws.plane[2 * ((i - 1) & 1) + 1].data() : nullptr;
        a.out = a.last ? d_out : ws.plane[2 * (i & 1)].data();
        a.var_out = a.last ? d_var_out : ws.plane[2 * (i & 1) + 1].data();
        const bool staged = atrous_staged(a.step, knob);
        const atrous::Args &plain = a;
        if (demod) {
            if (guide) {
                atrous::GuidedDemodArgs ad{};
                static_cast<atrous::GuidedArgs &>(ad) = a; ad.dm = dm;
                launch_level<true, true>(ad, staged, stream);
            } else {
                atrous::DemodArgs ad{};
                static_cast<atrous::Args &>(ad) = plain; ad.dm = dm;
                launch_level<false, true>(ad, staged, stream);
            }
        } else if (guide) launch_level<true, false>(a, staged, stream);
        else launch_level<false, false>(plain, staged, stream);
        ck(hipGetLastError(), "atrous launch");
    }
    if (!stats) return;
    ws.read_stats(nb, stream, "atrous", stats);
    stats->window_radius = 2 << (p.first_level + p.levels - 1); stats->patch_radius = 0;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// What both entry points refuse; `who` names the caller. Returns the parameters in force.
GdptAtrousParams check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                 const double *feat_var, int num_channels, const GdptAtrousParams *params, const GdptNlmGuide *guide,
                                 const GdptNlmDemod *demod, const double *out, const double *var_out) {
    gdpt::check_film(who, width, height, img, var, out, var_out);
    GdptAtrousParams p;
    if (params) p = *params;
    else gdpt_atrous_default_params(&p);
    gdpt::atrous_check_params(who, p);
    if (num_channels < 0 || num_channels > GDPT_NLM_MAX_CHANNELS)
        throw std::runtime_error(who + ": num_channels must be in [0, " + std::to_string(GDPT_NLM_MAX_CHANNELS) + "]");
    if (guide) {
        gdpt::nlm_check_guide(who, *guide);
        if (guide->num_channels != num_channels) throw std::runtime_error(who + ": guide num_channels must equal num_channels");
    }
    if (demod) gdpt::nlm_check_demod(who, *demod, num_channels);
    if ((guide && guide->num_groups > 0) || demod) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    if (feat && (out == feat || out == feat_var)) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && feat && (var_out == feat || var_out == feat_var)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    return p;
}

} // namespace

extern "C" {

void gdpt_atrous_default_params(GdptAtrousParams *p) {
    if (!p) return;
    *p = GdptAtrousParams{};
    p->levels = 5; p->first_level = 0;
    p->k = 2.0; p->alpha = 1.0; p->epsilon = 1e-10;
}

int gdpt_denoise_atrous_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               int num_channels, const GdptAtrousParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod,
                               double *d_out, double *d_var_out, void *stream, GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_atrous_device";
        const GdptAtrousParams p = check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, num_channels, params, guide, demod, d_out, d_var_out);
        need_a_device(who);
        gdpt::denoise_atrous_launch(width, height, d_img, d_var, d_feat, d_feat_var, p, guide, demod, d_out, d_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_atrous(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int num_channels,
                        const GdptAtrousParams *params, const GdptNlmGuide *guide, const GdptNlmDemod *demod, double *out, double *var_out,
                        GdptNlmStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_atrous";
        const GdptAtrousParams p = check_arguments(who, width, height, img, var, feat, feat_var, num_channels, params, guide, demod, out, var_out);
        need_a_device(who);
        const bool planes = (guide && guide->num_groups > 0) || demod;
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, planes ? (size_t)width * height * num_channels : 0, out, var_out);
        gdpt::denoise_atrous_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, p, guide, demod, m.out.d, m.var_out.d, nullptr, stats);
        m.down(out, var_out);
    });
}

} // extern "C"
