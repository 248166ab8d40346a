// nlm_joint.hip — joint filtering: the non-local-means weights of a guide film applied to companion films as well, for gfx950
// (include/gdpt.h: gdpt_denoise_nlm_joint*, where the definition stands; the joint filtering step of Manzi, Vicini, Zwicker 2016 and of
// Rousselle, Jarosz, Novak 2016). The guide film is filtered exactly as denoise_nlm.hip filters it: its weights w_o(p) also average
// NC companion films (a_j, s_j), which play no part in the weights beyond a pixel's validity.
//
// Kernels: joint_direct_kernel<GUIDED, NC> and joint_tiled_kernel<GUIDED, NC>, the two forms of denoise_nlm.hip (chosen by the same
// test knob nlm_direct) on the same device code (nlm_device.h): the tap loop and the stage are run through load_joint_pixel, the guide
// film's argument block is nlm::Args itself. Block partials go through leave_block_sum for finish_runs_kernel (image_kernels.h): a
// fixed order, the same bits every time. No launch writes a plane it reads.
//   The guide film's sums go through nlm::Accum::add and end in nlm::finish_pixel: with every companion valid its out, var_out and
//   sums are the guided filter's bit for bit. Accum::add returns the weight; the companions' terms go through nlm::add_term, the very
//   function Accum::add uses for the guide film (one copy of the two expressions, so one contraction into fma), and are divided as
//   finish_pixel divides: a companion that is the guide film itself comes back as out, var_out bit for bit.
//   The stage holds the guide film alone: the companions do not go into LDS. A thread reads a_j(p+o) and s_j(p+o) from global memory
//   at the point where it has w_o(p), as the guided kernel reads its feature planes there: a tile row of a film is 16 x 24 contiguous
//   bytes, a wave's read four such rows, served from L1 / L2. Per thread 6 NC accumulators more. NC is a compile-time count (1 .. 4; a
//   call without companions is the guided filter itself), so every accumulator index is static: no scratch, no spilled VGPR
//   (profiles/nlm_kernel_resources.txt).
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_host.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

namespace nlmj {

using namespace nlm;              // nlm_device.h; and film's kBlock, TileGrid, leave_block_sum through it

constexpr int kMaxN = GDPT_NLM_JOINT_MAX;
constexpr int kGuideRuns = 6;                      // what nlm::leave_partials leaves: runs 0 .. 5
constexpr int kMaxRuns = kGuideRuns + 2 * kMaxN;   // then sum_var_in[j], sum_var_out[j] of companion j as runs 6 + 2 j, 7 + 2 j

// the guide film's block (partials: kGuideRuns + 2 NC runs of gridDim.x doubles), and the companions
template <bool GUIDED, int NC>
struct Args : ArgsOf<GUIDED, false> {
    const double *comp[NC], *comp_var[NC];
    double *comp_out[NC], *comp_var_out[NC];      // comp_var_out[j] nullable
};

// whether every companion triple at film index i (3 (y w + x)) is finite, with finite variances >= 0
template <class A, int NC>
__device__ __forceinline__ bool valid_companions(const A &a, size_t i) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NC; j++) {
        double at[3], st[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { at[c] = a.comp[j][i + c]; st[c] = a.comp_var[j][i + c]; }
        ok = ok && valid_triples(at, st);
    }
    return ok;
}

// nlm::load_pixel of the guide film under the joint validity
template <class A, int NC>
__device__ __forceinline__ bool load_joint_pixel(const A &a, int x, int y, double u[3], double v[3]) {
    const bool ok = load_pixel(a, x, y, u, v);
    const bool okc = valid_companions<A, NC>(a, ((size_t)y * a.g.w + x) * 3);
    return ok && okc;
}

// a pixel's companion sums, and their terms of the film sums
template <int NC>
struct Companions {
    double num[NC][3], vnum[NC][3];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < NC; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) { num[j][c] = 0.0; vnum[j][c] = 0.0; }
    }
    // the terms of p+o = film index iq under the weight w_o(p)
    template <class A>
    __device__ __forceinline__ void add(const A &a, size_t iq, double wgt) {
#pragma unroll
        for (int j = 0; j < NC; j++) {
            double aq[3], sq[3];
#pragma unroll
            for (int c = 0; c < 3; c++) { aq[c] = a.comp[j][iq + c]; sq[c] = a.comp_var[j][iq + c]; }
            add_term(num[j], vnum[j], wgt, aq, sq);
        }
    }
};
template <int NC>
struct CompanionSums {
    double var_in[NC], var_out[NC];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < NC; j++) { var_in[j] = 0.0; var_out[j] = 0.0; }
    }
};

// the companions' outputs of valid pixel i, divided as nlm::finish_pixel divides the guide film's
template <class A, int NC>
__device__ __forceinline__ void finish_companions(const A &a, size_t i, const Accum &acc, const Companions<NC> &cp, CompanionSums<NC> &cs) {
    const double w2 = acc.wsum * acc.wsum;
#pragma unroll
    for (int j = 0; j < NC; j++) {
        double vi[3], vo[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double o = cp.num[j][c] / acc.wsum;
            vo[c] = cp.vnum[j][c] / w2;
            vi[c] = a.comp_var[j][i + c];
            a.comp_out[j][i + c] = o;
            if (a.comp_var_out[j]) a.comp_var_out[j][i + c] = vo[c];
        }
        cs.var_in[j] += (vi[0] + vi[1]) + vi[2];
        cs.var_out[j] += (vo[0] + vo[1]) + vo[2];
    }
}

// an invalid pixel's companion triples, bit for bit (nlm::keep_pixel keeps the guide film's and counts the pixel)
template <class A, int NC>
__device__ __forceinline__ void keep_companions(const A &a, size_t i) {
#pragma unroll
    for (int j = 0; j < NC; j++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a.comp_out[j][i + c] = a.comp[j][i + c];
            if (a.comp_var_out[j]) a.comp_var_out[j][i + c] = a.comp_var[j][i + c];
        }
}

template <class A, int NC>
__device__ __forceinline__ void leave_joint_partials(const A &a, const Sums &s, const CompanionSums<NC> &cs, double *red) {
    leave_partials(a, s, red);
#pragma unroll
    for (int j = 0; j < NC; j++) {
        leave_block_sum(a.partials, kGuideRuns + 2 * j, cs.var_in[j], red);
        leave_block_sum(a.partials, kGuideRuns + 2 * j + 1, cs.var_out[j], red);
    }
}

// nlm::direct_kernel with the companions: the literal definition, every read from global memory
template <bool GUIDED, int NC>
__global__ __launch_bounds__(kBlock) void joint_direct_kernel(Args<GUIDED, NC> a) {
    using A = Args<GUIDED, NC>;
    __shared__ double red[kBlock / 64];
    const int r = a.r;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_joint_pixel<A, NC>(a, x, y, u, v); };
    Sums s;
    CompanionSums<NC> cs;
    cs.clear();
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = tp.y;
        if (x >= a.g.w || y >= a.g.h) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (!load(x, y, u, v)) { keep_pixel(a, i, u, v, s); keep_companions<A, NC>(a, i); continue; }
        OwnFeatures own;
        if constexpr (GUIDED) own.load(a.gd, (size_t)y * a.g.w + x);
        Accum acc;
        Companions<NC> cp;
        cp.clear();
        for (int oy = -r; oy <= r; oy++)
            for (int ox = -r; ox <= r; ox++) {
                const int qx = x + ox, qy = y + oy;
                if (qx < 0 || qy < 0 || qx >= a.g.w || qy >= a.g.h) continue;
                double uq[3], vq[3];
                if (!load(qx, qy, uq, vq)) continue;
                double S;
                int C;
                patch_distance(a, load, x, y, ox, oy, S, C);      // (C >= 1: the tap n = 0 counts)
                const size_t q = (size_t)qy * a.g.w + qx;
                double wgt;
                if constexpr (GUIDED) wgt = acc.template add<true>(S, C, uq, vq, own.distance(a.gd, q));
                else wgt = acc.add(S, C, uq, vq);
                cp.add(a, q * 3, wgt);
            }
        finish_pixel(a, i, u, v, acc, s);
        finish_companions<A, NC>(a, i, acc, cp, cs);
    }
    leave_joint_partials<A, NC>(a, s, cs, red);
}

// nlm::tiled_kernel with the companions: the guide film's tile and halo staged under the joint validity; the companions' terms of
// p+o from global memory
template <bool GUIDED, int NC>
__global__ __launch_bounds__(kBlock) void joint_tiled_kernel(Args<GUIDED, NC> a) {
    using A = Args<GUIDED, NC>;
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    Stage st;
    st.lay_out(a.r, a.f, lds);
    const int pc = st.pc;
    const auto load = [&](int x, int y, double u[3], double v[3]) { return load_joint_pixel<A, NC>(a, x, y, u, v); };
    Sums s;
    CompanionSums<NC> cs;
    cs.clear();
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage has been read
        st.fill(a.g, tp.x0, tp.y0, load);
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const bool okp = inside && st.sflag[pc] != 0;
        OwnFeatures own;
        if constexpr (GUIDED) { if (okp) own.load(a.gd, (size_t)y * a.g.w + x); }
        Accum acc;
        Companions<NC> cp;
        cp.clear();
        st.sweep(a.k2, a.alpha, a.eps, okp, [&](int iq, double S, int C, int oy, int ox) {
            double uq[3], vq[3];
            st.mean(iq, uq); st.variance(iq, vq);
            const size_t q = (size_t)(y + oy) * a.g.w + (x + ox);
            double wgt;
            if constexpr (GUIDED) wgt = acc.template add<true>(S, C, uq, vq, own.distance(a.gd, q));
            else wgt = acc.add(S, C, uq, vq);
            cp.add(a, q * 3, wgt);
        });
        if (!inside) continue;
        const size_t i = ((size_t)y * a.g.w + x) * 3;
        double u[3], v[3];
        if (okp) {
            st.mean(pc, u); st.variance(pc, v);
            finish_pixel(a, i, u, v, acc, s);
            finish_companions<A, NC>(a, i, acc, cp, cs);
        } else {
            load_pixel(a, x, y, u, v);                  // (the stage holds zeros in its place)
            keep_pixel(a, i, u, v, s);
            keep_companions<A, NC>(a, i);
        }
    }
    leave_joint_partials<A, NC>(a, s, cs, red);
}

} // namespace nlmj

namespace gdpt {

namespace {

struct JointWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;    // kMaxRuns runs of kMaxBlocks
    DeviceBuffer<double> d_sums;      // kMaxRuns
    PinnedBuffer<double> h_sums;
    Event ev[2];
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<JointWorkspace> &g_workspaces = *new PerStream<JointWorkspace>();

struct JointCall {
    int w, h, n;
    const double *img, *var, *feat, *fvar;
    const double *const *comp, *const *comp_var;
    double *out, *var_out;
    double *const *comp_out, *const *comp_var_out;      // comp_var_out nullable
};

// one form of one instantiation, enqueued on `stream`
template <bool GUIDED, int NC>
void launch_form(const JointCall &c, const GdptNlmParams &p, const GdptNlmGuide &g, double *partials, bool direct, hipStream_t stream) {
    nlmj::Args<GUIDED, NC> a{};
    fill_base(a, c.w, c.h, p, c.img, c.var, c.out, c.var_out, partials);
    if constexpr (GUIDED) fill_guide(a.gd, g, c.feat, c.fvar, (size_t)c.w * c.h);
    for (int j = 0; j < NC; j++) {
        a.comp[j] = c.comp[j]; a.comp_var[j] = c.comp_var[j];
        a.comp_out[j] = c.comp_out[j]; a.comp_var_out[j] = c.comp_var_out ? c.comp_var_out[j] : nullptr;
    }
    if (direct) hipLaunchKernelGGL((nlmj::joint_direct_kernel<GUIDED, NC>), dim3(a.g.blocks), dim3(film::kBlock), 0, stream, a);
    else launch_staged(nlmj::joint_tiled_kernel<GUIDED, NC>, a.g.blocks, a.r, a.f, stream, a, "hipFuncSetAttribute(nlm joint stage)");
}

template <int NC>
void launch_count(const JointCall &c, const GdptNlmParams &p, const GdptNlmGuide &g, double *partials, bool direct, hipStream_t stream) {
    if (g.num_groups > 0) launch_form<true, NC>(c, p, g, partials, direct, stream);
    else launch_form<false, NC>(c, p, g, partials, direct, stream);
}

} // namespace

void denoise_nlm_joint_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, int n,
                              const double *const *d_comp, const double *const *d_comp_var, const GdptNlmParams &p, const GdptNlmGuide &g,
                              double *d_out, double *d_var_out, double *const *d_comp_out, double *const *d_comp_var_out, hipStream_t stream,
                              GdptNlmJointStats *stats) {
    if (n == 0) {                     // no companion: the guided filter itself, by its own kernels
        GdptNlmStats st{};
        denoise_nlm_guided_launch(w, h, d_img, d_var, d_feat, d_feat_var, p, g, d_out, d_var_out, stream, stats ? &st : nullptr);
        if (stats) { *stats = GdptNlmJointStats{}; stats->guide = st; }
        return;
    }
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    JointWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    if (!ws.partials) ws.partials.alloc((size_t)nlmj::kMaxRuns * film::kMaxBlocks, "hipMalloc(nlm joint partials)");
    if (!ws.d_sums) ws.d_sums.alloc(nlmj::kMaxRuns, "hipMalloc(nlm joint sums)");
    if (!ws.h_sums) ws.h_sums.alloc(nlmj::kMaxRuns, "hipHostMalloc(nlm joint sums)");
    for (auto &e : ws.ev) if (!e) e.create();

    const JointCall c{w, h, n, d_img, d_var, d_feat, d_feat_var, d_comp, d_comp_var, d_out, d_var_out, d_comp_out, d_comp_var_out};
    const int nb = film::tile_grid(w, h, kNlmTile, kNlmTile).blocks, runs = nlmj::kGuideRuns + 2 * n;
    const bool direct = debug_knob("nlm_direct", 0) != 0;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    switch (n) {
    case 1: launch_count<1>(c, p, g, ws.partials, direct, stream); break;
    case 2: launch_count<2>(c, p, g, ws.partials, direct, stream); break;
    case 3: launch_count<3>(c, p, g, ws.partials, direct, stream); break;
    default: launch_count<4>(c, p, g, ws.partials, direct, stream); break;
    }
    ck(hipGetLastError(), "nlm joint launch");
    if (!stats) return;
    film::launch_finish_runs(nb, runs, ws.partials, ws.d_sums, stream);
    ck(hipGetLastError(), "nlm joint reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_sums, ws.d_sums, runs * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(nlm joint sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(nlm joint)");
    *stats = GdptNlmJointStats{};
    const double *sums = ws.h_sums.data();
    GdptNlmStats &st = stats->guide;  // (runs 0 .. 5: nlm::leave_partials)
    st.pixels_left_out = (uint64_t)sums[2];
    st.sum_var_in = sums[0]; st.sum_sq_in = sums[1];
    st.sum_var_out = sums[3]; st.sum_sq_out = sums[4];
    st.error_in = std::sqrt(st.sum_var_in / st.sum_sq_in);
    st.error_out = std::sqrt(st.sum_var_out / st.sum_sq_out);
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); st.filter_ms = ms; }
    st.window_radius = p.window_radius; st.patch_radius = p.patch_radius;
    for (int j = 0; j < n; j++) {
        stats->sum_var_in[j] = sums[nlmj::kGuideRuns + 2 * j];
        stats->sum_var_out[j] = sums[nlmj::kGuideRuns + 2 * j + 1];
    }
}

// What both entry points refuse; `who` names the caller. Fills the parameters and the guide in force.
void nlm_joint_check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                               const double *feat_var, int n, const double *const *comp, const double *const *comp_var,
                               const GdptNlmParams *params, const GdptNlmGuide *guide, const double *out, const double *var_out,
                               double *const *comp_out, double *const *comp_var_out, GdptNlmParams &p, GdptNlmGuide &g) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    if (n < 0 || n > GDPT_NLM_JOINT_MAX) throw std::runtime_error(who + ": n must be in [0, " + std::to_string(GDPT_NLM_JOINT_MAX) + "]");
    if (n > 0) {
        if (!comp) throw std::runtime_error(who + ": comp is null");
        if (!comp_var) throw std::runtime_error(who + ": comp_var is null");
        if (!comp_out) throw std::runtime_error(who + ": comp_out is null");
        for (int j = 0; j < n; j++) {
            const std::string at = "[" + std::to_string(j) + "]";
            if (!comp[j]) throw std::runtime_error(who + ": comp" + at + " is null");
            if (!comp_var[j]) throw std::runtime_error(who + ": comp_var" + at + " is null");
            if (!comp_out[j]) throw std::runtime_error(who + ": comp_out" + at + " is null");
        }
    }
    if (params) p = *params;
    else gdpt_nlm_default_params(&p);
    nlm_check_params(who, p);
    if (guide) g = *guide;
    else gdpt_nlm_default_guide(&g);
    nlm_check_guide(who, g);
    if (g.num_groups > 0) {
        if (!feat) throw std::runtime_error(who + ": feat is null");
        if (!feat_var) throw std::runtime_error(who + ": feat_var is null");
    }
    // byte ranges: an output must not overlap an input or another output anywhere
    const size_t px = (size_t)width * height, film_bytes = px * 3 * sizeof(double), feat_bytes = px * (size_t)g.num_channels * sizeof(double);
    struct Range { std::string name; const void *p; size_t bytes; };
    std::vector<Range> ins{{"img", img, film_bytes}, {"var", var, film_bytes}}, outs{{"out", out, film_bytes}};
    if (feat) ins.push_back({"feat", feat, feat_bytes});
    if (feat_var) ins.push_back({"feat_var", feat_var, feat_bytes});
    if (var_out) outs.push_back({"var_out", var_out, film_bytes});
    for (int j = 0; j < n; j++) {
        const std::string at = "[" + std::to_string(j) + "]";
        ins.push_back({"comp" + at, comp[j], film_bytes});
        ins.push_back({"comp_var" + at, comp_var[j], film_bytes});
        outs.push_back({"comp_out" + at, comp_out[j], film_bytes});
        if (comp_var_out && comp_var_out[j]) outs.push_back({"comp_var_out" + at, comp_var_out[j], film_bytes});
    }
    auto overlap = [](const Range &a, const Range &b) {
        const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
        return x < y + b.bytes && y < x + a.bytes;
    };
    for (size_t i = 0; i < outs.size(); i++) {
        for (const Range &in : ins)
            if (overlap(outs[i], in)) throw std::runtime_error(who + ": " + outs[i].name + " must not alias an input (" + in.name + ")");
        for (size_t k = 0; k < i; k++)
            if (overlap(outs[i], outs[k])) throw std::runtime_error(who + ": " + outs[i].name + " must not alias " + outs[k].name);
    }
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

} // namespace

extern "C" {

int gdpt_denoise_nlm_joint_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                  int n, const double *const *d_comp, const double *const *d_comp_var, const GdptNlmParams *params,
                                  const GdptNlmGuide *guide, double *d_out, double *d_var_out, double *const *d_comp_out,
                                  double *const *d_comp_var_out, void *stream, GdptNlmJointStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_joint_device";
        GdptNlmParams p;
        GdptNlmGuide g;
        gdpt::nlm_joint_check_arguments(who, width, height, d_img, d_var, d_feat, d_feat_var, n, d_comp, d_comp_var, params, guide, d_out, d_var_out,
                                        d_comp_out, d_comp_var_out, p, g);
        need_a_device(who);
        gdpt::denoise_nlm_joint_launch(width, height, d_img, d_var, d_feat, d_feat_var, n, d_comp, d_comp_var, p, g, d_out, d_var_out, d_comp_out,
                                       d_comp_var_out, (hipStream_t)stream, stats);
    });
}

int gdpt_denoise_nlm_joint(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var, int n,
                           const double *const *comp, const double *const *comp_var, const GdptNlmParams *params, const GdptNlmGuide *guide,
                           double *out, double *var_out, double *const *comp_out, double *const *comp_var_out, GdptNlmJointStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_denoise_nlm_joint";
        GdptNlmParams p;
        GdptNlmGuide g;
        gdpt::nlm_joint_check_arguments(who, width, height, img, var, feat, feat_var, n, comp, comp_var, params, guide, out, var_out, comp_out,
                                        comp_var_out, p, g);
        need_a_device(who);
        gdpt::FilmMirrors m(width, height, img, var, feat, feat_var, g.num_groups > 0 ? (size_t)width * height * g.num_channels : 0, out, var_out);
        gdpt::Mirror m_comp[GDPT_NLM_JOINT_MAX], m_comp_var[GDPT_NLM_JOINT_MAX], m_comp_out[GDPT_NLM_JOINT_MAX], m_comp_var_out[GDPT_NLM_JOINT_MAX];
        const double *pc[GDPT_NLM_JOINT_MAX] = {}, *pcv[GDPT_NLM_JOINT_MAX] = {};
        double *pco[GDPT_NLM_JOINT_MAX] = {}, *pcvo[GDPT_NLM_JOINT_MAX] = {};
        for (int j = 0; j < n; j++) {
            m_comp[j].up(comp[j], m.elems); m_comp_var[j].up(comp_var[j], m.elems);
            m_comp_out[j].make(comp_out[j], m.elems);
            if (comp_var_out) m_comp_var_out[j].make(comp_var_out[j], m.elems);
            pc[j] = m_comp[j].d; pcv[j] = m_comp_var[j].d; pco[j] = m_comp_out[j].d; pcvo[j] = m_comp_var_out[j].d;
        }
        gdpt::denoise_nlm_joint_launch(width, height, m.img.d, m.var.d, m.feat.d, m.fvar.d, n, pc, pcv, p, g, m.out.d, m.var_out.d, pco, pcvo, nullptr, stats);
        m.down(out, var_out);
        for (int j = 0; j < n; j++) {
            m_comp_out[j].down(comp_out[j], m.elems);
            if (comp_var_out) m_comp_var_out[j].down(comp_var_out[j], m.elems);
        }
    });
}

} // extern "C"
