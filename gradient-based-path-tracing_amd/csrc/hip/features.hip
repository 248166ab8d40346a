// features.hip — first-hit feature buffers with per-pixel variances (include/gdpt.h: gdpt_features_render*, where the definition
// stands; Rousselle, Manzi, Zwicker 2013, section 3): albedo, shading normal, depth and coverage of the render's own base primary
// rays, folded per pixel in sample order.
//
// Kernel: a thread on a pixel, 16 x 16 tiles over the band through film::tile_grid (a film past the block cap takes further trips),
// the camera ray and the vertex made by the render kernels' own code (sample_primary, intersect_ctx / make_vertex, tex3). Two
// instantiations, as the render kernels have them: the scene copied to LDS with the fixed stack column (setup_trace<true, true>, the
// whole-leaf walk of render_twosided.h) where scene_fits_lds_wide says so, and the walk from HBM with the eager kernel's stack of
// GDPT_BVH_MAX_DEPTH slots per lane otherwise, or under the test knob no_lds_scene. A pixel's 16 running values (8 means, 8 sums of
// squared deviations) stay in registers; nothing is shared between pixels, so the two forms, and any cut into bands, give the same bits.
// It is no render route: it takes none of the handle's launch scratch and leaves gdpt_debug_last_route alone.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "render_device.h"
#include "scene_internal.h"

#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>

namespace feat {

constexpr int kTile = 16, kPlanes = GDPT_FEATURE_CHANNELS;
static_assert(kTile * kTile == film::kBlock && film::kBlock == gd::kBlock, "one thread per tile pixel");

struct Args {
    film::TileGrid g;                  // 16 x 16 tiles over the band's rows
    int row_begin, row_end;
    int spp, stream_spp, first_sample;
    double *mean, *var;                // 8 planes of W H doubles each
    unsigned long long *rays;          // nullable: primary rays traced
};

// the eight values of one sample of pixel (x, y): 0 on a miss
template <class TC>
__device__ __forceinline__ void sample_features(const DevSceneView &sv, const gd::TraceCtx &tx, int x, int y, gd::Pcg &rng, double f[kPlanes],
                                                gd::LaneCounters &lc, gd::TraceCounters &tc) {
    const DevCamera &cam = sv.cam;
    const int w = cam.width, h = cam.height;
    const double rx = gd::pcg_real(rng), ry = gd::pcg_real(rng);
    const gd::Ray ray = gd::sample_primary(cam, (x + rx) / w, (y + ry) / h);       // (grad_sample_eager's base ray)
    const double rd_spread = 0.25 / (double)max(w, h);
    gd::Vertex v;
#pragma unroll
    for (int c = 0; c < kPlanes; c++) f[c] = 0.0;
    if (!gd::intersect_ctx<TC>(sv, tx, ray, rd_spread, v, lc, tc)) return;
    const GdptMaterial &m = tx.materials[v.material_id];
    const gd::D3 albedo = m.type == GDPT_MAT_DISNEY_CLEARCOAT ? gd::splat(1.0) : gd::tex3(sv, m.tex[0], v);
    const gd::D3 dl = v.position - ray.org;
    f[0] = albedo.x; f[1] = albedo.y; f[2] = albedo.z;
    f[3] = v.frame.n.x; f[4] = v.frame.n.y; f[5] = v.frame.n.z;
    f[6] = sqrt(gd::dot(dl, dl));
    f[7] = 1.0;
}

template <bool LDS_SCENE>
__global__ __launch_bounds__(gd::kBlock, 2) void features_kernel(DevSceneView sv, Args a) {
    using TC = typename std::conditional<LDS_SCENE, gd::TraceCfg<true, true, false>, gd::TraceHbm>::type;
    __shared__ int s_stack[(LDS_SCENE ? gd::kLdsSceneLevels : GDPT_BVH_MAX_DEPTH) * gd::kBlock];
    __shared__ __attribute__((aligned(16))) unsigned char s_scene[LDS_SCENE ? gd::kLdsSceneBytes : 16];
    const int tid = threadIdx.x;
    const gd::TraceCtx tx = gd::setup_trace<LDS_SCENE, true>(sv, s_scene, s_stack, tid, gd::kBlock, false);
    const int W = sv.cam.width;
    const size_t plane = (size_t)W * sv.cam.height;
    gd::LaneCounters lc = {0, 0, 0};
    gd::TraceCounters tc = {0, 0, 0, 0, 0, 0};
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const film::TilePixel tp = film::tile_pixel<kTile, kTile>(a.g, t);
        const int x = tp.x, y = a.row_begin + tp.y;
        if (x >= W || y >= a.row_end) continue;
        const unsigned long long base = ((unsigned long long)y * W + x) * (unsigned long long)a.stream_spp + (unsigned long long)a.first_sample;
        double mean[kPlanes], m2[kPlanes];
#pragma unroll
        for (int c = 0; c < kPlanes; c++) { mean[c] = 0.0; m2[c] = 0.0; }
        for (int s = 0; s < a.spp; s++) {
            gd::Pcg rng = gd::pcg_init(base + (unsigned long long)s);
            double f[kPlanes];
            sample_features<TC>(sv, tx, x, y, rng, f, lc, tc);
            const double i = (double)(s + 1);
#pragma unroll
            for (int c = 0; c < kPlanes; c++) {          // (one rounding per operation: the products below are not contracted into the sums)
                const double d = f[c] - mean[c];
                const double q = d / i;
                mean[c] += q;
                const double e = f[c] - mean[c];
                const double p = d * e;
                m2[c] += p;
            }
        }
        const size_t i = (size_t)y * W + x;
        const double n = (double)a.spp, den = n * (n - 1.0);
#pragma unroll
        for (int c = 0; c < kPlanes; c++) {
            a.mean[c * plane + i] = mean[c];
            a.var[c * plane + i] = a.spp > 1 ? m2[c] / den : 0.0;
        }
    }
    if (a.rays) {
        const unsigned r = gd::wave_sum_u32(lc.rays);
        if ((tid & 63) == 0 && r) atomicAdd(a.rays, (unsigned long long)r);
    }
}

} // namespace feat

namespace {

using gdpt::ck;
using gdpt::need_a_device;

struct FeatureWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    gdpt::DeviceBuffer<unsigned long long> d_rays;
    gdpt::PinnedBuffer<unsigned long long> h_rays;
    gdpt::Event ev[2];
};
// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
gdpt::PerStream<FeatureWorkspace> &g_workspaces = *new gdpt::PerStream<FeatureWorkspace>();

struct Call { int spp, row_begin, row_end, stream_spp, first_sample; };

// What is refused on the values of the arguments alone, before the scene handle is read; `who` names the caller.
void check_fields(const std::string &who, const GdptScene *scene, const GdptRenderParams *p, const GdptSampleWindow *win, const double *mean,
                  const double *var) {
    if (!scene) throw std::runtime_error(who + ": scene is null");
    if (!mean) throw std::runtime_error(who + ": mean is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (mean == var) throw std::runtime_error(who + ": var must not alias mean");
    if (p) {
        if (p->rng_scheme == GDPT_RNG_TILE) throw std::runtime_error(who + ": rng_scheme: GDPT_RNG_TILE is refused (GDPT_RNG_SAMPLE only)");
        if (p->rng_scheme != GDPT_RNG_SAMPLE) throw std::runtime_error(who + ": rng_scheme must be GDPT_RNG_SAMPLE");
        if (p->shift_mode != 0) throw std::runtime_error(who + ": shift_mode must be 0");
        if (p->reserved != 0) throw std::runtime_error(who + ": reserved must be 0");
        if (p->row_begin < 0 || p->row_end < 0 || ((p->row_begin != 0 || p->row_end != 0) && p->row_begin >= p->row_end))
            throw std::runtime_error(who + ": row_begin, row_end: bad row band");
    }
    if (win) {
        if (win->stream_spp <= 0) throw std::runtime_error(who + ": window stream_spp must be > 0");
        if (win->first_sample < 0) throw std::runtime_error(who + ": window first_sample must be >= 0");
        if (p && p->spp > 0 && (long long)win->first_sample + p->spp > (long long)win->stream_spp)
            throw std::runtime_error(who + ": window [first_sample, first_sample + spp) must lie inside [0, stream_spp)");
    }
}

// ... and what needs the handle: the samples per pixel, the band against the film, the stream block against 63 bits
Call resolve_call(const std::string &who, const GdptScene *sc, const GdptRenderParams *p, const GdptSampleWindow *win) {
    const int W = sc->view.cam.width, H = sc->view.cam.height;
    Call c;
    c.spp = (p && p->spp > 0) ? p->spp : sc->scene_spp;
    if (c.spp <= 0) throw std::runtime_error(who + ": spp: samples per pixel must be > 0");
    c.row_begin = p ? p->row_begin : 0; c.row_end = p ? p->row_end : 0;
    if (c.row_begin == 0 && c.row_end == 0) c.row_end = H;
    if (c.row_end > H) throw std::runtime_error(who + ": row_end: the band leaves the film");
    c.stream_spp = c.spp; c.first_sample = 0;
    if (win) {
        if ((long long)win->first_sample + c.spp > (long long)win->stream_spp)
            throw std::runtime_error(who + ": window [first_sample, first_sample + spp) must lie inside [0, stream_spp)");
        c.stream_spp = win->stream_spp; c.first_sample = win->first_sample;
    }
    // the largest stream index, W * H * stream_spp - 1, goes through pcg_init's (index << 1) | 1
    if ((unsigned long long)W * (unsigned long long)H > (~0ull >> 1) / (unsigned long long)c.stream_spp)
        throw std::runtime_error(who + ": width * height * stream_spp does not fit 63 bits");
    return c;
}

} // namespace

namespace gdpt {

// Device pointers on the scene's device; the arguments have been checked. Enqueued on `stream`; waits for it if `stats` is asked for.
void features_launch(GdptScene *sc, const GdptRenderParams *params, const GdptSampleWindow *window, double *d_mean, double *d_var,
                     hipStream_t stream, GdptRenderStats *stats) {
    const std::string who = "gdpt_features_render";
    const Call c = resolve_call(who, sc, params, window);
    ck(hipSetDevice(sc->device), "hipSetDevice");
    const DevSceneView &v = sc->view;
    FeatureWorkspace &ws = g_workspaces.get(sc->device, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    feat::Args a{};
    a.g = film::tile_grid(v.cam.width, c.row_end - c.row_begin, feat::kTile, feat::kTile);
    a.row_begin = c.row_begin; a.row_end = c.row_end;
    a.spp = c.spp; a.stream_spp = c.stream_spp; a.first_sample = c.first_sample;
    a.mean = d_mean; a.var = d_var; a.rays = nullptr;
    if (stats) {
        if (!ws.d_rays) ws.d_rays.alloc(1, "hipMalloc(feature counters)");
        if (!ws.h_rays) ws.h_rays.alloc(1, "hipHostMalloc(feature counters)");
        for (auto &e : ws.ev) if (!e) e.create();
        ck(hipMemsetAsync(ws.d_rays, 0, sizeof(unsigned long long), stream), "hipMemsetAsync(feature counters)");
        a.rays = ws.d_rays;
        ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    }
    if (sc->traits.wide_stack_need > GDPT_BVH_MAX_DEPTH) throw std::runtime_error(who + ": traversal stack bound exceeds the builder's maximum");
    const bool lds = scene_fits_lds_wide(v.num_nodes4, v.num_prims, v.num_tris, v.num_materials, v.num_lights, sc->traits.wide_stack_need) &&
                     debug_knob_int("no_lds_scene", 0) == 0;
    // The kernel reads the scene's immutable tables and writes the caller's two arrays, nothing of the handle's: it goes on `stream`
    // as it is, with no join of the handle's render streams and no claim on its launch scratch (capi_device.hip: claim_scratch).
    if (lds) hipLaunchKernelGGL(feat::features_kernel<true>, dim3(a.g.blocks), dim3(gd::kBlock), 0, stream, v, a);
    else hipLaunchKernelGGL(feat::features_kernel<false>, dim3(a.g.blocks), dim3(gd::kBlock), 0, stream, v, a);
    ck(hipGetLastError(), "features launch");
    if (!stats) return;
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_rays, ws.d_rays, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(feature counters)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(features)");
    *stats = GdptRenderStats{};
    stats->samples = (uint64_t)v.cam.width * (uint64_t)(c.row_end - c.row_begin) * (uint64_t)c.spp;
    stats->rays = *ws.h_rays.data();
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->render_ms = ms; }
}

} // namespace gdpt

extern "C" {

int gdpt_features_render_device(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window, double *d_mean, double *d_var,
                                void *stream, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_features_render_device";
        check_fields(who, scene, params, window, d_mean, d_var);
        need_a_device(who);
        gdpt::features_launch(scene, params, window, d_mean, d_var, (hipStream_t)stream, stats);
    });
}

int gdpt_features_render(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window, double *mean, double *var,
                         GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_features_render";
        check_fields(who, scene, params, window, mean, var);
        need_a_device(who);
        ck(hipSetDevice(scene->device), "hipSetDevice");
        const int W = scene->view.cam.width, H = scene->view.cam.height;
        const size_t elems = (size_t)W * H * GDPT_FEATURE_CHANNELS, bytes = elems * sizeof(double);
        gdpt::DeviceBuffer<double> d_mean, d_var;
        d_mean.alloc(elems, "hipMalloc(feature planes)"); d_var.alloc(elems, "hipMalloc(feature planes)");
        // rows outside the band keep the caller's contents: upload them first when rendering a partial band
        const bool partial = params && (params->row_begin != 0 || params->row_end != 0) && !(params->row_begin == 0 && params->row_end == H);
        if (partial) {
            ck(hipMemcpy(d_mean, mean, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            ck(hipMemcpy(d_var, var, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        }
        GdptRenderStats local{};
        gdpt::features_launch(scene, params, window, d_mean, d_var, nullptr, stats ? stats : &local);
        ck(hipMemcpy(mean, d_mean, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        ck(hipMemcpy(var, d_var, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
