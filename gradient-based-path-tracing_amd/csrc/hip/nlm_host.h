// nlm_host.h — the host scaffold the non-local-means family shares (denoise_nlm.hip, nlm_joint.hip, nlm_regress.hip, nlm_collab.hip,
// denoise_atrous.hip, nlm_pyramid.hip): the sums workspace of a (device, stream) pair and the read-out of its statistics, the fills of
// the kernels' argument blocks from the blocks of include/gdpt.h, the launch of a kernel on the tiled form's stage, what every entry
// point refuses in its films, and the device copies of a host entry point's films.
#pragma once
#include "../../../include/gdpt.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"
#include "nlm_regress_device.h"

#include <cmath>
#include <mutex>
#include <string>

namespace gdpt {

// What a filter keeps per (device, stream) for its film sums. Each filter has a registry of its own (PerStream, device_mem.h).
struct SumsWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;    // six runs of block partials (nlm::leave_partials)
    DeviceBuffer<film::Estimate> d_est;     // [0] sum var in, sum u^2 in, left out; [1] sum var out, sum u^2 out, left out
    PinnedBuffer<film::Estimate> h_est;
    Event ev[2];                      // around the filter's launches, for filter_ms

    // `label` names the filter in an allocation's failure
    void prepare(const std::string &label) {
        if (!partials) partials.alloc(6 * film::kMaxBlocks, ("hipMalloc(" + label + " partials)").c_str());
        if (!d_est) d_est.alloc(2, ("hipMalloc(" + label + " sums)").c_str());
        if (!h_est) h_est.alloc(2, ("hipHostMalloc(" + label + " sums)").c_str());
        for (auto &e : ev) if (!e) e.create();
    }
    // After the filter's launches on `stream`, whose `nb` blocks left their partials, and with ev[0] recorded before them: the two
    // reductions, the wait for the stream, and the statistics but for the two radii.
    void read_stats(int nb, hipStream_t stream, const std::string &label, GdptNlmStats *stats) {
        film::launch_finish(nb, partials, d_est, stream);
        film::launch_finish(nb, partials.data() + 3 * nb, d_est.data() + 1, stream);
        ck(hipGetLastError(), (label + " reduction launch").c_str());
        ck(hipEventRecord(ev[1], stream), "hipEventRecord");
        ck(hipMemcpyAsync(h_est, d_est, 2 * sizeof(film::Estimate), hipMemcpyDeviceToHost, stream), ("hipMemcpyAsync(" + label + " sums)").c_str());
        ck(hipStreamSynchronize(stream), ("hipStreamSynchronize(" + label + ")").c_str());
        *stats = GdptNlmStats{};
        const film::Estimate &in = h_est.data()[0], &out = h_est.data()[1];
        stats->pixels_left_out = (uint64_t)in.left_out;
        stats->sum_var_in = in.sum_var; stats->sum_sq_in = in.sum_mean2;
        stats->sum_var_out = out.sum_var; stats->sum_sq_out = out.sum_mean2;
        stats->error_in = std::sqrt(in.sum_var / in.sum_mean2);
        stats->error_out = std::sqrt(out.sum_var / out.sum_mean2);
        { float ms = 0; ck(hipEventElapsedTime(&ms, ev[0], ev[1]), "hipEventElapsedTime"); stats->filter_ms = ms; }
    }
};

// the base fields of a kernel's argument block (nlm::Args and what derives from it)
template <class A>
void fill_base(A &a, int w, int h, const GdptNlmParams &p, const double *d_img, const double *d_var, double *d_out, double *d_var_out,
               double *partials) {
    a.g = film::tile_grid(w, h, kNlmTile, kNlmTile); a.r = p.window_radius; a.f = p.patch_radius;
    a.k2 = p.k * p.k; a.alpha = p.alpha; a.eps = p.epsilon;
    a.img = d_img; a.var = d_var; a.out = d_out; a.var_out = d_var_out; a.partials = partials;
}

// the guide of a guided kernel, on planes of `pixels` doubles; gd.used gains the channels the groups name
inline void fill_guide(nlm::Guide &gd, const GdptNlmGuide &g, const double *d_feat, const double *d_feat_var, size_t pixels) {
    gd.feat = d_feat; gd.fvar = d_feat_var; gd.plane = pixels;
    gd.groups = g.num_groups; gd.kf2 = g.k_f * g.k_f; gd.alpha_f = g.alpha_f;
    for (int j = 0; j < g.num_groups; j++) {
        const GdptNlmFeatureGroup &grp = g.groups[j];
        gd.first[j] = grp.first_channel; gd.count[j] = grp.num_channels; gd.tau[j] = grp.tau;
        for (int c = grp.first_channel; c < grp.first_channel + grp.num_channels; c++) gd.used |= 1u << c;
    }
}

// the regressors of a regression kernel; gd.used gains their channels
inline void fill_regress(nlmr::Regress &rg, nlm::Guide &gd, const GdptNlmRegress &r) {
    rg.m = r.num_regressors; rg.ridge = r.ridge;
    for (int j = 0; j < nlmr::kMaxM; j++) { rg.ch[j] = 0; rg.scale[j] = 1.0; }
    for (int j = 0; j < r.num_regressors; j++) { rg.ch[j] = r.channel[j]; rg.scale[j] = r.scale[j]; gd.used |= 1u << r.channel[j]; }
}

// a kernel of the tiled form on the stage of (r, f) (nlm::Stage), enqueued on `stream`; `label` names the failure of the LDS request
template <class K, class A>
void launch_staged(K kernel, int blocks, int r, int f, hipStream_t stream, const A &args, const char *label) {
    const size_t lds = (size_t)nlm::lds_doubles(r, f) * sizeof(double) + (size_t)nlm::lds_ints(r, f) * sizeof(int);
    ck(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), label);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(film::kBlock), lds, stream, args);
}

// what every entry point refuses in its films; `who` names the caller. var_out nullable.
inline void check_film(const std::string &who, int width, int height, const double *img, const double *var, const double *out, const double *var_out) {
    if (!img) throw std::runtime_error(who + ": img is null");
    if (!var) throw std::runtime_error(who + ": var is null");
    if (!out) throw std::runtime_error(who + ": out is null");
    if (out == img || out == var) throw std::runtime_error(who + ": out must not alias an input");
    if (var_out && (var_out == img || var_out == var || var_out == out)) throw std::runtime_error(who + ": var_out must not alias an input or out");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
}

// A host array's copy on the device, for a host entry point: up() makes and fills an input's, make() an output's, down() brings it
// back. A null host pointer or a count of 0 leaves it empty: a null device pointer.
struct Mirror {
    DeviceBuffer<double> d;
    void up(const double *host, size_t n) {
        if (!host || n == 0) return;
        d.alloc(n, "hipMalloc(film io)");
        ck(hipMemcpy(d, host, n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(H2D)");
    }
    void make(const double *host, size_t n) { if (host) d.alloc(n, "hipMalloc(film io)"); }
    void down(double *host, size_t n) const { if (host && n) ck(hipMemcpy(host, d, n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)"); }
};

// the films every filter's host entry point mirrors: img, var and the feature planes up, out and var_out (nullable) down
struct FilmMirrors {
    Mirror img, var, feat, fvar, out, var_out;
    size_t elems;
    // feature_elems: 0 where the call reads no plane
    FilmMirrors(int width, int height, const double *h_img, const double *h_var, const double *h_feat, const double *h_feat_var,
                size_t feature_elems, const double *h_out, const double *h_var_out) : elems((size_t)width * height * 3) {
        img.up(h_img, elems); var.up(h_var, elems); feat.up(h_feat, feature_elems); fvar.up(h_feat_var, feature_elems);
        out.make(h_out, elems); var_out.make(h_var_out, elems);
    }
    void down(double *h_out, double *h_var_out) const { out.down(h_out, elems); var_out.down(h_var_out, elems); }
};

} // namespace gdpt
