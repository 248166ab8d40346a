// progressive_group.hip — a progressive session whose samples are split over several devices (include/gdpt.h:
// gdpt_progressive_group_*): one slice session per device, and a total that is the merge of all of them.
//
// Why the cut is on the sample axis. The row-band host (multi_gpu.hip) equalises cost per ROW: it needs a halo row, an all-gather
// of three images, a pilot render and a rebalance loop. A session already has an axis on which every cut costs the same: pass k
// draws a window of every pixel's block of budget_spp streams, and that window is all that identifies its samples. Member i owns
// the slice [floor(i B / N), floor((i+1) B / N)) of the budget B; every member renders the whole film, the same work per sample, so
// nothing is balanced, and the only traffic is the members' (mean, M2) planes going to the total's device when it is rebuilt.
//
// A round: every member with budget left adds one pass, one host thread per member (the caller drives member 0). The threads share
// nothing and wait for nothing but their own device: a member that fails cannot leave another one waiting; its error is reported
// after all threads have been joined. Then the total (an accumulator on devices[0]) is emptied and all members are merged into it in
// member order (prg::merge, progressive.hip), so its bits do not depend on which member finished first.
//
// The error of the reconstruction (gdpt_progressive_group_reconstruct_error, _run_recon). The members are N independent estimates of
// the film, so their reconstructions are too: every member that holds samples reconstructs its own running means on its own device
// and stream (threads as in a round), the images of members on other devices are copied to devices[0], the total is reconstructed
// there, and recon_spread.hip takes the weighted spread of the members' images around their mean on the total's stream. Nothing of
// the render, the fold or the merge takes part.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "progressive_internal.h"
#include "filter_select.h"
#include "recon_spread.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <thread>

namespace {

using gdpt::ck;

struct Member {
    int device = 0;
    std::unique_ptr<GdptScene> scene;
    hipStream_t stream = nullptr;
    GdptProgressive *session = nullptr;
    std::string error;
};

} // namespace

struct GdptProgressiveGroup {
    std::vector<Member> members;
    hipStream_t total_stream = nullptr;
    GdptProgressive *total = nullptr;
    bool total_current = true;       // the total holds what the members hold
    GdptProgressive *half[2] = {nullptr, nullptr};     // accumulators beside the total, on its device and stream: the members that hold samples,
    bool halves_current = false;                       // in member order, merged alternately into [0] and [1] (gdpt_progressive_group_halves)
    std::vector<gdpt::DeviceBuffer<double>> recon_stage;     // on devices[0]: reconstructions of members on other devices, allocated on first use
    std::vector<gdpt::DeviceBuffer<double>> select_films;    // on devices[0]: gdpt_progressive_group_denoise_select's 3n filtered films, the halves' four planes,
    gdpt::DeviceBuffer<double> select_out, select_mse, select_feat[2];      // its outputs on their way to host memory; allocated on first use
    gdpt::DeviceBuffer<int32_t> select_sel;
    gdpt::DeviceBuffer<double> spread_var, spread_map;       // on devices[0]: the statistic's planes on their way to host memory, allocated on first use

    ~GdptProgressiveGroup() {
        for (GdptProgressive *h : half) if (h) gdpt_progressive_free(h);
        if (total) gdpt_progressive_free(total);
        for (Member &m : members) if (m.session) gdpt_progressive_free(m.session);
        if (!members.empty()) {
            hipSetDevice(members[0].device);
            recon_stage.clear(); spread_var.reset(); spread_map.reset();
            select_films.clear(); select_out.reset(); select_mse.reset(); select_sel.reset(); select_feat[0].reset(); select_feat[1].reset();
        }
        if (total_stream && !members.empty()) {
            gdpt::forget_stream(members[0].device, total_stream);     // the solvers' and reconstructions' per-stream scratch goes with the stream
            hipStreamDestroy(total_stream);
        }
        for (Member &m : members) {
            hipSetDevice(m.device);
            if (m.stream) hipStreamDestroy(m.stream);
            m.scene.reset();
        }
    }
};

namespace {

void rebuild_total(GdptProgressiveGroup &g) {
    prg::reset(*g.total);
    for (Member &m : g.members) prg::merge(*g.total, *m.session);
    g.total_current = true;
}

// one pass of every member with budget left; false when no member had any
bool round(GdptProgressiveGroup &g, int pass_spp) {
    std::vector<int> todo;
    for (int i = 0; i < (int)g.members.size(); i++) {
        g.members[(size_t)i].error.clear();
        const GdptProgressive &s = *g.members[(size_t)i].session;
        if (s.own_done < s.own) todo.push_back(i);
    }
    if (todo.empty()) return false;
    auto one = [&](int i) {
        Member &m = g.members[(size_t)i];
        try {
            GdptProgressive &s = *m.session;
            prg::add_pass(s, std::min(pass_spp, s.own - s.own_done), nullptr);
        } catch (const std::exception &e) { m.error = e.what(); }
        catch (...) { m.error = "unknown error"; }
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < todo.size(); k++) th.emplace_back(one, todo[k]);
    one(todo[0]);
    for (std::thread &t : th) t.join();
    g.total_current = g.halves_current = false;
    for (int i : todo) {
        const Member &m = g.members[(size_t)i];
        if (!m.error.empty()) throw std::runtime_error("device " + std::to_string(m.device) + " (member " + std::to_string(i) + "): " + m.error);
    }
    return true;
}

// the members that hold samples
std::vector<int> members_with_samples(const GdptProgressiveGroup &g) {
    std::vector<int> used;
    for (int i = 0; i < (int)g.members.size(); i++) if (g.members[(size_t)i].session->done > 0) used.push_back(i);
    return used;
}

// "" if the estimate can be taken now, else why not
std::string cannot_estimate(const GdptProgressiveGroup &g, const GdptGroupReconParams &p) {
    const std::vector<int> used = members_with_samples(g);
    if (used.size() < 2)
        return std::to_string(used.size()) + " of " + std::to_string(g.members.size()) + " members hold samples: the spread needs two independent estimates";
    if (p.weighted)
        for (int i : used)
            if (g.members[(size_t)i].session->passes < 2)
                return "member " + std::to_string(i) + " holds " + std::to_string(g.members[(size_t)i].session->passes) +
                       " pass: the variance-weighted reconstruction needs at least 2 in every member";
    return "";
}

void check_recon_params(const char *fn, const GdptProgressiveGroup &g, const GdptGroupReconParams *p) {
    const std::string who(fn);
    if (!p) throw std::runtime_error(who + ": null params");
    if (g.total->nbuf != 5) throw std::runtime_error(who + ": an Integrator::Path group has no gradients to reconstruct (GradPath groups only)");
    if (p->map_radius < 0 || p->map_radius > 8) throw std::runtime_error(who + ": map_radius must be in [0, 8]");
    if (p->weighted != 0 && p->weighted != 1) throw std::runtime_error(who + ": weighted must be 0 or 1");
}

// Every member used reconstructs, then the total, then the spread; the outputs (all nullable) as the entry point's. The total is current.
gdpt::ReconSpreadResult reconstruct_error(GdptProgressiveGroup &g, const GdptGroupReconParams &p, int on_device, double *out_image, double *out_map,
                                          double *out_var, GdptReconStats *recon_stats, int *num_used) {
    const std::vector<int> used = members_with_samples(g);
    for (int i : used) g.members[(size_t)i].error.clear();
    auto one = [&](int i) {
        Member &m = g.members[(size_t)i];
        try {
            GdptProgressive &s = *m.session;
            if (p.weighted) prg::reconstruct_weighted(s, p.dataCost, &p.wrecon, nullptr, nullptr);
            else prg::reconstruct(s, p.dataCost, &p.recon, nullptr);
            ck(hipStreamSynchronize(s.stream), "hipStreamSynchronize(member reconstruction)");
        } catch (const std::exception &e) { m.error = e.what(); }
        catch (...) { m.error = "unknown error"; }
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < used.size(); k++) th.emplace_back(one, used[k]);
    one(used[0]);
    for (std::thread &t : th) t.join();
    for (int i : used) {
        const Member &m = g.members[(size_t)i];
        if (!m.error.empty()) throw std::runtime_error("device " + std::to_string(m.device) + " (member " + std::to_string(i) + "): " + m.error);
    }

    GdptProgressive &t = *g.total;
    ck(hipSetDevice(t.device), "hipSetDevice");
    std::vector<const double *> images;
    std::vector<double> weights;
    g.recon_stage.resize(g.members.size());
    for (int i : used) {
        const GdptProgressive &s = *g.members[(size_t)i].session;
        const double *img = s.asm_buf[3];
        if (s.device != t.device) {          // into staging on the total's device, on the total's stream (as prg::merge copies the planes)
            int can = 0;
            ck(hipDeviceCanAccessPeer(&can, t.device, s.device), "hipDeviceCanAccessPeer");
            if (can) {
                const hipError_t e = hipDeviceEnablePeerAccess(s.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ck(e, "hipDeviceEnablePeerAccess");
                (void)hipGetLastError();
            }
            gdpt::DeviceBuffer<double> &st = g.recon_stage[(size_t)i];
            if (!st) st.alloc(t.elems, "hipMalloc(group reconstruction staging)");
            ck(hipMemcpyPeerAsync(st, t.device, img, s.device, t.elems * sizeof(double), t.stream), "hipMemcpyPeerAsync(member reconstruction)");
            img = st;
        }
        images.push_back(img);
        weights.push_back((double)s.done);
    }
    if (p.weighted) {
        GdptWeightedReconStats ws{};
        prg::reconstruct_weighted(t, p.dataCost, &p.wrecon, nullptr, &ws);
        if (recon_stats) *recon_stats = ws.recon;
    } else
        prg::reconstruct(t, p.dataCost, &p.recon, recon_stats);

    double *d_var = out_var, *d_map = out_map;
    if (!on_device) {
        if (out_var) { if (!g.spread_var) g.spread_var.alloc(t.elems, "hipMalloc(group spread planes)"); d_var = g.spread_var; }
        if (out_map) { if (!g.spread_map) g.spread_map.alloc(t.elems / 3, "hipMalloc(group spread planes)"); d_map = g.spread_map; }
    }
    const gdpt::ReconSpreadResult res = gdpt::recon_spread_device(t.w, t.h, (int)images.size(), images.data(), weights.data(), t.asm_buf[3], p.map_radius,
                                                                  d_var, d_map, t.stream);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_image) ck(hipMemcpyAsync(out_image, t.asm_buf[3], t.elems * sizeof(double), kind, t.stream), "hipMemcpyAsync(group reconstruction)");
    if (!on_device) {
        if (out_var) ck(hipMemcpyAsync(out_var, d_var, t.elems * sizeof(double), kind, t.stream), "hipMemcpyAsync(group spread planes)");
        if (out_map) ck(hipMemcpyAsync(out_map, d_map, t.elems / 3 * sizeof(double), kind, t.stream), "hipMemcpyAsync(group spread planes)");
    }
    ck(hipStreamSynchronize(t.stream), "hipStreamSynchronize(group reconstruction)");
    if (num_used) *num_used = (int)used.size();
    return res;
}

} // namespace

extern "C" {

int gdpt_progressive_group_create(const GdptSceneDesc *desc, const int32_t *devices, int num_devices, const GdptProgressiveConfig *config,
                                  GdptProgressiveGroup **out) {
    return gdpt::guarded([&]() {
        if (!desc || !devices || !out) throw std::runtime_error("gdpt_progressive_group_create: null argument");
        if (num_devices <= 0 || num_devices > GDPT_MULTI_MAX_DEVICES) throw std::runtime_error("gdpt_progressive_group_create: num_devices out of range");
        int ndev = 0;
        ck(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
        if (ndev <= 0) throw std::runtime_error("gdpt_progressive_group_create: no HIP device visible (this library has no CPU fallback)");
        const int n = num_devices;
        for (int i = 0; i < n; i++)
            if (devices[i] < 0 || devices[i] >= ndev)
                throw std::runtime_error("gdpt_progressive_group_create: device " + std::to_string(devices[i]) + " asked for, " + std::to_string(ndev) + " visible");
        GdptProgressiveConfig cfg = config ? *config : GdptProgressiveConfig{};
        if (cfg.budget_spp <= 0) cfg.budget_spp = desc->samples_per_pixel;      // the block must be one number for all members
        if (cfg.budget_spp <= 0) throw std::runtime_error("gdpt_progressive_group_create: budget_spp must be > 0");
        std::unique_ptr<GdptProgressiveGroup> g(new GdptProgressiveGroup());
        g->members.resize((size_t)n);
        {   // every member gets its own copy of the scene, made from one prepared scene
            std::vector<std::unique_ptr<GdptScene>> scenes = gdpt::upload_scenes(desc, devices, n);
            for (int i = 0; i < n; i++) { g->members[(size_t)i].device = devices[i]; g->members[(size_t)i].scene = std::move(scenes[(size_t)i]); }
        }
        const long long B = cfg.budget_spp;
        for (int i = 0; i < n; i++) {
            Member &m = g->members[(size_t)i];
            ck(hipSetDevice(m.device), "hipSetDevice");
            ck(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking), "hipStreamCreate");
            const int first = (int)(i * B / n), end = (int)((i + 1) * B / n);
            if (gdpt_progressive_create_slice(m.scene.get(), &cfg, first, end - first, m.stream, &m.session) != 0)
                throw std::runtime_error(gdpt_last_error());
        }
        ck(hipSetDevice(g->members[0].device), "hipSetDevice");
        ck(hipStreamCreateWithFlags(&g->total_stream, hipStreamNonBlocking), "hipStreamCreate");
        if (gdpt_progressive_create_slice(g->members[0].scene.get(), &cfg, 0, 0, g->total_stream, &g->total) != 0)
            throw std::runtime_error(gdpt_last_error());
        g->total->group_total = true;
        for (GdptProgressive *&h : g->half) {
            if (gdpt_progressive_create_slice(g->members[0].scene.get(), &cfg, 0, 0, g->total_stream, &h) != 0)
                throw std::runtime_error(gdpt_last_error());
            h->group_total = h->group_half = true;
        }
        *out = g.release();
    });
}

void gdpt_progressive_group_free(GdptProgressiveGroup *group) { delete group; }

int gdpt_progressive_group_run(GdptProgressiveGroup *group, double target_error, int pass_spp, int max_rounds, GdptProgressiveStatus *status) {
    return gdpt::guarded([&]() {
        if (!group) throw std::runtime_error("gdpt_progressive_group_run: null group");
        if (pass_spp <= 0) throw std::runtime_error("gdpt_progressive_group_run: pass_spp must be > 0");
        if (std::isnan(target_error)) throw std::runtime_error("gdpt_progressive_group_run: target_error is NaN");
        GdptProgressiveGroup &g = *group;
        GdptProgressive &t = *g.total;
        auto spent = [&]() {
            for (const Member &m : g.members) if (m.session->own_done < m.session->own) return false;
            return true;
        };
        if (!g.total_current) rebuild_total(g);          // (an earlier call failed between a round and its rebuild)
        int rounds = 0, why = GDPT_STOP_NONE;
        for (;;) {
            if (target_error > 0 && t.passes >= 2 && prg::error_estimate(t) <= target_error) { why = GDPT_STOP_TARGET; break; }
            if (spent()) { why = GDPT_STOP_BUDGET; break; }
            if (max_rounds > 0 && rounds >= max_rounds) { why = GDPT_STOP_MAX_PASSES; break; }
            round(g, pass_spp);
            rounds++;
            if (target_error > 0) rebuild_total(g);
        }
        if (!g.total_current) rebuild_total(g);
        t.stop_reason = why;
        prg::fill_status(t, status);
    });
}

int gdpt_progressive_group_reconstruct_error(GdptProgressiveGroup *group, const GdptGroupReconParams *params, int on_device, double *out_image,
                                             double *out_map, double *out_var, GdptReconSpreadStats *spread_stats, GdptReconStats *recon_stats) {
    return gdpt::guarded([&]() {
        const char *fn = "gdpt_progressive_group_reconstruct_error";
        if (!group || !out_image) throw std::runtime_error(std::string(fn) + ": null argument");
        GdptProgressiveGroup &g = *group;
        check_recon_params(fn, g, params);
        if (!g.total_current) rebuild_total(g);
        const std::string why = cannot_estimate(g, *params);
        if (!why.empty()) throw std::runtime_error(std::string(fn) + ": " + why);
        int n = 0;
        const gdpt::ReconSpreadResult r = reconstruct_error(g, *params, on_device, out_image, out_map, out_var, recon_stats, &n);
        gdpt::fill_spread_stats(spread_stats, n, params->map_radius, r);
    });
}

int gdpt_progressive_group_run_recon(GdptProgressiveGroup *group, double target_recon_error, int pass_spp, int max_rounds, int check_every,
                                     const GdptGroupReconParams *params, GdptProgressiveStatus *status, GdptReconSpreadStats *spread_stats) {
    return gdpt::guarded([&]() {
        const char *fn = "gdpt_progressive_group_run_recon";
        if (!group) throw std::runtime_error(std::string(fn) + ": null group");
        if (pass_spp <= 0) throw std::runtime_error(std::string(fn) + ": pass_spp must be > 0");
        if (std::isnan(target_recon_error)) throw std::runtime_error(std::string(fn) + ": target_recon_error is NaN");
        GdptProgressiveGroup &g = *group;
        check_recon_params(fn, g, params);
        GdptProgressive &t = *g.total;
        const int every = check_every <= 0 ? 1 : check_every;
        auto spent = [&]() {
            for (const Member &m : g.members) if (m.session->own_done < m.session->own) return false;
            return true;
        };
        // the estimate of the state the members hold now; false where it cannot be taken yet
        GdptReconSpreadStats est{};
        bool est_current = false;
        auto evaluate = [&]() {
            if (!g.total_current) rebuild_total(g);
            if (est_current) return true;
            if (!cannot_estimate(g, *params).empty()) return false;
            int n = 0;
            const gdpt::ReconSpreadResult r = reconstruct_error(g, *params, 1, nullptr, nullptr, nullptr, nullptr, &n);
            gdpt::fill_spread_stats(&est, n, params->map_radius, r);
            est_current = true;
            return true;
        };
        int rounds = 0, why = GDPT_STOP_NONE;
        for (;;) {
            if (target_recon_error > 0 && est_current && est.error_estimate <= target_recon_error) { why = GDPT_STOP_TARGET; break; }
            if (spent()) { why = GDPT_STOP_BUDGET; break; }
            if (max_rounds > 0 && rounds >= max_rounds) { why = GDPT_STOP_MAX_PASSES; break; }
            round(g, pass_spp);
            rounds++;
            est_current = false;
            if (target_recon_error > 0 && rounds % every == 0) evaluate();
        }
        if (!evaluate()) est = GdptReconSpreadStats{};
        t.stop_reason = why;
        prg::fill_status(t, status);
        if (spread_stats) *spread_stats = est;
    });
}

GdptProgressive *gdpt_progressive_group_total(GdptProgressiveGroup *group) { return group ? group->total : nullptr; }

int gdpt_progressive_group_halves(GdptProgressiveGroup *group, GdptProgressive **half_a, GdptProgressive **half_b) {
    return gdpt::guarded([&]() {
        const char *fn = "gdpt_progressive_group_halves";
        if (!group || !half_a || !half_b) throw std::runtime_error(std::string(fn) + ": null argument");
        GdptProgressiveGroup &g = *group;
        const std::vector<int> used = members_with_samples(g);
        if (used.size() < 2)
            throw std::runtime_error(std::string(fn) + ": two halves need at least two members that hold samples (" + std::to_string(used.size()) + " do)");
        if (!g.halves_current) {
            for (GdptProgressive *h : g.half) prg::reset(*h);
            for (size_t k = 0; k < used.size(); k++) prg::merge(*g.half[k & 1], *g.members[(size_t)used[k]].session);
            g.halves_current = true;
        }
        *half_a = g.half[0]; *half_b = g.half[1];
    });
}

// whether the candidate's session entry renders feature planes
static bool renders_features(const GdptSelectCandidate &c) {
    return c.filter == GDPT_SELECT_NLM_GUIDED || c.filter == GDPT_SELECT_NLM_DEMOD || c.filter == GDPT_SELECT_NLM_REGRESS ||
           c.filter == GDPT_SELECT_NLM_COLLAB ||
           (c.filter == GDPT_SELECT_ATROUS && ((c.guide && c.guide->num_groups > 0) || c.demod));
}

int gdpt_progressive_group_denoise_select(GdptProgressiveGroup *group, const GdptSelectCandidate *candidates, int n, const GdptSelectParams *select_params,
                                          int feature_spp, int on_device, double *out, int32_t *sel, double *mse, double *features, double *features_var,
                                          GdptSelectStats *stats, GdptNlmStats *cand_stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_progressive_group_denoise_select";
        if (!group) throw std::runtime_error(who + ": null group");
        if (!out) throw std::runtime_error(who + ": out is null");
        if (n < 1 || n > GDPT_SELECT_MAX_CANDIDATES) throw std::runtime_error(who + ": n must be in [1, " + std::to_string(GDPT_SELECT_MAX_CANDIDATES) + "]");
        if (!candidates) throw std::runtime_error(who + ": candidates is null");
        GdptSelectParams sp;
        if (select_params) sp = *select_params; else gdpt_select_default_params(&sp);
        gdpt::select_check_params(who, sp);
        bool any_features = false;
        for (int j = 0; j < n; j++) {
            const GdptSelectCandidate &c = candidates[j];
            const std::string cj = who + ": candidates[" + std::to_string(j) + "]: ";
            if (c.filter < GDPT_SELECT_MEAN || c.filter > GDPT_SELECT_NLM_COLLAB) throw std::runtime_error(cj + "filter must be one of GDPT_SELECT_MEAN .. GDPT_SELECT_NLM_COLLAB");
            const bool smoothable = c.filter == GDPT_SELECT_NLM || c.filter == GDPT_SELECT_NLM_GUIDED || c.filter == GDPT_SELECT_NLM_DEMOD;
            if (c.var_smooth_radius < -1 || c.var_smooth_radius > GDPT_VAR_SMOOTH_MAX_RADIUS)
                throw std::runtime_error(cj + "var_smooth_radius must be -1 (none) or in [0, " + std::to_string(GDPT_VAR_SMOOTH_MAX_RADIUS) + "]");
            if (c.var_smooth_radius >= 0 && !smoothable) throw std::runtime_error(cj + "var_smooth_radius must be -1 unless filter is GDPT_SELECT_NLM, _NLM_GUIDED or _NLM_DEMOD");
            if (c.filter == GDPT_SELECT_MEAN && (c.nlm || c.atrous || c.guide || c.demod || c.regress)) throw std::runtime_error(cj + "GDPT_SELECT_MEAN takes no parameter block");
            if (c.filter != GDPT_SELECT_ATROUS && c.atrous) throw std::runtime_error(cj + "atrous must be null unless filter is GDPT_SELECT_ATROUS");
            if (c.filter == GDPT_SELECT_ATROUS && c.nlm) throw std::runtime_error(cj + "nlm must be null for GDPT_SELECT_ATROUS");
            if (c.filter != GDPT_SELECT_NLM_REGRESS && c.filter != GDPT_SELECT_NLM_COLLAB && c.regress)
                throw std::runtime_error(cj + "regress must be null unless filter is GDPT_SELECT_NLM_REGRESS or GDPT_SELECT_NLM_COLLAB");
            if (c.filter != GDPT_SELECT_NLM_DEMOD && c.filter != GDPT_SELECT_ATROUS && c.demod) throw std::runtime_error(cj + "demod must be null unless filter is GDPT_SELECT_NLM_DEMOD or GDPT_SELECT_ATROUS");
            if (c.filter == GDPT_SELECT_NLM && c.guide) throw std::runtime_error(cj + "guide must be null for GDPT_SELECT_NLM");
            any_features = any_features || renders_features(c);
        }
        if ((features || features_var) && !any_features) throw std::runtime_error(who + ": features need a candidate that renders some (none does)");
        GdptProgressiveGroup &g = *group;
        // 1. the halves and the total are current
        GdptProgressive *half[2] = {nullptr, nullptr};
        if (gdpt_progressive_group_halves(group, &half[0], &half[1]) != 0) throw std::runtime_error(who + ": " + gdpt_last_error());
        if (!g.total_current) rebuild_total(g);
        {
            const std::vector<int> used = members_with_samples(g);
            for (int k = 0; k < 2; k++) {
                if (half[k]->passes >= 2) continue;
                std::string list;
                for (size_t i = (size_t)k; i < used.size(); i += 2) list += (list.empty() ? "" : ", ") + std::to_string(used[i]);
                throw std::runtime_error(who + ": half " + (k == 0 ? "A" : "B") + " (members " + list + ") holds " + std::to_string(half[k]->passes) +
                                         " pass: every half needs at least 2 for its variance");
            }
        }
        GdptProgressive &t = *g.total;
        ck(hipSetDevice(t.device), "hipSetDevice");
        const size_t px = (size_t)t.w * t.h;
        if (g.select_films.size() < (size_t)(3 * n + 4)) g.select_films.resize((size_t)(3 * n + 4));
        for (int i = 0; i < 3 * n + 4; i++) if (!g.select_films[(size_t)i]) g.select_films[(size_t)i].alloc(t.elems, "hipMalloc(group select films)");
        GdptProgressive *const part[3] = {half[0], half[1], g.total};
        const size_t fbytes = (size_t)GDPT_FEATURE_CHANNELS * px * sizeof(double);
        bool features_taken = false;
        // 2. one feature render, by the first run on the total that needs the planes; the halves get copies (they share the total's scene,
        // budget and stream, so their own renders would give the same bits) and no session renders again during this call
        struct KeepFeatures {
            GdptProgressive *const *part;
            ~KeepFeatures() { for (int k = 0; k < 3; k++) part[k]->feat_current = false; }
        } keep{part};
        // 3. every candidate on A, B and the total, into the group's films (device memory)
        const double *FA[GDPT_SELECT_MAX_CANDIDATES], *FB[GDPT_SELECT_MAX_CANDIDATES], *T[GDPT_SELECT_MAX_CANDIDATES];
        for (int j = 0; j < n; j++) {
            const GdptSelectCandidate &c = candidates[j];
            for (int k : {2, 0, 1}) {         // (the total first: it renders the planes)
                double *film = g.select_films[(size_t)(3 * j + k)];
                (k == 0 ? FA : k == 1 ? FB : T)[j] = film;
                GdptNlmStats st{};
                // the planes of the first feature-rendering run on the total go out with it
                double *fm = nullptr, *fv = nullptr;
                if (k == 2 && renders_features(c) && !features_taken && (features || features_var)) {
                    if (on_device) { fm = features; fv = features_var; }
                    else {
                        for (auto &b : g.select_feat) if (!b) b.alloc((size_t)GDPT_FEATURE_CHANNELS * px, "hipMalloc(group select features)");
                        fm = g.select_feat[0]; fv = g.select_feat[1];
                    }
                    features_taken = true;
                }
                GdptVarSmoothParams vs{};
                gdpt_var_smooth_default_params(&vs);
                vs.radius = c.var_smooth_radius;
                int rc = 0;
                switch (c.filter) {
                case GDPT_SELECT_MEAN: {
                    double *const means[5] = {film, nullptr, nullptr, nullptr, nullptr};
                    rc = gdpt_progressive_read(part[k], 1, means, nullptr, nullptr);
                    break;
                }
                case GDPT_SELECT_NLM:
                    rc = c.var_smooth_radius >= 0
                             ? gdpt_progressive_denoise_smoothed(part[k], GDPT_DENOISE_PLAIN, &vs, c.nlm, nullptr, nullptr, feature_spp, 1, film, nullptr, nullptr, nullptr, nullptr, &st, nullptr)
                             : gdpt_progressive_denoise(part[k], c.nlm, 1, film, nullptr, &st);
                    break;
                case GDPT_SELECT_NLM_GUIDED:
                    rc = c.var_smooth_radius >= 0
                             ? gdpt_progressive_denoise_smoothed(part[k], GDPT_DENOISE_GUIDED, &vs, c.nlm, c.guide, nullptr, feature_spp, 1, film, nullptr, nullptr, fm, fv, &st, nullptr)
                             : gdpt_progressive_denoise_guided(part[k], c.nlm, c.guide, feature_spp, 1, film, nullptr, fm, fv, &st);
                    break;
                case GDPT_SELECT_NLM_DEMOD:
                    rc = c.var_smooth_radius >= 0
                             ? gdpt_progressive_denoise_smoothed(part[k], GDPT_DENOISE_DEMOD, &vs, c.nlm, c.guide, c.demod, feature_spp, 1, film, nullptr, nullptr, fm, fv, &st, nullptr)
                             : gdpt_progressive_denoise_demod(part[k], c.nlm, c.guide, c.demod, feature_spp, 1, film, nullptr, fm, fv, &st);
                    break;
                case GDPT_SELECT_NLM_REGRESS:
                    rc = gdpt_progressive_denoise_regress(part[k], c.nlm, c.guide, c.regress, feature_spp, 1, film, nullptr, fm, fv, &st);
                    break;
                case GDPT_SELECT_NLM_COLLAB:
                    rc = gdpt_progressive_denoise_collab(part[k], c.nlm, c.guide, c.regress, feature_spp, 1, film, fm, fv, &st);
                    break;
                default:
                    rc = gdpt_progressive_denoise_atrous(part[k], c.atrous, c.guide, c.demod, feature_spp, 1, film, nullptr, fm, fv, &st);
                    break;
                }
                if (rc != 0) throw std::runtime_error(who + ": candidates[" + std::to_string(j) + "] on " + (k == 0 ? "half A" : k == 1 ? "half B" : "the total") + ": " + gdpt_last_error());
                if (k == 2 && cand_stats) cand_stats[j] = st;
                if (k == 2 && renders_features(c) && !t.feat_current) {
                    ck(hipSetDevice(t.device), "hipSetDevice");
                    for (int m = 0; m < 2; m++)
                        for (int b = 0; b < 2; b++) {
                            if (!half[m]->feat_buf[b]) half[m]->feat_buf[b].alloc((size_t)GDPT_FEATURE_CHANNELS * px, "hipMalloc(progressive features)");
                            ck(hipMemcpyAsync(half[m]->feat_buf[b], t.feat_buf[b], fbytes, hipMemcpyDeviceToDevice, g.total_stream), "hipMemcpyAsync(group select features)");
                        }
                    for (int m = 0; m < 3; m++) part[m]->feat_current = true;
                }
            }
        }
        ck(hipSetDevice(t.device), "hipSetDevice");
        double *uv[4];
        for (int i = 0; i < 4; i++) uv[i] = g.select_films[(size_t)(3 * n + i)];
        for (int k = 0; k < 2; k++) {
            double *const means[5] = {uv[2 * k], nullptr, nullptr, nullptr, nullptr};
            double *const vars[5] = {uv[2 * k + 1], nullptr, nullptr, nullptr, nullptr};
            if (gdpt_progressive_read(half[k], 1, means, vars, nullptr) != 0) throw std::runtime_error(who + ": " + gdpt_last_error());
        }
        // 4. the selection, on the total's stream
        double *d_out = out, *d_mse = mse;
        int32_t *d_sel = sel;
        if (!on_device) {
            if (!g.select_out) g.select_out.alloc(t.elems, "hipMalloc(group select outputs)");
            d_out = g.select_out;
            if (sel) { if (!g.select_sel) g.select_sel.alloc(px, "hipMalloc(group select outputs)"); d_sel = g.select_sel; }
            if (mse) { if (!g.select_mse) g.select_mse.alloc(px, "hipMalloc(group select outputs)"); d_mse = g.select_mse; }
        }
        GdptSelectStats st{};
        if (gdpt_filter_select_device(t.w, t.h, n, FA, FB, T, uv[0], uv[1], uv[2], uv[3], &sp, d_out, d_sel, d_mse, nullptr, g.total_stream, &st) != 0)
            throw std::runtime_error(who + ": " + gdpt_last_error());
        if (!on_device) {
            ck(hipMemcpyAsync(out, d_out, t.elems * sizeof(double), hipMemcpyDeviceToHost, g.total_stream), "hipMemcpyAsync(D2H)");
            if (sel) ck(hipMemcpyAsync(sel, d_sel, px * sizeof(int32_t), hipMemcpyDeviceToHost, g.total_stream), "hipMemcpyAsync(D2H)");
            if (mse) ck(hipMemcpyAsync(mse, d_mse, px * sizeof(double), hipMemcpyDeviceToHost, g.total_stream), "hipMemcpyAsync(D2H)");
            if (features_taken && features) ck(hipMemcpyAsync(features, g.select_feat[0], fbytes, hipMemcpyDeviceToHost, g.total_stream), "hipMemcpyAsync(D2H)");
            if (features_taken && features_var) ck(hipMemcpyAsync(features_var, g.select_feat[1], fbytes, hipMemcpyDeviceToHost, g.total_stream), "hipMemcpyAsync(D2H)");
        }
        ck(hipStreamSynchronize(g.total_stream), "hipStreamSynchronize(group select)");
        if (stats) *stats = st;
    });
}

int gdpt_progressive_group_member_status(const GdptProgressiveGroup *group, int member, GdptProgressiveStatus *status) {
    return gdpt::guarded([&]() {
        if (!group || !status) throw std::runtime_error("gdpt_progressive_group_member_status: null argument");
        if (member < 0 || member >= (int)group->members.size()) throw std::runtime_error("gdpt_progressive_group_member_status: no such member");
        prg::fill_status(*group->members[(size_t)member].session, status);
    });
}

} // extern "C"
