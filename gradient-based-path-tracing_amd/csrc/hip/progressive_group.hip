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
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "progressive_internal.h"

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

    ~GdptProgressiveGroup() {
        if (total) gdpt_progressive_free(total);
        for (Member &m : members) if (m.session) gdpt_progressive_free(m.session);
        if (total_stream && !members.empty()) {
            hipSetDevice(members[0].device);
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
    g.total_current = false;
    for (int i : todo) {
        const Member &m = g.members[(size_t)i];
        if (!m.error.empty()) throw std::runtime_error("device " + std::to_string(m.device) + " (member " + std::to_string(i) + "): " + m.error);
    }
    return true;
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
        {   // every member gets its own copy of the scene; the uploads run side by side (as gdpt_multi_create's do)
            std::vector<std::exception_ptr> errs((size_t)n);
            std::vector<std::thread> th;
            auto one = [&](int i) {
                try {
                    Member &m = g->members[(size_t)i];
                    m.device = devices[i];
                    m.scene.reset(new GdptScene());
                    gdpt::build_scene(desc, m.device, m.scene.get());       // sets the calling thread's device
                    m.scene->scene_spp = desc->samples_per_pixel;
                } catch (...) { errs[(size_t)i] = std::current_exception(); }
            };
            for (int i = 1; i < n; i++) th.emplace_back(one, i);
            one(0);
            for (std::thread &t : th) t.join();
            for (const std::exception_ptr &e : errs) if (e) std::rethrow_exception(e);
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

GdptProgressive *gdpt_progressive_group_total(GdptProgressiveGroup *group) { return group ? group->total : nullptr; }

int gdpt_progressive_group_member_status(const GdptProgressiveGroup *group, int member, GdptProgressiveStatus *status) {
    return gdpt::guarded([&]() {
        if (!group || !status) throw std::runtime_error("gdpt_progressive_group_member_status: null argument");
        if (member < 0 || member >= (int)group->members.size()) throw std::runtime_error("gdpt_progressive_group_member_status: no such member");
        prg::fill_status(*group->members[(size_t)member].session, status);
    });
}

} // extern "C"
