// capi_device.hip — device-side entry points of include/gdpt.h: scene upload (the tables host/scene_prepare.cpp
// makes, copied to HBM), the five-buffer render, gradient assembly, the Poisson solve and the whole GradPath pipeline.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "../device_scene.h"
#include "../host/scene_prepare.h"
#include "denoise_nlm.h"
#include "image_kernels.h"
#include "poisson_kernels.h"
#include "progressive_internal.h"
#include "recon_l1.h"
#include "recon_pcg.h"
#include "recon_spread.h"
#include "recon_weighted.h"
#include "render_kernels.h"
#include "scene_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace {

using gdpt::ck;

// a scene table, owned by the scene
template <class T>
T *upload(GdptScene *sc, const std::vector<T> &v) {
    if (v.empty()) return nullptr;
    gdpt::DeviceBuffer<unsigned char> d;
    d.alloc(v.size() * sizeof(T), "hipMalloc(scene)");
    ck(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(scene)");
    sc->allocations.push_back(std::move(d));
    return (T *)sc->allocations.back().data();
}

} // namespace

static constexpr int kWavefrontDefault = 0;       // HBM scenes: 1 = wavefront pipeline by default, 0 = lane machine

namespace gdpt {

namespace {

void check_device(int device) {
    int ndev = 0;
    ck(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (ndev <= 0) throw std::runtime_error("gdpt_scene_upload: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) throw std::runtime_error("gdpt_scene_upload: bad device index");
}

// The host half of an upload with the knobs resolved (host/scene_prepare.h). GDPT_HBM_BVH8 and GDPT_HBM_Q4 are tested here, in a
// translation unit the A/B builds recompile, and nowhere in a host object.
PreparedScene prepare(const GdptSceneDesc &desc) {
    PrepareOptions opt;
    opt.presplit = debug_knob("presplit", -1.0);
    opt.sbvh = debug_knob("sbvh", -1.0);
    opt.with_bvh8 = GDPT_HBM_BVH8 != 0;
    opt.with_q4 = GDPT_HBM_Q4 != 0;
    return prepare_scene(desc, opt);
}

} // namespace

void upload_scene(const PreparedScene &ps, int device, GdptScene *sc) {
    check_device(device);
    ck(hipSetDevice(device), "hipSetDevice");
    sc->device = device;
    sc->traits = ps.traits;
    DevSceneView &v = sc->view;
    v = ps.view;
    v.nodes = upload(sc, ps.nodes);
    v.nodes4 = upload(sc, ps.nodes4);
    v.nodes8 = upload(sc, ps.nodes8);
    v.nodes4q = upload(sc, ps.nodes4q);
    v.prims = upload(sc, ps.prims);
    v.tris = upload(sc, ps.tris);
    v.spheres = upload(sc, ps.spheres);
    v.materials = upload(sc, ps.materials);
    v.light_intensity = upload(sc, ps.light_intensity);
    v.images = upload(sc, ps.images);
    v.texels = upload(sc, ps.texels);
    v.lights = upload(sc, ps.lights);
    v.light_tri_cdf = upload(sc, ps.light_tri_cdf);
    v.light_tri_pos = upload(sc, ps.light_tri_pos);
    v.light_tri_nrm = upload(sc, ps.light_tri_nrm);
    v.env_cdf_rows = upload(sc, ps.env_cdf_rows);
    v.env_pdf_rows = upload(sc, ps.env_pdf_rows);
    v.env_cdf_marginals = upload(sc, ps.env_cdf_marginals);
    v.env_pdf_marginals = upload(sc, ps.env_pdf_marginals);
    v.light_pmf = upload(sc, ps.light_pmf);
    v.light_cdf = upload(sc, ps.light_cdf);

    sc->scratch[0].counters.alloc(1, "hipMalloc(counters)");
    sc->scratch[0].queue.alloc(1, "hipMalloc(queue)");
    sc->d_counters = sc->scratch[0].counters;
    for (auto &st : sc->render_stream) st.create();
    for (auto &ss : sc->scratch) { ss.rendered.create(hipEventDisableTiming); ss.released.create(hipEventDisableTiming); }
    for (auto &e : sc->ev_entry) e.create(hipEventDisableTiming);
    { hipDeviceProp_t prop; ck(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties"); sc->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }
    sc->h_counters.alloc(1, "hipHostMalloc(counters)");
    sc->ev0.create();
    sc->ev1.create();
}

void build_scene(const GdptSceneDesc *desc, int device, GdptScene *sc) {
    if (!desc) throw std::runtime_error("gdpt_scene_upload: null scene description");
    check_device(device);          // (before the description's own checks, and before the seconds a large mesh's tree takes)
    upload_scene(prepare(*desc), device, sc);
}

std::vector<std::unique_ptr<GdptScene>> upload_scenes(const GdptSceneDesc *desc, const int32_t *devices, int n) {
    if (!desc) throw std::runtime_error("gdpt_scene_upload: null scene description");
    for (int i = 0; i < n; i++) check_device(devices[i]);
    const PreparedScene ps = prepare(*desc);
    // every device gets its own copy of the tables; the fp64 texel pool of a textured mesh is hundreds of MB of pageable copy per
    // device, so the N uploads run side by side instead of one after the other
    std::vector<std::unique_ptr<GdptScene>> scenes((size_t)n);
    std::vector<std::exception_ptr> errs((size_t)n);
    std::vector<std::thread> th;
    auto one = [&](int i) {
        try {
            scenes[(size_t)i].reset(new GdptScene());
            upload_scene(ps, devices[i], scenes[(size_t)i].get());       // sets the calling thread's device
            scenes[(size_t)i]->scene_spp = desc->samples_per_pixel;
        } catch (...) { errs[(size_t)i] = std::current_exception(); }
    };
    for (int i = 1; i < n; i++) th.emplace_back(one, i);
    one(0);
    for (std::thread &t : th) t.join();
    for (const std::exception_ptr &e : errs) if (e) std::rethrow_exception(e);
    return scenes;
}

} // namespace gdpt

namespace {

using gdpt::build_scene;

struct Band { int spp, rng, row_begin, row_end, max_depth, shift, plan_rows, stream_spp, first_sample; };

Band resolve(const GdptScene *sc, const GdptRenderParams *p) {
    if (!sc) throw std::runtime_error("null scene handle");
    Band b;
    b.spp = (p && p->spp > 0) ? p->spp : 0;
    b.rng = p ? p->rng_scheme : GDPT_RNG_SAMPLE;
    b.row_begin = p ? p->row_begin : 0;
    b.row_end = p ? p->row_end : 0;
    if (b.row_begin == 0 && b.row_end == 0) b.row_end = sc->view.cam.height;
    if (b.row_begin < 0 || b.row_end > sc->view.cam.height || b.row_begin >= b.row_end) throw std::runtime_error("gdpt_render: bad row band");
    if (b.rng != GDPT_RNG_TILE && b.rng != GDPT_RNG_SAMPLE) throw std::runtime_error("gdpt_render: unknown rng_scheme");
    b.shift = p ? p->shift_mode : GDPT_SHIFT_REFERENCE;
    if (b.shift != GDPT_SHIFT_REFERENCE && b.shift != GDPT_SHIFT_RECONNECT) throw std::runtime_error("gdpt_render: unknown shift_mode");
    if (b.shift == GDPT_SHIFT_RECONNECT && b.rng != GDPT_RNG_SAMPLE) throw std::runtime_error("gdpt_render: GDPT_SHIFT_RECONNECT needs GDPT_RNG_SAMPLE");
    if (b.rng == GDPT_RNG_TILE && ((b.row_begin % 16) != 0 || ((b.row_end % 16) != 0 && b.row_end != sc->view.cam.height)))
        throw std::runtime_error("gdpt_render: GDPT_RNG_TILE bands must cover whole 16-pixel tile rows");
    b.max_depth = (p && p->max_depth_override != 0) ? p->max_depth_override : sc->view.max_depth;
    b.plan_rows = (p && p->plan_rows > 0) ? std::min(p->plan_rows, sc->view.cam.height) : sc->view.cam.height;
    if (p && p->plan_rows < 0) throw std::runtime_error("gdpt_render: plan_rows must be >= 0");
    return b;
}

// The band with its samples per pixel (the params' spp, else `scene_spp`).
// `win` (nullable) makes the samples a window of a larger stream block (include/gdpt.h: GdptSampleWindow).
Band resolve_spp(const GdptScene *sc, const GdptRenderParams *p, int scene_spp, const char *what, const GdptSampleWindow *win = nullptr) {
    Band b = resolve(sc, p);
    if (b.spp <= 0) b.spp = scene_spp;
    if (b.spp <= 0) throw std::runtime_error(std::string(what) + ": samples per pixel must be > 0");
    b.stream_spp = b.spp; b.first_sample = 0;
    if (win) {
        if (b.rng == GDPT_RNG_TILE) throw std::runtime_error(std::string(what) + ": GDPT_RNG_TILE has one stream per tile and no sample window (use GDPT_RNG_SAMPLE)");
        if (win->stream_spp <= 0 || win->first_sample < 0 || (long long)win->first_sample + b.spp > (long long)win->stream_spp)
            throw std::runtime_error(std::string(what) + ": sample window [first_sample, first_sample + spp) must lie inside [0, stream_spp)");
        // the largest stream index, W * H * stream_spp - 1, goes through pcg_init's (index << 1) | 1
        if ((unsigned long long)sc->view.cam.width * (unsigned long long)sc->view.cam.height > (~0ull >> 1) / (unsigned long long)win->stream_spp)
            throw std::runtime_error(std::string(what) + ": width * height * stream_spp does not fit 63 bits");
        b.stream_spp = win->stream_spp; b.first_sample = win->first_sample;
    }
    return b;
}

// The scratch set a launch was given, and whether an event of the handle's may follow it on the caller's stream.
struct ScratchClaim { GdptLaunchScratch *set = nullptr; bool record_release = true; };

// True while `stream` records a graph (or cannot tell: the null stream beside a capture elsewhere).
bool is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return true; }
    return st != hipStreamCaptureStatusNone;
}

// Host wait for everything that uses the handle's launch scratch: the render streams, and on the callers' streams the last user of
// each set. For the rare places that cannot be ordered by an event (a buffer about to be freed; a launch recorded into a graph).
void join_scratch(GdptScene *sc) {
    sc->join();
    for (auto &ss : sc->scratch) if (ss.used) ck(hipEventSynchronize(ss.released), "hipEventSynchronize(launch scratch)");
}

// The scratch set of the next launch on `stream`, with partials for `need` doubles, and the dependencies of that launch enqueued
// (scene_internal.h: GdptLaunchScratch). In-stream: set 0, everything on the caller's stream as if the handle had no other. Overlapped:
// sets and render streams alternate; the render stream waits for the reduction that last read the set (two frames back) and for the
// caller's stream AS IT WAS AT THE PREVIOUS CALL: behind frame k - 1's kernel the stream then holds frame k - 2's reduction and what the
// caller enqueued after it (its solve), so frame k's kernel starts beside frame k - 1's drain but not before frame k - 2 is through.
// Waiting for the stream as it is at this call would put frame k - 1's solve in front of the kernel, and nothing would overlap; not
// waiting at all lets a third kernel queue up while the small kernels of two frames (whose GEMMs need LDS the resident render blocks
// hold) starve behind it: profiles/render_overlap_times.txt has both schemes, measured. Where the handle says so (need_fence) both render streams wait
// for the caller's stream as it is now.
// An overlapped launch's resets (counters, queue head) are enqueued here, on the render stream, behind its wait for the set's release
// and AHEAD of its wait for the previous call: they depend on the set alone, and behind the second wait they were three small fills
// between the previous frame's solve and this frame's kernel (18-19 us of the 37 us gap, profiles/render_overlap_times.txt). Nothing
// reads a set's counters between its release and its next launch: their readers are the stats copy of run_launch (an in-stream launch,
// which joins the render streams first and records `released` behind itself) and the synchronous copy of multi_gpu.hip (through
// d_counters, after the host has waited for the render, before that host thread's next launch); the queue head is read by the render
// kernel only, which the render stream orders.
GdptLaunchScratch &claim_scratch(GdptScene *sc, bool overlap, bool capturing, size_t need, hipStream_t stream) {
    const int k = overlap ? (int)(sc->overlapped & 1) : 0;
    GdptLaunchScratch &ss = sc->scratch[k];
    const hipEvent_t entry = sc->ev_entry[sc->calls & 1], prev_entry = sc->calls ? (hipEvent_t)sc->ev_entry[(sc->calls + 1) & 1] : nullptr;
    if (!capturing) { ck(hipEventRecord(entry, stream), "hipEventRecord(entry)"); sc->calls++; }
    if (capturing) {
        // the launch is recorded on today's path, with no event of ours in the graph: whatever is in flight ends first
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        ck(hipThreadExchangeStreamCaptureMode(&mode), "hipThreadExchangeStreamCaptureMode");
        try { join_scratch(sc); } catch (...) { (void)hipThreadExchangeStreamCaptureMode(&mode); throw; }
        ck(hipThreadExchangeStreamCaptureMode(&mode), "hipThreadExchangeStreamCaptureMode");
    }
    if (!ss.counters) ss.counters.alloc(1, "hipMalloc(counters)");
    if (!ss.queue) ss.queue.alloc(1, "hipMalloc(queue)");
    if (need > ss.partials.size()) {       // never free what a launch in flight uses
        if (ss.partials) {                 // (a set's first buffer replaces nothing: no join, no fence)
            if (!capturing) join_scratch(sc);
            sc->need_fence = true;
        }
        ss.partials.alloc(need, "hipMalloc(work-item partials)");
    }
    if (!overlap) {
        if (!capturing) {
            sc->join();                    // the launch, and a host read of the counters behind it, have the handle to themselves (and the hint is cleared)
            if (ss.used) ck(hipStreamWaitEvent(stream, ss.released, 0), "hipStreamWaitEvent(launch scratch)");   // (another caller's stream)
        }
    } else {
        if (sc->have_caller && stream != sc->last_caller) {      // another caller's stream: it joins the render streams, they join it
            for (auto &o : sc->scratch) ck(hipStreamWaitEvent(stream, o.rendered, 0), "hipStreamWaitEvent(render stream)");
            sc->need_fence = true;
        }
        if (ss.used) ck(hipStreamWaitEvent(sc->render_stream[k], ss.released, 0), "hipStreamWaitEvent(launch scratch)");
        sc->in_flight = true;              // (from here on a render stream may hold work: GdptScene::join)
        ck(hipMemsetAsync(ss.counters, 0, sizeof(gdpt::RenderCounters), sc->render_stream[k]), "hipMemsetAsync(counters)");
        ck(hipMemsetAsync(ss.queue, 0, sizeof(unsigned long long), sc->render_stream[k]), "hipMemsetAsync(queue)");
        if (sc->need_fence || !prev_entry) {
            for (auto &st : sc->render_stream) ck(hipStreamWaitEvent(st, entry, 0), "hipStreamWaitEvent(fence)");
            sc->need_fence = false;
        } else
            ck(hipStreamWaitEvent(sc->render_stream[k], prev_entry, 0), "hipStreamWaitEvent(previous call)");
    }
    sc->have_caller = true; sc->last_caller = stream;
    return ss;
}

// Chooses the route of a render of band `b` and fills the launch fields both integrators share; a persistent route gets its
// work-item plan (made here, once) and a partials buffer that holds it. The knobs are the A/B overrides of the parity tests
// (include/gdpt_debug.h); every default is the product path.
// A launch of the one-sided lane machine that the host does not wait for is overlapped: its kernel goes on one of the handle's two
// render streams and may start while the previous frame's kernel drains and its reduction and solve run (knob no_render_overlap
// keeps it in-stream). Launches with stats, every other route and a launch recorded into a graph stay on the caller's stream.
gdpt::RenderLaunch begin_launch(GdptScene *sc, const Band &b, bool path, int take_pct, hipStream_t stream, const GdptRenderStats *stats, ScratchClaim *claim) {
    auto knob = [](const char *name, int def) { return gdpt::debug_knob_int(name, def); };
    const DevSceneView &v = sc->view;
    gdpt::RouteInputs in{};
    in.path = path; in.rng_scheme = b.rng; in.shift_mode = b.shift; in.max_depth = b.max_depth; in.rr_depth = v.rr_depth;
    in.one_sided = sc->traits.one_sided; in.has_rough = sc->traits.has_rough; in.lambert_only = sc->traits.lambert_only; in.material_mask = sc->traits.material_mask;
    in.has_spheres = v.num_spheres != 0; in.const_textures = v.all_textures_constant != 0; in.has_envmap = v.has_envmap != 0;
    in.fits_lds = gdpt::scene_fits_lds(v.num_nodes, v.num_prims, v.num_tris, v.num_materials, v.num_lights, sc->traits.bvh_depth);
    in.fits_lds_wide = gdpt::scene_fits_lds_wide(v.num_nodes4, v.num_prims, v.num_tris, v.num_materials, v.num_lights, sc->traits.wide_stack_need);
    in.force_eager = knob("force_eager", 0) != 0; in.no_lds_scene = knob("no_lds_scene", 0) != 0; in.lds_wide = knob("lds_wide", 1) != 0;
    in.no_twosided_machine = knob("no_twosided_machine", 0) != 0; in.wavefront = knob("wavefront", kWavefrontDefault) != 0;
    in.stamps = knob("stamps", 0) != 0; in.no_plain_kernel = knob("no_plain_kernel", 0) != 0;
    in.full_material_switch = knob("full_material_switch", 0) != 0; in.whole_leaf_trips = knob("whole_leaf_trips", 0) != 0;
    in.no_setup_batch = knob("no_setup_batch", 0) != 0;
    gdpt::RenderLaunch rl{};
    rl.route = gdpt::choose_route(in);
    rl.whole_leaf_trips = in.whole_leaf_trips; rl.no_setup_batch = in.no_setup_batch;
    rl.spp = b.spp; rl.stream_spp = b.stream_spp; rl.first_sample = b.first_sample; rl.row_begin = b.row_begin; rl.row_end = b.row_end; rl.max_depth = b.max_depth;
    rl.count_traversal = stats && stats->nodes_visited == ~0ull;   // request flag: caller presets nodes_visited = UINT64_MAX
    rl.force_log2k = knob("log2k", -1);
    rl.thresh_a = knob("keep_frac", -1); rl.thresh_c = knob("search_frac", -1);
    rl.num_cus = sc->num_cus; rl.blocks_per_cu = knob("blocks_per_cu", 0);
    const bool capturing = is_capturing(stream);
    const bool overlap = !stats && gdpt::can_overlap(rl.route) && !capturing && knob("no_render_overlap", 0) == 0;
    size_t need = 0;
    if (gdpt::is_persistent(rl.route)) {
        // The plan is made for a band of plan_rows rows (default: the whole film), whatever band is rendered: a pixel's samples
        // are cut (and its partial sums merged) the same way by every render that names the same plan_rows, so a sharded render
        // equals the unsharded one with that plan bit for bit. (Round 2 always planned for the whole film: a 64-row band of the
        // 512x512x256 film, 1/8 of the work, then held 32 k items of 128 samples and took 9.3 ms instead of 3.8 —
        // profiles/r03_band_costs.txt.)
        rl.plan = gdpt::make_chunk_plan(b.spp, rl.force_log2k, (long long)v.cam.width * b.plan_rows, gdpt::resident_lanes(rl), take_pct);
        need = (size_t)16 * (size_t)gdpt::band_slots(v.cam.width, b.row_end - b.row_begin) * (size_t)rl.plan.n;
    }
    GdptLaunchScratch &ss = claim_scratch(sc, overlap, capturing, need, stream);
    rl.counters = ss.counters; sc->d_counters = ss.counters;
    if (gdpt::is_persistent(rl.route)) { rl.partials = ss.partials; rl.queue_head = ss.queue; }
    if (overlap) { rl.kernel_stream = sc->render_stream[sc->overlapped & 1]; rl.kernel_done = ss.rendered; rl.resets_enqueued = true; }   // (claim_scratch)
    claim->set = &ss; claim->record_release = !capturing;
    return rl;
}

// Enqueues the counter reset (unless claim_scratch has: an overlapped launch), the launch and, when stats are requested, waits for the render and reports it.
void run_launch(GdptScene *sc, const gdpt::RenderLaunch &rl, const ScratchClaim &claim, const Band &b, hipStream_t stream, GdptRenderStats *stats) {
    const bool stamped = gdpt::is_stamped(rl.route);
    const hipStream_t ks = rl.kernel_stream ? rl.kernel_stream : stream;       // (begin_launch: an overlapped launch)
    if (rl.kernel_stream) sc->in_flight = true;           // (from here on a render stream may hold work: GdptScene::join)
    if (!rl.resets_enqueued) ck(hipMemsetAsync(rl.counters, 0, sizeof(gdpt::RenderCounters), ks), "hipMemsetAsync(counters)");
    if (stamped) ck(hipMemsetAsync(&rl.counters->stamps[12], 0xFF, 2 * sizeof(unsigned long long), ks), "hipMemsetAsync(stamps)");   // min slots
    if (stats) ck(hipEventRecord(sc->ev0, stream), "hipEventRecord");
    gdpt::launch_render(sc->view, rl, stream);
    if (rl.kernel_stream) {
        sc->overlapped++;                                 // (a launch that threw leaves the set parity where it was)
        // a solve enqueued from here on may find this kernel's blocks resident: tell it what they leave (render_kernels.h)
        gdpt::set_render_beside_hint(sc->device, sc, gdpt::render_free_lds_per_cu(sc->view, rl));
    }
    // the set is free again behind this point of the caller's stream (a launch recorded into a graph leaves no event of ours in it)
    if (claim.record_release) { ck(hipEventRecord(claim.set->released, stream), "hipEventRecord(launch scratch)"); claim.set->used = true; }
    if (!stats) return;
    ck(hipEventRecord(sc->ev1, stream), "hipEventRecord");
    ck(hipMemcpyAsync(sc->h_counters, rl.counters, sizeof(gdpt::RenderCounters), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(counters)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(render)");
    float ms = 0;
    ck(hipEventElapsedTime(&ms, sc->ev0, sc->ev1), "hipEventElapsedTime");
    const gdpt::RenderCounters &c = *sc->h_counters;
    std::memset(stats, 0, sizeof(*stats));
    stats->samples = (uint64_t)sc->view.cam.width * (uint64_t)(b.row_end - b.row_begin) * (uint64_t)b.spp;
    stats->rays = c.rays; stats->bounces = c.bounces; stats->nonfinite_samples = c.nonfinite;
    stats->nodes_visited = c.nodes; stats->tris_tested = c.prims;
    stats->render_ms = ms;
    if (!gdpt::is_path(rl.route)) {   // (Integrator::Path leaves them 0)
        stats->wave_node_trips = c.wave_node_trips; stats->wave_leaf_trips = c.wave_leaf_trips;
        stats->wave_steps = c.wave_steps; stats->lane_steps = c.lane_steps;
    }
    if (stamped) gdpt::debug_store_stamps(c.stamps, 16);
    stats->node_bytes = gdpt::walks_bvh2(rl.route) ? sizeof(DevBvhNode) : sizeof(DevBvh4Node);
}

} // namespace

namespace gdpt {
// Enqueues one render; returns after enqueue unless stats are requested.
void render_device_impl(GdptScene *sc, const GdptRenderParams *params, int scene_spp,
                        double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                        hipStream_t stream, GdptRenderStats *stats, const GdptSampleWindow *window) {
    reset_route();           // (include/gdpt_debug.h: "" until this render has launched its kernel)
    ck(hipSetDevice(sc->device), "hipSetDevice");
    const Band b = resolve_spp(sc, params, scene_spp, "gdpt_render", window);
    if (!img || !cx0 || !cy0 || !cx1 || !cy1) throw std::runtime_error("gdpt_render: null output buffer");
    ScratchClaim claim;
    RenderLaunch rl = begin_launch(sc, b, false, sc->traits.plan_take_pct, stream, stats, &claim);
    rl.img = img; rl.cx0 = cx0; rl.cy0 = cy0; rl.cx1 = cx1; rl.cy1 = cy1;
    rl.wide_stack_need = GDPT_HBM_BVH8 ? std::min(sc->traits.wide8_stack_need, GDPT_BVH_MAX_DEPTH) : sc->traits.wide_stack_need;   // LDS slots; the BVH8 may go on in private memory
    rl.lds_stack_need = walks_bvh2(rl.route) ? sc->traits.bvh_depth : sc->traits.wide_stack_need;      // (the tree the LDS copy holds)
    rl.lds_fixed_layout = debug_knob_int("lds_fixed_layout", 0) != 0;
    rl.replay_per_step = debug_knob_int("replay_per_step", 0);
    const long long items = band_slots(sc->view.cam.width, b.row_end - b.row_begin) * rl.plan.n;
    if (needs_bounce_log(rl.route)) {
        sc->d_bounce_log.grow(twosided_log_bytes(persistent_blocks(rl, items)), stream, "hipMalloc(bounce log)");
        rl.bounce_log = sc->d_bounce_log; rl.bounce_log_bytes = sc->d_bounce_log.size();
    }
    if (is_wavefront(rl.route)) {
        int slots = wf_slot_count(items);
        { const int forced = debug_knob_int("wf_slots", 0); if (forced > 0) slots = std::min(slots, (forced + 255) / 256 * 256); }   // tests: force slot reuse
        sc->d_wf_state.grow((size_t)slots * wf_words(), stream, "hipMalloc(wavefront state)");
        sc->d_wf_live.grow((size_t)slots, stream, "hipMalloc(wavefront live list)");
        sc->d_wf_aux.grow(wf_aux_bytes(slots), stream, "hipMalloc(wavefront ray / hit records)");
        if (!sc->d_wf_counters) sc->d_wf_counters.alloc((size_t)3 * wf_max_generations(), "hipMalloc(wavefront counters)");
        if (!sc->h_wf_word) sc->h_wf_word.alloc(1, "hipHostMalloc(wavefront)");
        if (!sc->wf_event) sc->wf_event.create(hipEventDisableTiming);
        rl.wf_aux = sc->d_wf_aux; rl.wf_sort = debug_knob_int("wf_sort", 1);
        for (int k = 0; k < 6; k++) rl.wf_bounds[k] = sc->traits.bounds[k];
        rl.wf_state = sc->d_wf_state; rl.wf_live = sc->d_wf_live; rl.wf_counters = sc->d_wf_counters; rl.wf_host = sc->h_wf_word;
        rl.wf_event = sc->wf_event; rl.wf_slots = slots;       // exactly the slots this band needs (the buffers may be larger)
    }
    run_launch(sc, rl, claim, b, stream, stats);
}

} // namespace gdpt

namespace {
using gdpt::render_device_impl;
// Integrator::Path: enqueues one render of `img`; returns after enqueue unless stats are requested.
void path_render_device_impl(GdptScene *sc, const GdptRenderParams *params, double *img, hipStream_t stream, GdptRenderStats *stats,
                             const GdptSampleWindow *window) {
    gdpt::reset_route();
    ck(hipSetDevice(sc->device), "hipSetDevice");
    if (sc->view.num_lights <= 0) throw std::runtime_error("gdpt_path_render: the scene has no emitter to sample");
    const Band b = resolve_spp(sc, params, sc->scene_spp, "gdpt_path_render", window);
    if (!img) throw std::runtime_error("gdpt_path_render: null output buffer");
    ScratchClaim claim;
    gdpt::RenderLaunch rl = begin_launch(sc, b, true, 0, stream, stats, &claim);   // (the plan takes the default share: see make_chunk_plan)
    rl.img = img;
    run_launch(sc, rl, claim, b, stream, stats);
}

// GdptReconParams -> the L1 solver's parameters, defaults filled in (include/gdpt.h); refuses what the header says is refused
gdpt::ReconL1Params resolve_recon(const GdptReconParams &in) {
    if (in.norm != GDPT_RECON_L1) throw std::runtime_error("gdpt_reconstruct: unknown norm (GDPT_RECON_L2 | GDPT_RECON_L1)");
    for (double v : {in.eps_init, in.eps_decay, in.eps_floor, in.cg_tol})
        if (!std::isfinite(v) || v < 0) throw std::runtime_error("gdpt_reconstruct: eps_init, eps_decay, eps_floor and cg_tol must be finite and >= 0 (0 = default)");
    if (in.eps_decay > 1.0) throw std::runtime_error("gdpt_reconstruct: eps_decay must lie in (0, 1]");
    gdpt::ReconL1Params p;
    p.irls_iters = in.irls_iters == 0 ? 20 : std::max(in.irls_iters, 0);
    p.cg_max_iters = in.cg_max_iters > 0 ? in.cg_max_iters : 1000;
    p.eps_init = in.eps_init > 0 ? in.eps_init : 0.05;
    p.eps_decay = in.eps_decay > 0 ? in.eps_decay : 0.5;
    p.eps_floor = in.eps_floor > 0 ? in.eps_floor : 1e-3;
    p.cg_tol = in.cg_tol > 0 ? in.cg_tol : 1e-6;
    return p;
}
// The host-pointer entry points of the solvers: the k host planes of `in` (W*H*3 doubles each) go to device planes d[0..k), `run` works
// on them and writes the plane d[k], which comes back into `out`. The planes go when this returns or throws.
using Planes = std::vector<gdpt::DeviceBuffer<double>>;
template <class F>
void on_device_planes(std::initializer_list<const double *> in, int width, int height, double *out, const char *what, F &&run) {
    const size_t elems = (size_t)width * height * 3, bytes = elems * sizeof(double);
    Planes d(in.size() + 1);
    for (auto &b : d) b.alloc(elems, what);
    size_t k = 0;
    for (const double *h : in) ck(hipMemcpy(d[k++], h, bytes, hipMemcpyHostToDevice), "hipMemcpy");
    run(d);
    ck(hipMemcpy(out, d.back(), bytes, hipMemcpyDeviceToHost), "hipMemcpy");
}

void fill_poisson_stats(GdptPoissonStats *s, const gdpt::PoissonResult &r) {
    if (!s) return;
    s->iterations = r.iterations; s->solver = r.solver; s->rel_residual = r.rel_residual; s->solve_ms = r.solve_ms;
}
void fill_recon_stats(GdptReconStats *s, const gdpt::ReconL1Result &r) {
    if (!s) return;
    s->norm = GDPT_RECON_L1; s->irls_rounds = r.irls_rounds; s->cg_iters_total = r.cg_iters_total; s->cg_iters_last = r.cg_iters_last;
    s->energy_first = r.energy_first; s->energy_last = r.energy_last; s->rel_residual_last = r.rel_residual_last; s->solve_ms = r.solve_ms;
}
void fill_recon_stats_l2(GdptReconStats *s, double solve_ms) {
    if (!s) return;
    *s = GdptReconStats{};
    s->norm = GDPT_RECON_L2; s->solve_ms = solve_ms;
}

// GdptWeightedReconParams (nullable) -> the solver's parameters; GDPT_RECON_L2 here means round 0 alone
gdpt::ReconL1Params resolve_weighted(const GdptWeightedReconParams *in, double *conf_floor, int *norm) {
    GdptReconParams rp = in ? in->recon : GdptReconParams{};
    *norm = rp.norm;
    if (rp.norm != GDPT_RECON_L2 && rp.norm != GDPT_RECON_L1) throw std::runtime_error("gdpt_reconstruct_weighted: unknown norm (GDPT_RECON_L2 | GDPT_RECON_L1)");
    rp.norm = GDPT_RECON_L1;
    gdpt::ReconL1Params p = resolve_recon(rp);
    if (*norm == GDPT_RECON_L2) p.irls_iters = 0;
    const double d = in ? in->conf_floor : 0.0;
    if (!std::isfinite(d) || d < 0) throw std::runtime_error("gdpt_reconstruct_weighted: conf_floor must be finite and > 0 (0 = default 0.05)");
    *conf_floor = d > 0 ? d : 0.05;
    return p;
}
void fill_weighted_stats(GdptWeightedReconStats *s, int norm, const gdpt::ReconWeightedResult &r) {
    if (!s) return;
    *s = GdptWeightedReconStats{};
    fill_recon_stats(&s->recon, r.recon);
    s->recon.norm = norm;
    s->scale_data = r.scale_data; s->scale_grad = r.scale_grad; s->rows_dropped = r.rows_dropped; s->pixels_isolated = r.pixels_isolated;
}

} // namespace

extern "C" {

#ifndef GDPT_BUILD_ARCH
#error "GDPT_BUILD_ARCH must name the --offload-arch the kernels were compiled for (csrc/Makefile passes it)"
#endif
const char *gdpt_build_arch(void) { return GDPT_BUILD_ARCH; }

// include/gdpt_debug.h: the work-item plan of the persistent kernels, for host-side tests (no GPU needed)
int gdpt_debug_chunk_plan(int spp, int force_log2k, long long film_pixels, long long resident_lanes, int32_t *begin, int capacity) {
    const gdpt::ChunkPlan p = gdpt::make_chunk_plan(spp, force_log2k, film_pixels, resident_lanes);
    if (!begin || capacity < p.n + 1) return -1;
    for (int c = 0; c <= p.n; c++) begin[c] = p.begin[c];
    return p.n;
}

// include/gdpt_debug.h: which kernel the calling thread's last render launched (render_kernels.hip: launch_render)
const char *gdpt_debug_last_route(void) { return gdpt::last_route(); }
const char *gdpt_debug_last_dct_shape(void) { return gdpt::last_dct_shape(); }
long long gdpt_debug_overlapped_launches(const GdptScene *scene) { return scene ? (long long)scene->overlapped : -1; }
int gdpt_debug_leaf_histogram(const GdptScene *scene, int32_t hist[4]) {
    return gdpt::guarded([&]() {
        if (!scene || !hist) throw std::runtime_error("gdpt_debug_leaf_histogram: null argument");
        for (int i = 0; i < 4; i++) hist[i] = scene->traits.leaf_hist[i];
    });
}
int gdpt_debug_route_names(const char **out, int capacity) { return gdpt::route_names(out, capacity); }

// include/gdpt_debug.h: the grid of an image-space launch, from the two rules the launches themselves call (image_kernels.h; no GPU
// needed). A stride rule counts `per_pixel` elements a pixel under `cap` blocks, at least `floor`; a tile rule has tw x th pixel tiles
// and reports the tiles, or with `pixel_groups` the groups of 256 pixels the same blocks stride over (pcg_step_b).
struct ImageGridRule { const char *name; int tw, th; bool pixel_groups; int per_pixel, cap, floor; };
const ImageGridRule kImageGridRules[] = {
    {"fold", 0, 0, false, 1, film::kMaxBlocks, 1},
    {"variance", 0, 0, false, 3, 4 * film::kMaxBlocks, 1},
    {"spread", 0, 0, false, 1, film::kMaxBlocks, 1},
    {"box", gdpt::kSpreadTileW, gdpt::kSpreadTileH, false, 0, 0, 0},
    {"nlm", gdpt::kNlmTile, gdpt::kNlmTile, false, 0, 0, 0},
    {"recon_tiles", rl1::kTileW, rl1::kTileH, false, 0, 0, 0},
    {"recon_pixels", rl1::kTileW, rl1::kTileH, true, 0, 0, 0},
    {"cg", 0, 0, false, 3, film::kMaxBlocks, 0},
};

int gdpt_debug_image_grid(const char *kernel, int width, int height, int32_t out[2]) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_image_grid";
        if (!kernel || !out) throw std::runtime_error(who + ": null argument");
        if (width < 1 || height < 1 || (long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width and height must be >= 1, the film at most 2^29 pixels");
        const std::string k(kernel);
        const size_t npix = (size_t)width * height;
        for (const ImageGridRule &r : kImageGridRules) {
            if (k != r.name) continue;
            if (r.tw == 0) { const film::StrideGrid g = film::stride_grid(r.per_pixel * npix, r.cap, r.floor); out[0] = g.blocks; out[1] = g.groups; }
            else {
                const film::TileGrid g = film::tile_grid(width, height, r.tw, r.th);
                out[0] = g.blocks; out[1] = r.pixel_groups ? film::stride_grid(npix, g.blocks).groups : g.tiles;
            }
            return;
        }
        std::string names;
        for (const ImageGridRule &r : kImageGridRules) names += std::string(names.empty() ? "" : ", ") + r.name;
        throw std::runtime_error(who + ": unknown kernel '" + k + "' (" + names + ")");
    });
}

int gdpt_scene_upload(const GdptSceneDesc *desc, int device, GdptScene **out_scene) {
    return gdpt::guarded([&]() {
        if (!out_scene) throw std::runtime_error("gdpt_scene_upload: null output");
        std::unique_ptr<GdptScene> sc(new GdptScene());
        build_scene(desc, device, sc.get());
        sc->scene_spp = desc->samples_per_pixel;
        *out_scene = sc.release();
    });
}

void gdpt_scene_free(GdptScene *scene) {
    if (!scene) return;
    delete scene;
}

int gdpt_scene_set_camera(GdptScene *scene, const GdptCamera *camera) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_scene_set_camera";
        if (!scene) throw std::runtime_error(who + ": scene is null");
        if (!camera) throw std::runtime_error(who + ": camera is null");
        const DevCamera &old = scene->view.cam;
        if (camera->width != old.width) throw std::runtime_error(who + ": width must stay as uploaded");
        if (camera->height != old.height) throw std::runtime_error(who + ": height must stay as uploaded");
        if (camera->filter_type != old.filter_type) throw std::runtime_error(who + ": filter_type must stay as uploaded");
        if (!(camera->filter_param == old.filter_param)) throw std::runtime_error(who + ": filter_param must stay as uploaded");
        for (int i = 0; i < 16; i++) {
            if (!std::isfinite(camera->sample_to_cam[i])) throw std::runtime_error(who + ": sample_to_cam has a non-finite entry");
            if (!std::isfinite(camera->cam_to_world[i])) throw std::runtime_error(who + ": cam_to_world has a non-finite entry");
        }
        // the tree is not rebuilt: its boxes keep the padding of the upload, which covers origins up to this extent (host/scene_prepare.cpp)
        if (!(gdpt::camera_extent(*camera) <= scene->traits.pad_extent))
            throw std::runtime_error(who + ": cam_to_world puts the camera outside the extent the scene was uploaded with");
        // (launches in flight hold their own copy of the view: it is a kernel argument)
        gdpt::fill_camera(*camera, &scene->view.cam);
    });
}

int gdpt_scene_info(const GdptScene *scene, int32_t *num_nodes, int32_t *num_tris, int32_t *num_spheres, int32_t *bvh_depth) {
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        if (num_nodes) *num_nodes = scene->view.num_nodes;
        if (num_tris) *num_tris = scene->view.num_tris;
        if (num_spheres) *num_spheres = scene->view.num_spheres;
        if (bvh_depth) *bvh_depth = scene->traits.bvh_depth;
    });
}

int gdpt_render_device(GdptScene *scene, const GdptRenderParams *params,
                       double *d_img, double *d_cx0, double *d_cy0, double *d_cx1, double *d_cy1,
                       void *stream, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        render_device_impl(scene, params, scene->scene_spp, d_img, d_cx0, d_cy0, d_cx1, d_cy1, (hipStream_t)stream, stats);
    });
}

int gdpt_render(GdptScene *scene, const GdptRenderParams *params,
                double *img, double *cx0, double *cy0, double *cx1, double *cy1, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        if (!img || !cx0 || !cy0 || !cx1 || !cy1) throw std::runtime_error("gdpt_render: null output buffer");
        ck(hipSetDevice(scene->device), "hipSetDevice");
        size_t elems = (size_t)scene->view.cam.width * scene->view.cam.height * 3;
        scene->ensure_buffers(elems);
        Band b = resolve(scene, params);
        double *host[5] = {img, cx0, cy0, cx1, cy1};
        // rows outside the band keep the caller's contents: upload them first when rendering a partial band
        bool partial = (b.row_begin != 0 || b.row_end != scene->view.cam.height);
        if (partial) for (int k = 0; k < 5; k++) ck(hipMemcpy(scene->d_buf[k], host[k], elems * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        GdptRenderStats local{};
        render_device_impl(scene, params, scene->scene_spp, scene->d_buf[0], scene->d_buf[1], scene->d_buf[2], scene->d_buf[3], scene->d_buf[4],
                           nullptr, stats ? stats : &local);
        for (int k = 0; k < 5; k++) ck(hipMemcpy(host[k], scene->d_buf[k], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

int gdpt_tile_row_costs(GdptScene *scene, int spp, double *cost, int capacity) {
    return gdpt::guarded([&]() {
        if (!scene || !cost) throw std::runtime_error("gdpt_tile_row_costs: null argument");
        const int H = scene->view.cam.height, T = (H + 15) / 16;
        if (capacity < T) throw std::runtime_error("gdpt_tile_row_costs: capacity < ceil(height / 16)");
        ck(hipSetDevice(scene->device), "hipSetDevice");
        scene->ensure_buffers((size_t)scene->view.cam.width * H * 3);
        for (int t = 0; t < T; t++) {       // one small launch per tile row; the counters are exact, so is the cost
            GdptRenderParams p{};
            p.spp = spp > 0 ? spp : 1; p.rng_scheme = GDPT_RNG_SAMPLE; p.row_begin = t * 16; p.row_end = std::min(H, t * 16 + 16);
            GdptRenderStats st{};
            render_device_impl(scene, &p, scene->scene_spp, scene->d_buf[0], scene->d_buf[1], scene->d_buf[2], scene->d_buf[3], scene->d_buf[4], nullptr, &st);
            cost[t] = (double)st.rays;
        }
    });
}

int gdpt_path_render_device(GdptScene *scene, const GdptRenderParams *params, double *d_img, void *stream, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        path_render_device_impl(scene, params, d_img, (hipStream_t)stream, stats, nullptr);
    });
}

int gdpt_render_window_device(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window,
                              double *d_img, double *d_cx0, double *d_cy0, double *d_cx1, double *d_cy1,
                              void *stream, GdptRenderStats *stats) {
    if (!window) return gdpt_render_device(scene, params, d_img, d_cx0, d_cy0, d_cx1, d_cy1, stream, stats);
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        render_device_impl(scene, params, scene->scene_spp, d_img, d_cx0, d_cy0, d_cx1, d_cy1, (hipStream_t)stream, stats, window);
    });
}

int gdpt_path_render_window_device(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window, double *d_img,
                                   void *stream, GdptRenderStats *stats) {
    if (!window) return gdpt_path_render_device(scene, params, d_img, stream, stats);
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        path_render_device_impl(scene, params, d_img, (hipStream_t)stream, stats, window);
    });
}

int gdpt_path_render(GdptScene *scene, const GdptRenderParams *params, double *img, GdptRenderStats *stats) {
    return gdpt::guarded([&]() {
        if (!scene) throw std::runtime_error("null scene handle");
        if (!img) throw std::runtime_error("gdpt_path_render: null output buffer");
        ck(hipSetDevice(scene->device), "hipSetDevice");
        size_t elems = (size_t)scene->view.cam.width * scene->view.cam.height * 3;
        scene->ensure_buffers(elems);
        Band b = resolve(scene, params);
        const bool partial = (b.row_begin != 0 || b.row_end != scene->view.cam.height);
        if (partial) ck(hipMemcpy(scene->d_buf[0], img, elems * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(H2D)");
        GdptRenderStats local{};
        path_render_device_impl(scene, params, scene->d_buf[0], nullptr, stats ? stats : &local, nullptr);
        ck(hipMemcpy(img, scene->d_buf[0], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

int gdpt_assemble_rows_device(int width, int height, int row_begin, int row_end, const double *d_img, const double *d_cx0, const double *d_cy0,
                              const double *d_cx1, const double *d_cy1, double *d_c, double *d_cx, double *d_cy, void *stream) {
    return gdpt::guarded([&]() {
        if (!d_img || !d_cx0 || !d_cy0 || !d_cx1 || !d_cy1 || !d_c || !d_cx || !d_cy) throw std::runtime_error("gdpt_assemble_device: null buffer");
        gdpt::launch_assemble(width, height, row_begin, row_end, d_img, d_cx0, d_cy0, d_cx1, d_cy1, d_c, d_cx, d_cy, (hipStream_t)stream);
    });
}
int gdpt_assemble_device(int width, int height, const double *d_img, const double *d_cx0, const double *d_cy0,
                         const double *d_cx1, const double *d_cy1, double *d_c, double *d_cx, double *d_cy, void *stream) {
    return gdpt_assemble_rows_device(width, height, 0, 0, d_img, d_cx0, d_cy0, d_cx1, d_cy1, d_c, d_cx, d_cy, stream);
}

int gdpt_assemble_solve_device(int width, int height, const double *d_img, const double *d_cx0, const double *d_cy0, const double *d_cx1, const double *d_cy1,
                               double *d_c, double *d_cx, double *d_cy, double dataCost, double *d_out, int solver, double tol, int max_iters,
                               void *stream, GdptPoissonStats *stats) {
    return gdpt::guarded([&]() {
        if (!d_img || !d_cx0 || !d_cy0 || !d_cx1 || !d_cy1 || !d_c || !d_cx || !d_cy || !d_out) throw std::runtime_error("gdpt_assemble_solve_device: null buffer");
        gdpt::PoissonResult r = gdpt::assemble_solve_device(width, height, d_img, d_cx0, d_cy0, d_cx1, d_cy1, d_c, d_cx, d_cy, dataCost, d_out, solver, tol, max_iters,
                                                            (hipStream_t)stream, stats != nullptr);
        fill_poisson_stats(stats, r);
    });
}

int gdpt_poisson_forget_stream(void *stream) {
    return gdpt::guarded([&]() {
        int dev = 0;
        ck(hipGetDevice(&dev), "hipGetDevice");
        gdpt::forget_stream(dev, (hipStream_t)stream);
    });
}

int gdpt_poisson_solve_device(int width, int height, const double *d_c, const double *d_gx, const double *d_gy,
                              double dataCost, double *d_out, int solver, double tol, int max_iters,
                              void *stream, GdptPoissonStats *stats) {
    return gdpt::guarded([&]() {
        if (!d_c || !d_gx || !d_gy || !d_out) throw std::runtime_error("gdpt_poisson_solve_device: null buffer");
        gdpt::PoissonResult r = gdpt::poisson_solve_device(width, height, d_c, d_gx, d_gy, dataCost, d_out, solver, tol, max_iters, (hipStream_t)stream, stats != nullptr);
        fill_poisson_stats(stats, r);
    });
}

int gdpt_poisson_solve_ex(int width, int height, const double *imgData, const double *imgGradX, const double *imgGradY,
                          double dataCost, double *imgOut, int solver, double tol, int max_iters, GdptPoissonStats *stats) {
    return gdpt::guarded([&]() {
        if (!imgData || !imgGradX || !imgGradY || !imgOut) throw std::runtime_error("gdpt_poisson_solve: null buffer");
        if (width <= 0 || height <= 0) throw std::runtime_error("gdpt_poisson_solve: empty image");
        int ndev = 0;
        ck(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
        if (ndev <= 0) throw std::runtime_error("gdpt_poisson_solve: no HIP device visible (this library has no CPU fallback)");
        on_device_planes({imgData, imgGradX, imgGradY}, width, height, imgOut, "hipMalloc(poisson io)", [&](const Planes &d) {
            fill_poisson_stats(stats, gdpt::poisson_solve_device(width, height, d[0], d[1], d[2], dataCost, d[3], solver, tol, max_iters, nullptr, stats != nullptr));
        });
    });
}

int gdpt_poisson_solve(int width, int height, const double *imgData, const double *imgGradX, const double *imgGradY,
                       double dataCost, double *imgOut) {
    return gdpt_poisson_solve_ex(width, height, imgData, imgGradX, imgGradY, dataCost, imgOut, GDPT_SOLVER_DEFAULT, 0.0, 0, nullptr);
}

int gdpt_gradient_path_render(GdptScene *scene, const GdptRenderParams *params, double dataCost, double *out_image,
                              double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                              GdptRenderStats *rstats, GdptPoissonStats *pstats) {
    return gdpt::guarded([&]() {
        if (!scene || !out_image) throw std::runtime_error("gdpt_gradient_path_render: null argument");
        ck(hipSetDevice(scene->device), "hipSetDevice");
        const int w = scene->view.cam.width, h = scene->view.cam.height;
        size_t elems = (size_t)w * h * 3;
        scene->ensure_buffers(elems);
        auto &b = scene->d_buf;
        GdptRenderParams p = params ? *params : GdptRenderParams{};
        p.row_begin = 0; p.row_end = 0;   // the solve is global: whole image only
        GdptRenderStats local{};
        render_device_impl(scene, &p, scene->scene_spp, b[0], b[1], b[2], b[3], b[4], nullptr, rstats ? rstats : &local);
        gdpt::PoissonResult r = gdpt::assemble_solve_device(w, h, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], dataCost, b[8], GDPT_SOLVER_DEFAULT, 0.0, 0, nullptr, pstats != nullptr);
        fill_poisson_stats(pstats, r);
        ck(hipMemcpy(out_image, b[8], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        double *host[5] = {img, cx0, cy0, cx1, cy1};
        for (int k = 0; k < 5; k++) if (host[k]) ck(hipMemcpy(host[k], b[k], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

int gdpt_reconstruct_device(int width, int height, const double *d_c, const double *d_gx, const double *d_gy, double dataCost,
                            const GdptReconParams *params, double *d_out, void *stream, GdptReconStats *stats) {
    if (!params || params->norm == GDPT_RECON_L2) {
        GdptPoissonStats ps{};
        const int rc = gdpt_poisson_solve_device(width, height, d_c, d_gx, d_gy, dataCost, d_out, GDPT_SOLVER_DEFAULT, 0.0, 0, stream, stats ? &ps : nullptr);
        if (rc == 0) fill_recon_stats_l2(stats, ps.solve_ms);
        return rc;
    }
    return gdpt::guarded([&]() {
        if (!d_c || !d_gx || !d_gy || !d_out) throw std::runtime_error("gdpt_reconstruct_device: null buffer");
        const gdpt::ReconL1Params p = resolve_recon(*params);
        fill_recon_stats(stats, gdpt::recon_l1_device(width, height, d_c, d_gx, d_gy, dataCost, p, d_out, (hipStream_t)stream));
    });
}

int gdpt_reconstruct(int width, int height, const double *c, const double *gx, const double *gy, double dataCost,
                     const GdptReconParams *params, double *out, GdptReconStats *stats) {
    if (!params || params->norm == GDPT_RECON_L2) {
        GdptPoissonStats ps{};
        const int rc = gdpt_poisson_solve_ex(width, height, c, gx, gy, dataCost, out, GDPT_SOLVER_DEFAULT, 0.0, 0, stats ? &ps : nullptr);
        if (rc == 0) fill_recon_stats_l2(stats, ps.solve_ms);
        return rc;
    }
    return gdpt::guarded([&]() {
        if (!c || !gx || !gy || !out) throw std::runtime_error("gdpt_reconstruct: null buffer");
        if (width < 2 || height < 2) throw std::runtime_error("gdpt_reconstruct: width and height must be >= 2");
        const gdpt::ReconL1Params p = resolve_recon(*params);
        int ndev = 0;
        ck(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
        if (ndev <= 0) throw std::runtime_error("gdpt_reconstruct: no HIP device visible (this library has no CPU fallback)");
        on_device_planes({c, gx, gy}, width, height, out, "hipMalloc(reconstruct io)", [&](const Planes &d) {
            fill_recon_stats(stats, gdpt::recon_l1_device(width, height, d[0], d[1], d[2], dataCost, p, d[3], nullptr));
        });
    });
}

int gdpt_reconstruct_weighted_device(int width, int height, const double *d_c, const double *d_gx, const double *d_gy,
                                     const double *d_var_c, const double *d_var_gx, const double *d_var_gy, double dataCost,
                                     const GdptWeightedReconParams *params, double *d_out, double *const d_confidence[3], void *stream,
                                     GdptWeightedReconStats *stats) {
    return gdpt::guarded([&]() {
        if (!d_c || !d_gx || !d_gy || !d_out) throw std::runtime_error("gdpt_reconstruct_weighted_device: null buffer");
        if (!d_var_c || !d_var_gx || !d_var_gy) throw std::runtime_error("gdpt_reconstruct_weighted_device: null variance plane");
        double conf_floor = 0;
        int norm = 0;
        const gdpt::ReconL1Params p = resolve_weighted(params, &conf_floor, &norm);
        fill_weighted_stats(stats, norm, gdpt::recon_weighted_device(width, height, d_c, d_gx, d_gy, d_var_c, d_var_gx, d_var_gy, dataCost, p, conf_floor,
                                                                     d_out, d_confidence, (hipStream_t)stream));
    });
}

int gdpt_reconstruct_weighted(int width, int height, const double *c, const double *gx, const double *gy, const double *var_c,
                              const double *var_gx, const double *var_gy, double dataCost, const GdptWeightedReconParams *params, double *out,
                              double *const confidence[3], GdptWeightedReconStats *stats) {
    return gdpt::guarded([&]() {
        if (!c || !gx || !gy || !out) throw std::runtime_error("gdpt_reconstruct_weighted: null buffer");
        if (!var_c || !var_gx || !var_gy) throw std::runtime_error("gdpt_reconstruct_weighted: null variance plane");
        if (width < 2 || height < 2) throw std::runtime_error("gdpt_reconstruct_weighted: width and height must be >= 2");
        if (!(dataCost > 0) || !std::isfinite(dataCost)) throw std::runtime_error("gdpt_reconstruct_weighted: dataCost must be finite and > 0");
        for (const double *in : {c, gx, gy, var_c, var_gx, var_gy}) if (out == in) throw std::runtime_error("gdpt_reconstruct_weighted: the output must not alias an input");
        double conf_floor = 0;
        int norm = 0;
        const gdpt::ReconL1Params p = resolve_weighted(params, &conf_floor, &norm);
        int ndev = 0;
        ck(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
        if (ndev <= 0) throw std::runtime_error("gdpt_reconstruct_weighted: no HIP device visible (this library has no CPU fallback)");
        on_device_planes({c, gx, gy, var_c, var_gx, var_gy}, width, height, out, "hipMalloc(reconstruct io)", [&](const Planes &d) {
            fill_weighted_stats(stats, norm, gdpt::recon_weighted_device(width, height, d[0], d[1], d[2], d[3], d[4], d[5], dataCost, p, conf_floor, d[6],
                                                                         confidence, nullptr));
        });
    });
}

int gdpt_gradient_path_render_recon(GdptScene *scene, const GdptRenderParams *params, double dataCost, const GdptReconParams *recon,
                                    double *out_image, double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                                    GdptRenderStats *rstats, GdptReconStats *cstats) {
    if (!recon || recon->norm == GDPT_RECON_L2) {
        GdptPoissonStats ps{};
        const int rc = gdpt_gradient_path_render(scene, params, dataCost, out_image, img, cx0, cy0, cx1, cy1, rstats, cstats ? &ps : nullptr);
        if (rc == 0) fill_recon_stats_l2(cstats, ps.solve_ms);
        return rc;
    }
    return gdpt::guarded([&]() {
        if (!scene || !out_image) throw std::runtime_error("gdpt_gradient_path_render_recon: null argument");
        const gdpt::ReconL1Params rp = resolve_recon(*recon);
        ck(hipSetDevice(scene->device), "hipSetDevice");
        const int w = scene->view.cam.width, h = scene->view.cam.height;
        size_t elems = (size_t)w * h * 3;
        scene->ensure_buffers(elems);
        auto &b = scene->d_buf;
        GdptRenderParams p = params ? *params : GdptRenderParams{};
        p.row_begin = 0; p.row_end = 0;   // the reconstruction is global: whole image only
        GdptRenderStats local{};
        render_device_impl(scene, &p, scene->scene_spp, b[0], b[1], b[2], b[3], b[4], nullptr, rstats ? rstats : &local);
        gdpt::launch_assemble(w, h, 0, 0, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr);
        fill_recon_stats(cstats, gdpt::recon_l1_device(w, h, b[5], b[6], b[7], dataCost, rp, b[8], nullptr));
        ck(hipMemcpy(out_image, b[8], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        double *host[5] = {img, cx0, cy0, cx1, cy1};
        for (int k = 0; k < 5; k++) if (host[k]) ck(hipMemcpy(host[k], b[k], elems * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
