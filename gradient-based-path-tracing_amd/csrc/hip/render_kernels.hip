// render_kernels.hip — route choice and launch dispatch of the GDPT render kernels (device code: render_device.h).
#include "render_twosided.h"
#include "render_wavefront.h"

#include "../capi_common.h"
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

namespace gdpt {

namespace {
thread_local const char *g_route = "";
// include/gdpt_debug.h lists what they mean; the order is that of enum Route
const char *const kRouteNames[] = {
    "lambert_plain/lds_const", "lambert_plain/lds_tex", "lambert_plain/hbm_const", "lambert_plain/hbm_tex",
    "lambert/lds_wide", "lambert/lds_bvh2", "lambert/hbm",
    "lambert_stamped/lds_plain", "lambert_stamped/lds", "lambert_stamped/hbm",
    "general_set_a/disney_diffuse", "general_set_a/disney_metal", "general_set_b/disney_clearcoat", "general_set_b/disney_sheen",
    "general/lds_wide", "general/lds_bvh2", "general/hbm",
    "twosided/lds", "twosided/hbm", "twosided/hbm_glass",
    "wavefront/lambert", "wavefront/general",
    "eager", "tile_eager", "tile_phases_lambert", "tile_phases_general",
    "reconnect/lds_lambert", "reconnect/hbm_lambert", "reconnect/general",
    "path/tile", "path/eager",
    "path_persistent/lds_lambert_plain", "path_persistent/lds_lambert", "path_persistent/lds_lambert_env",
    "path_persistent/hbm_lambert", "path_persistent/hbm_lambert_env",
    "path_persistent/lds_general", "path_persistent/lds_general_env", "path_persistent/hbm_general", "path_persistent/hbm_general_env",
};
constexpr int kNumRoutes = (int)(sizeof(kRouteNames) / sizeof(kRouteNames[0]));
static_assert(kNumRoutes == (int)Route::COUNT, "one name per Route");
} // namespace
const char *route_name(Route r) { return kRouteNames[(int)r]; }
void set_route(Route r) { g_route = route_name(r); }
void reset_route() { g_route = ""; }
const char *last_route() { return g_route; }
int route_names(const char **out, int capacity) {
    if (!out) return kNumRoutes;
    if (capacity < kNumRoutes) return -1;
    for (int i = 0; i < kNumRoutes; i++) out[i] = kRouteNames[i];
    return kNumRoutes;
}

Route choose_route(const RouteInputs &in) {
    const bool sample = in.rng_scheme == GDPT_RNG_SAMPLE;
    if (!sample && in.rng_scheme != GDPT_RNG_TILE) throw std::runtime_error("choose_route: unknown rng_scheme");
    const bool no_spheres = !in.has_spheres && !in.no_plain_kernel;   // kernels built without sphere code
    if (in.path) {
        // LDS-resident scenes are walked in their BVH4 form
        const bool lds = in.fits_lds_wide && !in.no_lds_scene;
        if (!sample) return Route::PATH_TILE;
        if (in.force_eager) return Route::PATH_EAGER;
        if (in.lambert_only) {
            if (lds && no_spheres && in.const_textures && !in.has_envmap) return Route::PATH_PERSISTENT_LDS_LAMBERT_PLAIN;
            return lds ? (in.has_envmap ? Route::PATH_PERSISTENT_LDS_LAMBERT_ENV : Route::PATH_PERSISTENT_LDS_LAMBERT)
                       : (in.has_envmap ? Route::PATH_PERSISTENT_HBM_LAMBERT_ENV : Route::PATH_PERSISTENT_HBM_LAMBERT);
        }
        return lds ? (in.has_envmap ? Route::PATH_PERSISTENT_LDS_GENERAL_ENV : Route::PATH_PERSISTENT_LDS_GENERAL)
                   : (in.has_envmap ? Route::PATH_PERSISTENT_HBM_GENERAL_ENV : Route::PATH_PERSISTENT_HBM_GENERAL);
    }
    const bool fits = in.fits_lds && !in.no_lds_scene;            // the scene is copied to LDS ...
    const bool wide = fits && in.lds_wide && in.fits_lds_wide;     // ... in its BVH4 form
    if (in.shift_mode == GDPT_SHIFT_RECONNECT) {
        // straight per-sample loop; the general kernel walks the HBM tree
        if (!sample) throw std::runtime_error("choose_route: GDPT_SHIFT_RECONNECT needs GDPT_RNG_SAMPLE");
        return !in.lambert_only ? Route::RECONNECT_GENERAL : wide ? Route::RECONNECT_LDS_LAMBERT : Route::RECONNECT_HBM_LAMBERT;
    }
    const bool one_sided = in.one_sided && !in.has_rough;          // the phase machine with lazy offsets is exact
    // two-sided lobes (DisneyGlass, DisneyBSDF) without rough ones: lane machine with offsets replayed from a bounce log
    // (a depth bound that lets a path outrun the replay's bounce log takes the straight-loop evaluator: render_twosided.h)
    const bool two_sided = !in.one_sided && !in.has_rough && !in.force_eager && sample && !in.no_twosided_machine &&
                           twosided_log_covers(in.max_depth, in.rr_depth);
    const bool phases = (one_sided || two_sided) && !in.force_eager;
    if (!sample) return !phases ? Route::TILE_EAGER : in.lambert_only ? Route::TILE_PHASES_LAMBERT : Route::TILE_PHASES_GENERAL;
    if (!phases) return Route::EAGER;
    // scenes walked from HBM with one-sided lobes: the wavefront pipeline (knob; the product default is the lane machine)
    if (in.wavefront && one_sided && !fits && in.shift_mode == GDPT_SHIFT_REFERENCE && !two_sided)
        return in.lambert_only ? Route::WAVEFRONT_LAMBERT : Route::WAVEFRONT_GENERAL;
    const unsigned mask = in.full_material_switch ? 0x1FFu : in.material_mask;
    if (two_sided) return wide ? Route::TWOSIDED_LDS : (mask & ~gd::kSetGlass) == 0 ? Route::TWOSIDED_HBM_GLASS : Route::TWOSIDED_HBM;
    if (in.lambert_only && in.stamps && (!fits || wide))
        return !fits ? Route::LAMBERT_STAMPED_HBM : (no_spheres && in.const_textures) ? Route::LAMBERT_STAMPED_LDS_PLAIN : Route::LAMBERT_STAMPED_LDS;
    if (in.lambert_only && no_spheres && (!fits || wide))
        return fits ? (in.const_textures ? Route::LAMBERT_PLAIN_LDS_CONST : Route::LAMBERT_PLAIN_LDS_TEX)
                    : (in.const_textures ? Route::LAMBERT_PLAIN_HBM_CONST : Route::LAMBERT_PLAIN_HBM_TEX);
    if (in.lambert_only) return !fits ? Route::LAMBERT_HBM : wide ? Route::LAMBERT_LDS_WIDE : Route::LAMBERT_LDS_BVH2;
    // HBM triangle scenes of Lambertian + one Disney lobe: the kernel built for that set (render_phases_general_sets.h)
    auto only = [&](int lobe) { return (mask & ~(1u << GDPT_MAT_LAMBERTIAN | 1u << lobe)) == 0; };
    if (!fits && no_spheres) {
        if (only(GDPT_MAT_DISNEY_DIFFUSE)) return Route::GENERAL_SET_A_DISNEY_DIFFUSE;
        if (only(GDPT_MAT_DISNEY_METAL)) return Route::GENERAL_SET_A_DISNEY_METAL;
        if (only(GDPT_MAT_DISNEY_CLEARCOAT)) return Route::GENERAL_SET_B_DISNEY_CLEARCOAT;
        if (only(GDPT_MAT_DISNEY_SHEEN)) return Route::GENERAL_SET_B_DISNEY_SHEEN;
    }
    return !fits ? Route::GENERAL_HBM : wide ? Route::GENERAL_LDS_WIDE : Route::GENERAL_LDS_BVH2;
}

// Straight per-sample loops: K = 2^log2k lanes per pixel, blocks of kBlock / K pixels in tiles of tile_w x tile_h.
static dim3 static_mapping(gd::KernelArgs &a, const RenderLaunch &rl, int W, int rows) {
    const long long pixels = (long long)W * rows;
    int log2k = 0;
    while ((1 << (log2k + 1)) <= rl.spp && log2k < 6 && (pixels << log2k) < (1LL << 19)) log2k++;
    if (rl.force_log2k >= 0) { log2k = rl.force_log2k; while (log2k > 0 && (1 << log2k) > rl.spp) log2k--; }
    a.log2k = log2k;
    const int ppb = gd::kBlock >> log2k;                 // pixels per block
    a.tile_w = ppb >= 16 ? 16 : ppb;
    a.tile_h = ppb / a.tile_w;
    a.tiles_x = (W + a.tile_w - 1) / a.tile_w;
    return dim3((unsigned)(a.tiles_x * ((rows + a.tile_h - 1) / a.tile_h)));
}

// Persistent lanes pulling (pixel, chunk) items of rl.plan: the item layout (render_device.h: item_to_pixel), the queue reset
// and the grid.
static dim3 start_queue(gd::KernelArgs &a, const RenderLaunch &rl, int W, hipStream_t stream) {
    a.num_chunks = rl.plan.n;
    for (int c = 0; c <= rl.plan.n; c++) a.chunk_begin[c] = rl.first_sample + rl.plan.begin[c];   // a sample's index in its pixel's stream block
    a.tiles_x = (W + 15) / 16;
    a.num_slots = band_slots(W, rl.row_end - rl.row_begin);
    a.num_items = a.num_slots * rl.plan.n;
    if (a.num_items >= (1LL << 32)) throw std::runtime_error("launch_render: image band too large for the 32-bit work queue");
    a.partials = rl.partials; a.queue_head = rl.queue_head;
    if (!a.partials || !a.queue_head) throw std::runtime_error("launch_render: work-queue buffers missing");
    if (!rl.resets_enqueued && hipMemsetAsync(a.queue_head, 0, sizeof(unsigned long long), stream) != hipSuccess) throw std::runtime_error("launch_render: queue reset failed");
    return dim3(persistent_blocks(rl, a.num_items));
}

int wf_words() { return gd::WF_WORDS; }
int wf_max_generations() { return gd::kWfMaxGen; }
int wf_slot_count(long long num_items) {
    long long n = num_items < (1LL << 21) ? num_items : (1LL << 21);       // 2 M slots = 0.75 GB of path state
    n = (n + gd::kBlock - 1) / gd::kBlock * gd::kBlock;
    return (int)(n < gd::kBlock ? gd::kBlock : n);
}
// layout of the auxiliary block: rays | hits | keys | hist | offsets | overflow stacks (all 16-byte aligned)
namespace {
struct WfAux { size_t rays, hits, keys, hist, offsets, blocks, ovf, total; };
WfAux wf_aux_layout(int slots) {
    WfAux l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    l.rays = take((size_t)slots * 32); l.hits = take((size_t)slots * 32); l.keys = take((size_t)slots * 8);
    l.hist = take((size_t)gd::kWfBins * 4); l.offsets = take((size_t)gd::kWfBins * 4);
    l.blocks = take((size_t)(slots / gd::kBlock) * 16);
    l.ovf = take((size_t)slots * (size_t)(GDPT_BVH_MAX_DEPTH - gd::kWfLdsLevels) * 4);
    l.total = off;
    return l;
}
}
size_t wf_aux_bytes(int slots) { return wf_aux_layout(slots).total; }

// Generations are enqueued in chunks; the host reads the number of slots that still need a step one chunk behind the
// launches (the speculative chunk behind a finished render finds nothing to do: its kernels return at once).
static void run_wavefront(const DevSceneView &sv, const gd::KernelArgs &a, const RenderLaunch &rl, bool lambert, hipStream_t stream) {
    static_assert(GDPT_BVH_MAX_DEPTH > gd::kWfLdsLevels, "overflow stack levels");
    const WfAux lay = wf_aux_layout(rl.wf_slots);
    char *aux = (char *)rl.wf_aux;
    gd::WfBuf w{};
    w.state = rl.wf_state; w.live = rl.wf_live; w.counters = rl.wf_counters; w.n = rl.wf_slots; w.gen = 0;
    w.rays = (float4 *)(aux + lay.rays); w.hits = (float4 *)(aux + lay.hits); w.keys = (uint2 *)(aux + lay.keys);
    w.hist = (unsigned *)(aux + lay.hist); w.offsets = (unsigned *)(aux + lay.offsets);
    w.block_counts = (uint4 *)(aux + lay.blocks); w.totals = rl.counters;
    w.sort = rl.wf_sort; w.tiles_x = (sv.cam.width + 15) / 16;
    for (int k = 0; k < 3; k++) {
        const float lo = rl.wf_bounds[k], hi = rl.wf_bounds[3 + k];
        w.bmin[k] = lo;
        w.cell_scale[k] = (hi > lo) ? 16.0f / (hi - lo) : 0.0f;
    }
    gd::WfTrace t{};
    t.nodes4 = sv.nodes4; t.nodes4q = sv.nodes4q; t.prims = sv.prims; t.spheres = sv.spheres; t.rays = w.rays; t.hits = w.hits; t.live = w.live;
    t.ovf = (int *)(aux + lay.ovf); t.ovf_stride = (unsigned)rl.wf_slots; t.counters = rl.counters;
    t.num_tris = sv.num_tris; t.num_nodes4 = sv.num_nodes4; t.num_spheres = sv.num_spheres; t.search_frac = a.thresh_c; t.count_stats = a.count;
    auto ckh = [](hipError_t e, const char *what) { if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); };
    ckh(hipMemsetAsync(rl.wf_counters, 0, sizeof(unsigned) * 3 * gd::kWfMaxGen, stream), "hipMemsetAsync(wavefront counters)");
    ckh(hipMemsetAsync(w.hist, 0, sizeof(unsigned) * gd::kWfBins, stream), "hipMemsetAsync(wavefront histogram)");
    launch_wf_init(w, stream);
    // The trace grid covers the slots that can still hold a ray: all of them until the host has seen a generation with
    // fewer active slots (from then on the work queue is empty and the number only falls). The kernel strides over the
    // queue, so a grid that is too small would still be correct.
    unsigned active_bound = (unsigned)rl.wf_slots;
    const int chunk = 8;
    int gen = 0;
    auto enqueue_chunk = [&]() {
        for (int k = 0; k < chunk; k++, gen++) {
            if (gen >= gd::kWfMaxGen) throw std::runtime_error("launch_render: wavefront generation limit reached");
            w.gen = gen;
            if (lambert) launch_wf_step_lambert(sv, a, w, stream); else launch_wf_step_general(sv, a, w, stream);
            launch_wf_sort(w, stream);
            t.count = rl.wf_counters + gen;
            launch_wf_trace(t, sv.num_spheres > 0, (active_bound + gd::kWfTraceBlock - 1) / gd::kWfTraceBlock, stream);
        }
    };
    enqueue_chunk();
    for (;;) {
        ckh(hipMemcpyAsync(rl.wf_host, rl.wf_counters + 2 * gd::kWfMaxGen + (gen - 1), sizeof(unsigned), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(wavefront live count)");
        ckh(hipEventRecord(rl.wf_event, stream), "hipEventRecord");
        const bool room = gen + chunk <= gd::kWfMaxGen;
        if (room) enqueue_chunk();
        ckh(hipEventSynchronize(rl.wf_event), "hipEventSynchronize");
        if (*rl.wf_host == 0u) break;
        if (*rl.wf_host < active_bound) active_bound = *rl.wf_host;
        if (!room) throw std::runtime_error("launch_render: wavefront generation limit reached");
    }
}

// The dynamic LDS of a lane machine on an LDS-resident scene: the one place that lays it out (launch_render's kernel arguments and
// render_free_lds_per_cu both come from here).
static gd::LdsLayout phases_lds_layout(const DevSceneView &sv, const RenderLaunch &rl) {
    const bool wide = !walks_bvh2(rl.route);
    const gd::LdsSceneCounts c{wide ? sv.num_nodes4 : sv.num_nodes, sv.num_prims, sv.num_tris, sv.num_materials, sv.num_lights};
    const gd::LdsLayout l = gd::lds_scene_layout(wide, c, rl.lds_stack_need, rl.lds_fixed_layout);
    if (!l.ok) throw std::runtime_error("launch_render: the scene does not fit the block's LDS copy");
    return l;
}
int render_free_lds_per_cu(const DevSceneView &sv, const RenderLaunch &rl) {
    if (!phases_lds_scene(rl.route)) return 0;
    const int setup = (has_setup_batch(rl.route) && !rl.no_setup_batch) ? gd::kPhasesSetupLds : 0;      // s_setup of the SETUP builds
    const int per_block = gd::lds_allocated(gd::kPhasesStaticLds + setup + (is_stamped(rl.route) ? gd::kPhasesStampLds : 0) + phases_lds_layout(sv, rl).total);
    const int left = gd::kLdsPerCu - (rl.blocks_per_cu > 0 ? rl.blocks_per_cu : 2) * per_block;
    return left > 0 ? left : 0;
}
namespace {
struct BesideHint { const void *owner = nullptr; int free_lds = 0; };
std::mutex g_hint_mu;
std::map<int, BesideHint> &g_hints = *new std::map<int, BesideHint>();     // (leaked on purpose, like the solver's registries)
}
void set_render_beside_hint(int device, const void *owner, int free_lds_per_cu) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    BesideHint &h = g_hints[device];
    h.owner = owner; h.free_lds = free_lds_per_cu;
}
void clear_render_beside_hint(int device, const void *owner) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    auto it = g_hints.find(device);
    if (it != g_hints.end() && it->second.owner == owner) it->second = BesideHint();
}
int render_beside_hint(int device) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    auto it = g_hints.find(device);
    return it == g_hints.end() ? 0 : it->second.free_lds;
}

void launch_render(const DevSceneView &sv, const RenderLaunch &rl, hipStream_t stream) {
    const Route r = rl.route;
    // an overlapped launch (rl.kernel_stream): queue reset and render kernel on that stream; what writes the images stays on `stream`
    if (rl.kernel_stream && (!can_overlap(r) || !rl.kernel_done)) throw std::runtime_error("launch_render: this route does not overlap");
    if (rl.resets_enqueued && !rl.kernel_stream) throw std::runtime_error("launch_render: resets enqueued ahead of a launch that does not overlap");
    const hipStream_t ks = rl.kernel_stream ? rl.kernel_stream : stream;
    gd::KernelArgs a{};
    a.spp = rl.spp; a.stream_spp = rl.stream_spp; a.first_sample = rl.first_sample; a.row_begin = rl.row_begin; a.row_end = rl.row_end; a.max_depth = rl.max_depth;
    a.img = rl.img; a.cx0 = rl.cx0; a.cy0 = rl.cy0; a.cx1 = rl.cx1; a.cy1 = rl.cy1; a.counters = rl.counters;
    // trace phase is left when this fraction (/256) of the rays that entered it is still unfinished
    a.thresh_a = rl.thresh_a >= 0 ? (rl.thresh_a > 255 ? 255 : rl.thresh_a) : 64;
    // ... and its inner-node loop when this fraction of the live rays is still looking for the next leaf
    a.thresh_c = rl.thresh_c >= 0 ? (rl.thresh_c > 255 ? 255 : rl.thresh_c) : 112;
    a.count = rl.count_traversal ? 1 : 0;
    const int W = sv.cam.width, rows = rl.row_end - rl.row_begin;
    if (W <= 0 || rows <= 0 || rl.spp <= 0) throw std::runtime_error("launch_render: empty image band or spp <= 0");
    if (rl.first_sample < 0 || (long long)rl.first_sample + rl.spp > (long long)rl.stream_spp) throw std::runtime_error("launch_render: sample window outside its stream block");
    const int ntx = (W + 15) / 16, nty = (sv.cam.height + 15) / 16;    // tile streams: one lane per 16x16 tile
    dim3 grid((unsigned)((ntx * nty + 63) / 64));
    if (is_persistent(r)) {
        // scenes walked from HBM: stack slots = the tree's own bound (host-verified at upload)
        a.stack_levels = rl.wide_stack_need > 0 ? rl.wide_stack_need : GDPT_BVH_MAX_DEPTH;
        a.replay_per_step = rl.replay_per_step >= 1 ? rl.replay_per_step : 4;       // render_twosided.h: kReplayPerStep
        if (a.stack_levels > GDPT_BVH_MAX_DEPTH) throw std::runtime_error("launch_render: traversal stack bound exceeds the builder's maximum");
        if (phases_lds_scene(r)) {          // the stack and the scene copy behind it, both sized from the scene (lds_layout.h)
            const gd::LdsLayout l = phases_lds_layout(sv, rl);
            a.stack_levels = l.stack_levels; a.lds_scene_bytes = l.total - l.scene_off;
        }
        grid = start_queue(a, rl, W, ks);
    }
    if (needs_bounce_log(r) && (!rl.bounce_log || rl.bounce_log_bytes < twosided_log_bytes(grid.x))) throw std::runtime_error("launch_render: bounce log missing");
    if (is_wavefront(r) && (!rl.wf_state || !rl.wf_live || !rl.wf_counters || !rl.wf_host || !rl.wf_aux || rl.wf_slots <= 0))
        throw std::runtime_error("launch_render: wavefront buffers missing");
    set_route(r);
    const bool wl = rl.whole_leaf_trips;       // (knob; read by the LDS-resident one-sided lane machines only)
    const bool sb = !rl.no_setup_batch;        // (knob; read by the has_setup_batch routes only)
    switch (r) {
    case Route::LAMBERT_PLAIN_LDS_CONST: launch_phases_lambert_plain(sv, a, grid, true, true, wl, sb, ks); break;
    case Route::LAMBERT_PLAIN_LDS_TEX: launch_phases_lambert_plain(sv, a, grid, true, false, wl, false, ks); break;
    case Route::LAMBERT_PLAIN_HBM_CONST: launch_phases_lambert_plain(sv, a, grid, false, true, wl, false, ks); break;
    case Route::LAMBERT_PLAIN_HBM_TEX: launch_phases_lambert_plain(sv, a, grid, false, false, wl, false, ks); break;
    case Route::LAMBERT_LDS_WIDE: launch_phases_lambert(sv, a, grid, true, true, wl, ks); break;
    case Route::LAMBERT_LDS_BVH2: launch_phases_lambert(sv, a, grid, true, false, wl, ks); break;
    case Route::LAMBERT_HBM: launch_phases_lambert(sv, a, grid, false, false, wl, ks); break;
    case Route::LAMBERT_STAMPED_LDS_PLAIN: launch_phases_lambert_stamped(sv, a, grid, true, true, wl, sb, stream); break;
    case Route::LAMBERT_STAMPED_LDS: launch_phases_lambert_stamped(sv, a, grid, true, false, wl, false, stream); break;
    case Route::LAMBERT_STAMPED_HBM: launch_phases_lambert_stamped(sv, a, grid, false, false, wl, false, stream); break;
    case Route::GENERAL_SET_A_DISNEY_DIFFUSE: launch_phases_general_set_a(sv, a, grid, GDPT_MAT_DISNEY_DIFFUSE, ks); break;
    case Route::GENERAL_SET_A_DISNEY_METAL: launch_phases_general_set_a(sv, a, grid, GDPT_MAT_DISNEY_METAL, ks); break;
    case Route::GENERAL_SET_B_DISNEY_CLEARCOAT: launch_phases_general_set_b(sv, a, grid, GDPT_MAT_DISNEY_CLEARCOAT, ks); break;
    case Route::GENERAL_SET_B_DISNEY_SHEEN: launch_phases_general_set_b(sv, a, grid, GDPT_MAT_DISNEY_SHEEN, ks); break;
    case Route::GENERAL_LDS_WIDE: launch_phases_general(sv, a, grid, true, true, wl, ks); break;
    case Route::GENERAL_LDS_BVH2: launch_phases_general(sv, a, grid, true, false, wl, ks); break;
    case Route::GENERAL_HBM: launch_phases_general(sv, a, grid, false, false, wl, ks); break;
    case Route::TWOSIDED_LDS: launch_phases_twosided(sv, a, grid, true, rl.bounce_log, stream); break;
    case Route::TWOSIDED_HBM: launch_phases_twosided(sv, a, grid, false, rl.bounce_log, stream); break;
    case Route::TWOSIDED_HBM_GLASS: launch_phases_twosided_glass(sv, a, grid, rl.bounce_log, stream); break;
    case Route::WAVEFRONT_LAMBERT: run_wavefront(sv, a, rl, true, stream); break;
    case Route::WAVEFRONT_GENERAL: run_wavefront(sv, a, rl, false, stream); break;
    case Route::EAGER: launch_eager(sv, a, static_mapping(a, rl, W, rows), stream); break;
    case Route::TILE_EAGER: launch_tile_eager(sv, a, grid, ntx, nty, stream); break;
    case Route::TILE_PHASES_LAMBERT: launch_tile_phases_lambert(sv, a, grid, ntx, nty, stream); break;
    case Route::TILE_PHASES_GENERAL: launch_tile_phases_general(sv, a, grid, ntx, nty, stream); break;
    case Route::RECONNECT_LDS_LAMBERT: launch_reconnect(sv, a, static_mapping(a, rl, W, rows), true, true, stream); break;
    case Route::RECONNECT_HBM_LAMBERT: launch_reconnect(sv, a, static_mapping(a, rl, W, rows), false, true, stream); break;
    case Route::RECONNECT_GENERAL: launch_reconnect(sv, a, static_mapping(a, rl, W, rows), false, false, stream); break;
    case Route::PATH_TILE: launch_tile_path(sv, a, grid, ntx, nty, stream); break;
    case Route::PATH_EAGER: launch_path(sv, a, static_mapping(a, rl, W, rows), stream); break;
    case Route::PATH_PERSISTENT_LDS_LAMBERT_PLAIN: launch_path_persistent(sv, a, grid, true, true, false, true, stream); break;
    case Route::PATH_PERSISTENT_LDS_LAMBERT: launch_path_persistent(sv, a, grid, true, true, false, false, stream); break;
    case Route::PATH_PERSISTENT_LDS_LAMBERT_ENV: launch_path_persistent(sv, a, grid, true, true, true, false, stream); break;
    case Route::PATH_PERSISTENT_HBM_LAMBERT: launch_path_persistent(sv, a, grid, true, false, false, false, stream); break;
    case Route::PATH_PERSISTENT_HBM_LAMBERT_ENV: launch_path_persistent(sv, a, grid, true, false, true, false, stream); break;
    case Route::PATH_PERSISTENT_LDS_GENERAL: launch_path_persistent(sv, a, grid, false, true, false, false, stream); break;
    case Route::PATH_PERSISTENT_LDS_GENERAL_ENV: launch_path_persistent(sv, a, grid, false, true, true, false, stream); break;
    case Route::PATH_PERSISTENT_HBM_GENERAL: launch_path_persistent(sv, a, grid, false, false, false, false, stream); break;
    case Route::PATH_PERSISTENT_HBM_GENERAL_ENV: launch_path_persistent(sv, a, grid, false, false, true, false, stream); break;
    case Route::COUNT: throw std::runtime_error("launch_render: no route");
    }
    if (rl.kernel_stream) {
        if (hipEventRecord(rl.kernel_done, ks) != hipSuccess || hipStreamWaitEvent(stream, rl.kernel_done, 0) != hipSuccess)
            throw std::runtime_error("launch_render: joining the render stream failed");
    }
    if (is_persistent(r) && !is_path(r)) launch_reduce_partials(sv, a, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw std::runtime_error(std::string("render kernel launch failed: ") + hipGetErrorString(e));
}

unsigned persistent_blocks(const RenderLaunch &rl, long long num_items) {
    long long waves_needed = (num_items + 63) / 64;
    long long blocks = resident_lanes(rl) / gd::kBlock;                 // 2 resident blocks per CU by default (LDS-bound)
    if (blocks > (waves_needed + 3) / 4) blocks = (waves_needed + 3) / 4;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// Work items per pixel. A lane processes an item's samples one after the other, so when the queue runs dry the kernel
// still needs as long as its longest unfinished item: with equal chunks of 4+ samples that drain was 0.44 ms of a 2.5 ms
// launch on cbox 512x512x16 (tests/prof_drain.py; bounding the path length barely changed it, so it is the ITEM, not the
// longest path). Chunks therefore shrink along the queue — each takes about 55 % of the samples still unassigned, the
// last ones are single samples — and the queue hands out chunk 0 of every pixel, then chunk 1, ...: long items start
// early, the tail of the launch consists of one-sample items. The rule is applied per ROUND of items, not per chunk (below):
// 16 spp on a 512^2 film -> 5,5,2,2,1,1 (8,5,2,1 until round 3); 64 -> 18,18,8,8,3,3,2,2,1,1; a 64-row band of that film at 128 spp
// -> 8 x 8, 5 x 8, 2 x 8, 1 x 8. Small bands with many samples (multi-GPU row bands) cap the chunk size so that every resident lane
// still sees several items. One 128-byte partial record per item; gdpt_reduce_partials merges a pixel's records in chunk order,
// so the result depends neither on which lane ran what nor on when.
ChunkPlan make_chunk_plan(int spp, int force_log2k, long long pixels, long long lanes, int take_pct_arg) {
    ChunkPlan p{};
    if (spp < 1) spp = 1;
    if (force_log2k >= 0) {                                    // tests: 2^k equal chunks
        int k = force_log2k;
        while (k > 0 && ((1 << k) > spp || (1 << k) > kMaxChunks)) k--;
        p.n = 1 << k;
        for (int c = 0; c <= p.n; c++) p.begin[c] = (int)(((long long)c * spp) >> k);
        return p;
    }
    {   // test knob plan_digits: the chunk sizes spelled out as decimal digits (552211 = 5,5,2,2,1,1), used if they add up to spp
        long long digits = (long long)gdpt::debug_knob("plan_digits", 0.0);
        int sz[18], m = 0, sum = 0;
        for (; digits > 0 && m < 18; digits /= 10) { sz[m] = (int)(digits % 10); sum += sz[m]; if (sz[m] == 0) sum = -1000000; m++; }
        if (m > 0 && sum == spp) {
            p.n = m; p.begin[0] = 0;
            for (int c = 0; c < m; c++) p.begin[c + 1] = p.begin[c] + sz[m - 1 - c];
            return p;
        }
    }
    // at least ~4 items per resident lane, as far as the sample count allows
    long long cap = (long long)spp * pixels / (lanes > 0 ? lanes * 4 : 1);
    if (cap < 1) cap = 1;
    // The queue is chunk-major, so one ROUND of items — one per resident lane — spans lanes / pixels chunks. What is in flight when the
    // queue runs dry is the last round and the stragglers of the ones before it, so the sizes have to fall off per ROUND, not per
    // chunk: a 64-row band of the 512x512 film at 128 spp (pixels = lanes / 4) with the tail "..., 8, 5, 2, 1" had 8-, 5-, 2- and
    // 1-sample items in its last round together — queue dry after 1.95 ms, then 1.0 ms of drain, against 0.39 ms for the whole film at
    // 16 spp (profiles/r03_prof_band.txt). The plan is therefore made for spp / q samples and every chunk of it is laid down q times,
    // q = ceil(rounds * lanes / pixels): every size of the shrinking tail then lasts `rounds` rounds. rounds = 4 (measured: the band
    // above 2.67 -> 2.23 ms, the speed of the whole film; the 512x512 film itself, q = 2: 16 spp -> 5,5,2,2,1,1 instead of 8,5,2,1,
    // +1.3 % at 16 spp and +3 % at 256 spp, profiles/r03_ab_plan_rounds.txt; 6 and 8 rounds no better).
    long long rounds = gdpt::debug_knob_int("plan_rounds", 4);
    rounds = rounds <= 0 ? 4 : std::min(8LL, rounds);                                                    // (test knob; 0 = the default)
    long long q = (pixels > 0 && rounds * lanes > pixels) ? (rounds * lanes + pixels - 1) / pixels : 1;
    if (q > 8) q = 8;
    if ((long long)spp <= q) q = 1;                             // (nothing to shape: the rule below makes single samples)
    const long long slots = kMaxChunks / q;                     // chunks the virtual plan may have (q = 1: kMaxChunks)
    const long long head = q > 1 ? (slots > 4 ? slots - 4 : 1) : kMaxChunks - 8;      // of which for cap-sized chunks (the rest: the shrinking tail)
    const int v = (int)(((long long)spp + q - 1) / q);          // samples of the virtual plan; q * v - spp < q are taken back below
    if ((long long)v > cap * head) cap = ((long long)v + head - 1) / head;             // never more than kMaxChunks chunks
    // share of the unassigned samples a chunk takes, in percent: 55, or what the caller asks for (capi_device.hip: 40 for scenes whose
    // paths are long-tailed — DisneyGlass: an item's time varies more, smaller items balance it, +9..15 %, profiles/r03_sweep_plan_twosided.txt)
    long long take_pct = gdpt::debug_knob_int("plan_shrink", 0);                                         // (test knob; 0 = no override)
    if (take_pct <= 0) take_pct = take_pct_arg > 0 ? take_pct_arg : 55;
    take_pct = std::min(90LL, std::max(10LL, take_pct));
    int sizes[kMaxChunks];
    int rem = v, m = 0;
    while (rem > 0) {
        long long sz = ((long long)rem * take_pct + 99) / 100; // ceil(0.55 * rem)
        if (rem <= 2) sz = 1;                                  // the tail of the queue: single samples
        if (sz > cap) sz = cap;
        if (sz < 1) sz = 1;
        if (m == (int)slots - 1) sz = rem;
        rem -= (int)sz;
        sizes[m++] = (int)sz;
    }
    int excess = (int)(q * v - spp);                            // < q <= 8 samples too many: the last copies of the smallest size above 1 give
    int shrink = -1;                                            // one back each (the sizes stay in descending order); all single: chunks dropped
    for (int c = 0; c < m; c++) if (sizes[c] > 1) shrink = c;
    int n = 0;
    p.begin[0] = 0;
    for (int c = 0; c < m; c++)
        for (int r = 0; r < (int)q; r++) {
            int sz = sizes[c];
            if (c == shrink && r >= (int)q - excess) sz--;
            p.begin[n + 1] = p.begin[n] + sz;
            n++;
        }
    if (shrink < 0) n -= excess;                                // (every chunk a single sample: q * v - spp of them too many)
    p.n = n;
    return p;
}

bool scene_fits_lds(int num_nodes, int num_prims, int num_tris, int num_materials, int num_lights, int bvh_depth) {
    size_t bytes = (size_t)num_nodes * sizeof(DevBvhNode) + (size_t)num_prims * sizeof(DevPrim) +
                   (size_t)num_tris * sizeof(DevTriShade) + (size_t)num_materials * sizeof(GdptMaterial) + 8 + (size_t)num_lights * 24;
    return bytes <= (size_t)gd::kLdsSceneBytes && bvh_depth <= gd::kLdsSceneLevels && num_nodes > 0;
}

bool scene_fits_lds_wide(int num_nodes4, int num_prims, int num_tris, int num_materials, int num_lights, int wide_stack_need) {
    size_t bytes = (size_t)num_nodes4 * sizeof(DevBvh4Node) + (size_t)num_prims * sizeof(DevPrim) +
                   (size_t)num_tris * sizeof(DevTriShade) + (size_t)num_materials * sizeof(GdptMaterial) + 8 + (size_t)num_lights * 24;
    return bytes <= (size_t)gd::kLdsSceneBytes && wide_stack_need <= gd::kLdsSceneLevels && num_nodes4 > 0;
}

} // namespace gdpt
