// render_kernels.h — launch interface of the GDPT render kernels (host side of render_kernels.hip).
#pragma once
#include "../device_scene.h"
#include <hip/hip_runtime.h>

namespace gdpt {

// A pixel's samples are cut into work items ("chunks"): chunk c covers samples [begin[c], begin[c+1]).
constexpr int kMaxChunks = 64;
struct ChunkPlan { int n; int begin[kMaxChunks + 1]; };

struct RenderCounters {            // device-resident, zeroed per render
    unsigned long long rays, bounces, nonfinite, nodes, prims;
    unsigned long long wave_node_trips, wave_leaf_trips, wave_steps, lane_steps;   // counting builds: SIMT utilisation
    unsigned long long stamps[16];  // diagnostic build (knob "stamps"): wave cycles per segment, render_device.h SEG_*
};

// The kernel a render launches, one per name of include/gdpt_debug.h (route_name gives it), grouped as listed there:
// GradPath lane machines that pull work items (.. WAVEFRONT_GENERAL), GradPath straight loops (EAGER .. RECONNECT_GENERAL),
// Integrator::Path (PATH_TILE ..).
enum class Route : int {
    LAMBERT_PLAIN_LDS_CONST, LAMBERT_PLAIN_LDS_TEX, LAMBERT_PLAIN_HBM_CONST, LAMBERT_PLAIN_HBM_TEX,
    LAMBERT_LDS_WIDE, LAMBERT_LDS_BVH2, LAMBERT_HBM,
    LAMBERT_STAMPED_LDS_PLAIN, LAMBERT_STAMPED_LDS, LAMBERT_STAMPED_HBM,
    GENERAL_SET_A_DISNEY_DIFFUSE, GENERAL_SET_A_DISNEY_METAL, GENERAL_SET_B_DISNEY_CLEARCOAT, GENERAL_SET_B_DISNEY_SHEEN,
    GENERAL_LDS_WIDE, GENERAL_LDS_BVH2, GENERAL_HBM,
    TWOSIDED_LDS, TWOSIDED_HBM, TWOSIDED_HBM_GLASS,
    WAVEFRONT_LAMBERT, WAVEFRONT_GENERAL,
    EAGER, TILE_EAGER, TILE_PHASES_LAMBERT, TILE_PHASES_GENERAL,
    RECONNECT_LDS_LAMBERT, RECONNECT_HBM_LAMBERT, RECONNECT_GENERAL,
    PATH_TILE, PATH_EAGER,
    PATH_PERSISTENT_LDS_LAMBERT_PLAIN, PATH_PERSISTENT_LDS_LAMBERT, PATH_PERSISTENT_LDS_LAMBERT_ENV,
    PATH_PERSISTENT_HBM_LAMBERT, PATH_PERSISTENT_HBM_LAMBERT_ENV,
    PATH_PERSISTENT_LDS_GENERAL, PATH_PERSISTENT_LDS_GENERAL_ENV, PATH_PERSISTENT_HBM_GENERAL, PATH_PERSISTENT_HBM_GENERAL_ENV,
    COUNT
};
const char *route_name(Route r);
inline bool is_path(Route r) { return r >= Route::PATH_TILE; }
// pulls (pixel, chunk) work items from the queue into `partials` (GradPath: merged by gdpt_reduce_partials)
inline bool is_persistent(Route r) { return r <= Route::WAVEFRONT_GENERAL || r >= Route::PATH_PERSISTENT_LDS_LAMBERT_PLAIN; }
inline bool is_wavefront(Route r) { return r == Route::WAVEFRONT_LAMBERT || r == Route::WAVEFRONT_GENERAL; }
inline bool needs_bounce_log(Route r) { return r >= Route::TWOSIDED_LDS && r <= Route::TWOSIDED_HBM_GLASS; }
inline bool is_stamped(Route r) { return r >= Route::LAMBERT_STAMPED_LDS_PLAIN && r <= Route::LAMBERT_STAMPED_HBM; }
// the one-sided lane machine (gdpt_render_phases) in its product builds: its launch touches nothing but the scene, its partials,
// queue head and counters, so it may run beside the previous frame's tail (capi_device.hip: begin_launch)
inline bool can_overlap(Route r) { return r <= Route::GENERAL_HBM && !is_stamped(r); }
// gdpt_render_phases on an LDS-resident scene (the stamped builds included): the launch sizes its scene copy and stack from the scene
// (../lds_layout.h)
inline bool phases_lds_scene(Route r) {
    return r == Route::LAMBERT_PLAIN_LDS_CONST || r == Route::LAMBERT_PLAIN_LDS_TEX || r == Route::LAMBERT_LDS_WIDE || r == Route::LAMBERT_LDS_BVH2 ||
           r == Route::LAMBERT_STAMPED_LDS_PLAIN || r == Route::LAMBERT_STAMPED_LDS || r == Route::GENERAL_LDS_WIDE || r == Route::GENERAL_LDS_BVH2;
}
// the gdpt_render_phases builds with the batched sample set-up and its per-wave table in static LDS (render_device.h: SETUP): the plain
// Lambertian kernel for an LDS-resident scene with constant textures and its stamped twin; RenderLaunch::no_setup_batch selects their
// twins without
inline bool has_setup_batch(Route r) { return r == Route::LAMBERT_PLAIN_LDS_CONST || r == Route::LAMBERT_STAMPED_LDS_PLAIN; }
// the only kernels that walk the LDS copy in its BVH2 form; every other route walks a BVH4 (or the HBM tree)
inline bool walks_bvh2(Route r) { return r == Route::LAMBERT_LDS_BVH2 || r == Route::GENERAL_LDS_BVH2; }

// Everything the route depends on. The caller resolves the knobs (include/gdpt_debug.h) into the overrides.
struct RouteInputs {
    bool path;                     // Integrator::Path (else GradPath)
    int rng_scheme, shift_mode;    // GDPT_RNG_*, GDPT_SHIFT_*
    int max_depth, rr_depth;       // effective maxDepth, the scene's rrDepth (twosided_log_covers)
    // scene traits
    bool one_sided;                // no DisneyGlass / DisneyBSDF / RoughDielectric
    bool has_rough;                // RoughPlastic / RoughDielectric
    bool lambert_only;             // every material is Lambertian
    unsigned material_mask;        // bit t = some material of the scene has type t (selects kernels built for small sets)
    bool has_spheres, const_textures, has_envmap;
    bool fits_lds;                 // scene_fits_lds: the BVH2 form + primitive records fit the block's LDS copy
    bool fits_lds_wide;            // scene_fits_lds_wide: the same for the BVH4 form
    // knob overrides (defaults: the product path)
    bool force_eager, no_lds_scene, lds_wide, no_twosided_machine, wavefront, stamps, no_plain_kernel, full_material_switch;
    // knob whole_leaf_trips: picks no other route — the LDS-resident one-sided lane machines run their LEAF_K = 0 instantiation (a leaf
    // trip tests the whole leaf) under the route name they always have; launch_render takes it from RenderLaunch::whole_leaf_trips
    bool whole_leaf_trips;
    // knob no_setup_batch: picks no other route either — the has_setup_batch routes run their instantiation with lane_camera in the step
    // (RenderLaunch::no_setup_batch)
    bool no_setup_batch;
};
// Pure: no HIP call, no knob read. Throws std::runtime_error for an rng_scheme / shift_mode pair no kernel serves.
Route choose_route(const RouteInputs &in);

struct RenderLaunch {
    Route route;                   // choose_route
    int spp;
    int stream_spp, first_sample;  // sample window (GdptSampleWindow); a plain render has stream_spp = spp, first_sample = 0
    int row_begin, row_end;
    int max_depth;                 // effective (scene value or override)
    double *img, *cx0, *cy0, *cx1, *cy1;   // device, W*H*3 each (Path: img only)
    RenderCounters *counters;      // device
    bool count_traversal;          // counting build: BVH nodes / primitives per ray
    ChunkPlan plan;                // persistent routes: the work-item plan (make_chunk_plan)
    int thresh_a, thresh_c;        // trace-phase exit fractions /256 (unfinished rays; lanes still searching a leaf), -1 = default
    int force_log2k;               // lanes per pixel = 2^force_log2k (-1 = automatic)
    int wide_stack_need;           // traversal-stack bound of the tree the HBM kernels walk (host-verified)
    int lds_stack_need;            // phases_lds_scene routes: the same bound of the tree the LDS copy holds (BVH4: wide_stack_need, BVH2: its depth)
    bool lds_fixed_layout;         // knob lds_fixed_layout: the caps (kLdsSceneLevels, kLdsSceneBytes) instead of what the scene needs
    void *bounce_log;              // two-sided routes: per-lane log (device), sized by twosided_log_bytes(blocks)
    size_t bounce_log_bytes;
    int num_cus;                   // compute units of the device (persistent grid size)
    int blocks_per_cu;             // persistent blocks per CU (0 = default 2)
    // wavefront pipeline (render_wavefront.h)
    unsigned long long *wf_state;  // device, wf_words() * wf_slots 8-byte words
    unsigned *wf_live;             // device, wf_slots
    void *wf_aux;                  // device, wf_aux_bytes(wf_slots): ray / hit records, sort keys, histogram, overflow stacks
    int wf_sort;                   // 0 = queue in slot order, 1 = sorted (octant, origin cell), 2 = sorted (origin cell, octant)
    float wf_bounds[6];            // scene bounds (min xyz, max xyz) for the origin cells of the sort key
    unsigned *wf_counters;         // device, 3 * wf_max_generations()
    unsigned *wf_host;             // pinned, 1 word (live-count read-back)
    hipEvent_t wf_event;
    int wf_slots;
    int replay_per_step;           // two-sided lane machine (render_twosided.h), 0 = default
    bool whole_leaf_trips;         // RouteInputs::whole_leaf_trips
    bool no_setup_batch;           // RouteInputs::no_setup_batch
    double *partials;              // device, >= 16 doubles per work item (partial sums)
    unsigned long long *queue_head;// device, work-queue head
    // overlapped launch (can_overlap routes only; nullptr = everything on the caller's stream): the queue reset and the render kernel
    // go on kernel_stream, kernel_done is recorded behind them and the caller's stream waits for it before gdpt_reduce_partials
    hipStream_t kernel_stream;
    hipEvent_t kernel_done;
    // an overlapped launch whose counters and queue head were zeroed on kernel_stream when its scratch set was claimed, ahead of the
    // stream's wait for the previous call (capi_device.hip: claim_scratch): launch_render then enqueues no reset of its own
    bool resets_enqueued;
};
bool scene_fits_lds(int num_nodes, int num_prims, int num_tris, int num_materials, int num_lights, int bvh_depth);
bool scene_fits_lds_wide(int num_nodes4, int num_prims, int num_tris, int num_materials, int num_lights, int wide_stack_need);

// Lanes of the persistent grid resident at once (blocks_per_cu 0 = 2 blocks per CU).
inline long long resident_lanes(const RenderLaunch &rl) { return (long long)rl.num_cus * (rl.blocks_per_cu > 0 ? rl.blocks_per_cu : 2) * 256; }
// Pixel slots of a band: 16x16-pixel tiles of 256 slots (ragged edge tiles keep all 256). Work items = slots * plan.n.
inline long long band_slots(int width, int rows) { return (long long)((width + 15) / 16) * ((rows + 15) / 16) * 256; }
size_t twosided_log_bytes(unsigned blocks);
unsigned persistent_blocks(const RenderLaunch &rl, long long num_items);
// Chunk sizes shrink along the queue (about 40 % of what is left each time, ending in single samples) unless
// force_log2k >= 0 asks for 2^k equal chunks (tests). `lanes` = resident lanes of the persistent grid.
ChunkPlan make_chunk_plan(int spp, int force_log2k, long long pixels, long long lanes, int take_pct = 0);    // take_pct: share of the unassigned samples a chunk takes (0 = the default 55)

int wf_words();
int wf_max_generations();
// Path slots of the wavefront pipeline for a band of `num_items` work items.
int wf_slot_count(long long num_items);
size_t wf_aux_bytes(int slots);
// Enqueues the render of rl.route on `stream` and records the route (last_route). Throws std::runtime_error on a launch failure.
void launch_render(const DevSceneView &sv, const RenderLaunch &rl, hipStream_t stream);

// LDS a CU has left beside the resident blocks of this launch, allocation granule counted; 0 for every route but phases_lds_scene.
int render_free_lds_per_cu(const DevSceneView &sv, const RenderLaunch &rl);
// Per-device hint for the solver (poisson_kernels.hip), owned by the render launcher: > 0 while a lane machine on an LDS-resident scene
// may be resident on the device's CUs on a render stream — the value is render_free_lds_per_cu of the last such launch. `owner` is the
// handle that set it; only its owner clears it (an in-stream launch, GdptScene::join, destruction of the handle). It follows the call
// sequence, not the clock: nothing asks the device.
void set_render_beside_hint(int device, const void *owner, int free_lds_per_cu);
void clear_render_beside_hint(int device, const void *owner);
int render_beside_hint(int device);

// Route of the calling thread's last render launch (include/gdpt_debug.h: gdpt_debug_last_route): launch_render sets it,
// reset_route clears it ("") at the start of a render.
void set_route(Route r);
void reset_route();
const char *last_route();
int route_names(const char **out, int capacity);
// The two-sided replay machine logs gd::kLogCap bounce iterations per sample (render_twosided.h); false when the depth
// bound lets a path run past the log, where the replay would stop following the reference.
bool twosided_log_covers(int max_depth, int rr_depth);

} // namespace gdpt
