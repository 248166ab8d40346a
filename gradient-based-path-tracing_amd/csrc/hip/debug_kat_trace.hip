// debug_kat_trace.hip — test instrument (include/gdpt_debug.h: gdpt_debug_kat_trace): the closest-hit and occlusion walks of the render
// kernels on arrays of rays, one thread per ray, so that a test can compare every hit with a brute force over the primitives. The
// kernels call the product's code as it is: setup_trace with the LDS arrays and the stack the product kernels declare, trav_init, and
// trav_run driven as trace_pending drives it (re-entered with a stop_below until no lane is pending); the two wavefront rows call
// launch_wf_trace itself on a ray queue written as the step kernel writes it. One row of the table per distinct (TraceCfg, residency)
// that a product kernel instantiates. The host admits a call only if every stack and LDS size is the product's own rule for the
// uploaded scene; everything else is refused before any launch. An any_hit query is taken by every row and re-entered like a
// closest-hit one: more than the product asks (occluded_ctx runs TraceHbm and the reconnect configuration to completion, stop_below
// = 0), and a superset of it. Nothing in lajolla, in bench.py's timed region or in the library calls this entry point.
#include "../../../include/gdpt_debug.h"
#include "../capi_common.h"
#include "render_path.h"
#include "render_twosided.h"
#include "render_wavefront.h"
#include "scene_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

using gdpt::ck;
constexpr int kTraceMaxRays = 1 << 20;

// One ray per thread in blocks of kBlock; the lanes past n start finished, as idle lanes do in the product.
template <class TC, bool LDS_SCENE>
__global__ void __launch_bounds__(gd::kBlock, 2) kat_trace_kernel(DevSceneView sv, int n, int keep_frac, int search_frac, const GdptKatTraceQuery *in, GdptKatTraceResult *out) {
    // (gdpt_render_phases) LDS-resident scenes: the fixed column of kLdsSceneLevels slots + the scene copy; scenes walked from HBM:
    // dynamic LDS = the tree's own stack bound per lane
    __shared__ int s_stack_fixed[LDS_SCENE ? gd::kLdsSceneLevels * gd::kBlock : 1];
    __shared__ __attribute__((aligned(16))) unsigned char s_scene[LDS_SCENE ? gd::kLdsSceneBytes : 16];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    int *s_stack = LDS_SCENE ? s_stack_fixed : (int *)s_dyn;
    const int tid = threadIdx.x;
    const gd::TraceCtx tx = gd::setup_trace<LDS_SCENE, TC::WIDE>(sv, s_scene, s_stack, tid, gd::kBlock, false);
    if (!LDS_SCENE) __syncthreads();
    const int i = (int)(blockIdx.x * (unsigned)gd::kBlock) + tid;
    gd::D3 org = gd::splat(0.0), dir = gd::mk(0.0, 0.0, 1.0);
    float tnear = 0.0f, tfar = __builtin_huge_valf();
    bool any_hit = false;
    gd::Trav tv;
    gd::trav_init(sv, tv, __builtin_huge_val());
    if (i < n) {
        const GdptKatTraceQuery q = in[i];
        org = gd::mk(q.org[0], q.org[1], q.org[2]); dir = gd::mk(q.dir[0], q.dir[1], q.dir[2]);
        tnear = (float)q.tnear; tfar = (float)q.tfar;           // (intersect_ctx, occluded_ctx)
        any_hit = q.any_hit != 0;
        gd::trav_init(sv, tv, q.tfar);
    } else tv.cur = gd::kTravDone;
    gd::TraceCounters tc = {0, 0, 0, 0, 0, 0};
    for (;;) {                                                  // trace_pending, until the wave has no pending ray
        const bool pending = tv.cur != gd::kTravDone;
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int stop_below = (__popcll(m) * keep_frac) >> 8;  // < popcount: every trip finishes a ray
        if (pending) gd::trav_run<TC>(sv, tx, org, dir, tnear, tfar, tv, stop_below, search_frac, tc, any_hit);
    }
    if (i < n) {
        GdptKatTraceResult r;
        r.gid = tv.best.gid < 0 ? -1 : tv.best.gid;
        r.t = tv.best.t; r.u = tv.best.u; r.v = tv.best.v;
        r.ng[0] = tv.best.ngx; r.ng[1] = tv.best.ngy; r.ng[2] = tv.best.ngz;
        out[i] = r;
    }
}

typedef void (*TraceLaunch)(const DevSceneView &, int, int, int, size_t, const GdptKatTraceQuery *, GdptKatTraceResult *, hipStream_t);
template <class TC, bool LDS_SCENE>
void launch_trace(const DevSceneView &sv, int n, int keep_frac, int search_frac, size_t dyn_lds, const GdptKatTraceQuery *in, GdptKatTraceResult *out, hipStream_t stream) {
    hipLaunchKernelGGL((kat_trace_kernel<TC, LDS_SCENE>), dim3((unsigned)((n + gd::kBlock - 1) / gd::kBlock)), dim3(gd::kBlock), LDS_SCENE ? 0 : dyn_lds, stream,
                       sv, n, keep_frac, search_frac, in, out);
}

struct TraceVariant { GdptKatTraceVariant row; TraceLaunch launch; };
template <class TC, bool LDS_SCENE>
constexpr TraceVariant trace_row(const char *name) {
    return {{name, TC::WW, TC::WIDE, TC::FLAT, TC::SPHERES, TC::SPEC, TC::LEAF_K, LDS_SCENE, 0, LDS_SCENE ? gd::kLdsSceneLevels : 0}, launch_trace<TC, LDS_SCENE>};
}
constexpr int kK = gd::kPhasesLdsLeafK;
// PhasesTraceCfg<LDS_SCENE, WIDE, WW, PLAIN, LEAF_K>: the configuration gdpt_render_phases<LAMBERT, LDS_SCENE, WIDE, WW, STAMPED, PLAIN,
// LEAF_K> walks with; the launch sites that instantiate each are named behind the row.
const TraceVariant kTraceVariants[] = {
    trace_row<gd::PhasesTraceCfg<true, true, true, 0, kK>, true>("lds_wide_cursor"),                           // render_phases_{lambert,general,diag}.hip
    trace_row<gd::PhasesTraceCfg<true, true, true, 0, 0>, true>("lds_wide_whole"),                             // ... under whole_leaf_trips; = TraceCfg<true, true, false> of render_twosided.h:351, render_reconnect.h:217, render_path.h:586
    trace_row<gd::PhasesTraceCfg<true, true, true, gd::kPlainNoSpheres, kK>, true>("lds_wide_cursor_tris"),    // render_phases_lambert_plain.hip, render_phases_diag.hip
    trace_row<gd::PhasesTraceCfg<true, true, true, gd::kPlainNoSpheres, 0>, true>("lds_wide_whole_tris"),      // ... under whole_leaf_trips; render_path.h:586 with kPlainBoth
    trace_row<gd::PhasesTraceCfg<true, false, false, 0, kK>, true>("lds_bvh2_cursor"),                         // render_phases_{lambert,general}.hip, BVH2 form
    trace_row<gd::PhasesTraceCfg<true, false, false, 0, 0>, true>("lds_bvh2_whole"),
    trace_row<gd::PhasesTraceCfg<false, true, true, 0, 0>, false>("hbm_spec"),                                 // render_phases_{lambert,general,diag}.hip, walked from HBM
    trace_row<gd::PhasesTraceCfg<false, true, true, gd::kPlainNoSpheres, 0>, false>("hbm_spec_tris"),          // render_phases_lambert_plain.hip, render_phases_general_sets.h
    trace_row<gd::TraceHbm, false>("hbm"),                                                                     // the eager kernels, render_twosided.h:351, render_reconnect.h:217, render_path.h:586 walked from HBM
    {{"wavefront_spheres", 1, 1, 1, 1, 0, 0, 0, 1, gd::kWfLdsLevels}, nullptr},                                // launch_wf_trace(t, true, ...)
    {{"wavefront_tris", 1, 1, 1, 0, 0, 0, 0, 1, gd::kWfLdsLevels}, nullptr},                                   // launch_wf_trace(t, false, ...)
};
constexpr int kNumTraceVariants = (int)(sizeof(kTraceVariants) / sizeof(kTraceVariants[0]));

// what a query must satisfy to reach a kernel; `wavefront`: the row takes closest-hit queries to infinity only
void check_query(const std::string &who, int i, const GdptKatTraceQuery &q, bool wavefront) {
    const std::string at = who + ": ray " + std::to_string(i) + ": ";
    float d[3];
    for (int k = 0; k < 3; k++) {
        d[k] = (float)q.dir[k];
        if (!std::isfinite(q.org[k]) || !std::isfinite(q.dir[k]) || !std::isfinite((float)q.org[k]) || !std::isfinite(d[k]))
            throw std::runtime_error(at + "origin or direction is not a finite fp32 number");
    }
    if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) throw std::runtime_error(at + "the direction is zero");
    if (!std::isfinite(q.tnear) || std::isnan(q.tfar) || q.tfar == -HUGE_VAL) throw std::runtime_error(at + "tnear or tfar is not a number");
    if (q.tnear < 0.0) throw std::runtime_error(at + "tnear < 0");
    if (q.tfar < q.tnear) throw std::runtime_error(at + "tfar < tnear");
    if (q.any_hit != 0 && q.any_hit != 1) throw std::runtime_error(at + "any_hit is 0 or 1");
    if (wavefront && (q.any_hit != 0 || q.tfar != HUGE_VAL)) throw std::runtime_error(at + "a wavefront row takes closest-hit queries with tfar = infinity only");
}

// the two rows that run gdpt_wf_trace: ray records as gdpt_wf_step writes them, an identity queue, the overflow stacks as
// wf_aux_layout sizes them (GDPT_BVH_MAX_DEPTH - kWfLdsLevels levels for every lane of the grid)
void run_wavefront_row(const GdptScene *scene, bool spheres, int n, int search_frac, const GdptKatTraceQuery *in, GdptKatTraceResult *out) {
    const DevSceneView &sv = scene->view;
    const unsigned blocks = (unsigned)((n + gd::kWfTraceBlock - 1) / gd::kWfTraceBlock);
    const size_t slots = (size_t)blocks * gd::kWfTraceBlock;
    std::vector<float4> rays(2 * slots, make_float4(0, 0, 0, 0)), hits(2 * slots);
    std::vector<unsigned> live(slots);
    for (size_t s = 0; s < slots; s++) live[s] = (unsigned)s;
    for (int i = 0; i < n; i++) {
        rays[2 * (size_t)i] = make_float4((float)in[i].org[0], (float)in[i].org[1], (float)in[i].org[2], (float)in[i].tnear);
        rays[2 * (size_t)i + 1] = make_float4((float)in[i].dir[0], (float)in[i].dir[1], (float)in[i].dir[2], 0.0f);
    }
    ck(hipSetDevice(scene->device), "hipSetDevice");
    const hipStream_t stream = scene->render_stream[0];
    gdpt::DeviceBuffer<float4> d_rays, d_hits;
    gdpt::DeviceBuffer<unsigned> d_live, d_count;
    gdpt::DeviceBuffer<int> d_ovf;
    static_assert(GDPT_BVH_MAX_DEPTH > gd::kWfLdsLevels, "overflow stack levels");
    const size_t ovf_ints = slots * (size_t)(GDPT_BVH_MAX_DEPTH - gd::kWfLdsLevels);
    d_rays.alloc(2 * slots, "hipMalloc(kat rays)"); d_hits.alloc(2 * slots, "hipMalloc(kat hits)");
    d_live.alloc(slots, "hipMalloc(kat queue)"); d_count.alloc(1, "hipMalloc(kat count)"); d_ovf.alloc(ovf_ints, "hipMalloc(kat overflow stacks)");
    const unsigned count = (unsigned)n;
    ck(hipMemcpyAsync(d_rays, rays.data(), rays.size() * sizeof(float4), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(kat rays)");
    ck(hipMemcpyAsync(d_live, live.data(), live.size() * sizeof(unsigned), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(kat queue)");
    ck(hipMemcpyAsync(d_count, &count, sizeof(unsigned), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(kat count)");
    ck(hipMemsetAsync(d_hits, 0, 2 * slots * sizeof(float4), stream), "hipMemsetAsync(kat hits)");
    gd::WfTrace t{};
    t.nodes4 = sv.nodes4; t.nodes4q = sv.nodes4q; t.prims = sv.prims; t.spheres = sv.spheres; t.rays = d_rays; t.hits = d_hits; t.live = d_live;
    t.count = d_count; t.ovf = d_ovf; t.ovf_stride = (unsigned)slots; t.counters = nullptr;
    t.num_tris = sv.num_tris; t.num_nodes4 = sv.num_nodes4; t.num_spheres = sv.num_spheres; t.search_frac = search_frac; t.count_stats = 0;
    gdpt::launch_wf_trace(t, spheres, blocks, stream);
    ck(hipGetLastError(), "kat wavefront trace launch");
    ck(hipMemcpyAsync(hits.data(), d_hits, hits.size() * sizeof(float4), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(kat hits)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(kat)");
    for (int i = 0; i < n; i++) {
        const float4 h = hits[2 * (size_t)i], g = hits[2 * (size_t)i + 1];
        GdptKatTraceResult r;
        unsigned bits; std::memcpy(&bits, &h.w, 4);
        r.gid = (int)bits < 0 ? -1 : (int)bits;
        r.t = h.x; r.u = h.y; r.v = h.z; r.ng[0] = g.x; r.ng[1] = g.y; r.ng[2] = g.z;
        out[i] = r;
    }
}

} // namespace

extern "C" {

int gdpt_debug_kat_trace_variants(GdptKatTraceVariant *out, int capacity) {
    int count = -1;
    const int rc = gdpt::guarded([&]() {
        if (out) {
            if (capacity < kNumTraceVariants) throw std::runtime_error("gdpt_debug_kat_trace_variants: capacity too small");
            for (int i = 0; i < kNumTraceVariants; i++) out[i] = kTraceVariants[i].row;
        }
        count = kNumTraceVariants;
    });
    return rc ? -1 : count;
}

int gdpt_debug_kat_trace(const GdptScene *scene, int variant, int n, const GdptKatTraceQuery *in, GdptKatTraceResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_trace";
        if (!scene) throw std::runtime_error(who + ": null scene handle");
        if (n < 0 || n > kTraceMaxRays) throw std::runtime_error(who + ": n must be in [0, " + std::to_string(kTraceMaxRays) + "]");
        if (n > 0 && (!in || !out)) throw std::runtime_error(who + ": null query or result array");
        if (variant < 0 || variant >= kNumTraceVariants) throw std::runtime_error(who + ": variant " + std::to_string(variant) + " is not in the table of " + std::to_string(kNumTraceVariants) + " variants");
        const TraceVariant &tv = kTraceVariants[variant];
        const GdptKatTraceVariant &row = tv.row;
        const DevSceneView &v = scene->view;
        const std::string name = std::string("variant '") + row.name + "'";
        if (row.lds_scene) {
            const bool fits = row.wide ? gdpt::scene_fits_lds_wide(v.num_nodes4, v.num_prims, v.num_tris, v.num_materials, v.num_lights, scene->traits.wide_stack_need)
                                       : gdpt::scene_fits_lds(v.num_nodes, v.num_prims, v.num_tris, v.num_materials, v.num_lights, scene->traits.bvh_depth);
            if (!fits) throw std::runtime_error(who + ": " + name + " walks the scene's copy in LDS, and this scene does not fit there");
        }
        if (!row.spheres && v.num_spheres != 0) throw std::runtime_error(who + ": " + name + " is built without sphere code, and this scene has spheres");
        // scenes walked from HBM: stack slots = the tree's own bound (launch_render)
        const int need = GDPT_HBM_BVH8 ? std::min(scene->traits.wide8_stack_need, GDPT_BVH_MAX_DEPTH) : scene->traits.wide_stack_need;
        const int stack_levels = need > 0 ? need : GDPT_BVH_MAX_DEPTH;
        if (stack_levels > GDPT_BVH_MAX_DEPTH || scene->traits.wide_stack_need > GDPT_BVH_MAX_DEPTH) throw std::runtime_error(who + ": traversal stack bound exceeds the builder's maximum");
        for (int i = 0; i < n; i++) check_query(who, i, in[i], row.wavefront != 0);
        if (n == 0) return;
        // the knobs of the render kernels, with the product's defaults (launch_render)
        const int ka = gdpt::debug_knob_int("keep_frac", -1), kc = gdpt::debug_knob_int("search_frac", -1);
        const int keep_frac = ka >= 0 ? std::min(ka, 255) : 64, search_frac = kc >= 0 ? std::min(kc, 255) : 112;
        if (row.wavefront) { run_wavefront_row(scene, row.spheres != 0, n, search_frac, in, out); return; }
        ck(hipSetDevice(scene->device), "hipSetDevice");
        const hipStream_t stream = scene->render_stream[0];
        gdpt::DeviceBuffer<GdptKatTraceQuery> d_in;
        gdpt::DeviceBuffer<GdptKatTraceResult> d_out;
        d_in.alloc((size_t)n, "hipMalloc(kat queries)");
        d_out.alloc((size_t)n, "hipMalloc(kat results)");
        ck(hipMemcpyAsync(d_in, in, (size_t)n * sizeof(GdptKatTraceQuery), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(kat queries)");
        tv.launch(v, n, keep_frac, search_frac, (size_t)stack_levels * gd::kBlock * sizeof(int), d_in, d_out, stream);
        ck(hipGetLastError(), "kat kernel launch");
        ck(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(GdptKatTraceResult), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(kat results)");
        ck(hipStreamSynchronize(stream), "hipStreamSynchronize(kat)");
    });
}

} // extern "C"
