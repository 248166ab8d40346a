// scene_internal.h — the device-resident scene handle and the render entry shared by the C-ABI translation units
// (capi_device.hip: single-device entry points; multi_gpu.hip: the row-band host of several devices).
#pragma once
#include "../../../include/gdpt.h"
#include "../device_scene.h"
#include "../host/scene_prepare.h"
#include "device_mem.h"
#include "render_kernels.h"

#include <hip/hip_runtime.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

// What one launch of a persistent render kernel owns while it is in flight. A handle has two (GdptScene::scratch): consecutive
// overlapped launches alternate between them, so frame k + 1's kernel can run while frame k's partials wait to be reduced.
struct GdptLaunchScratch {
    gdpt::DeviceBuffer<double> partials;              // work-item partial sums of the persistent render kernel
    gdpt::DeviceBuffer<unsigned long long> queue;     // work-queue head
    gdpt::DeviceBuffer<gdpt::RenderCounters> counters;
    gdpt::Event rendered;    // behind the render kernel, on the set's render stream
    gdpt::Event released;    // behind the last reader or writer of the set on a caller's stream (gdpt_reduce_partials; an in-stream launch)
    bool used = false;       // `released` has been recorded
};

struct GdptScene {
    int device = 0;
    DevSceneView view{};
    gdpt::SceneTraits traits;      // what chooses a render's route (host/scene_prepare.h), read by begin_launch
    int scene_spp = 0;             // <sampler sampleCount> of the description (default spp)
    std::vector<gdpt::DeviceBuffer<unsigned char>> allocations;   // the uploaded scene tables `view` points into
    // cached output/work buffers for the host-pointer entry points
    gdpt::DeviceBuffer<double> d_buf[9];
    gdpt::RenderCounters *d_counters = nullptr;       // the counters block of the last launch (scratch[k].counters)
    gdpt::PinnedBuffer<gdpt::RenderCounters> h_counters;
    gdpt::DeviceBuffer<unsigned char> d_bounce_log;   // per-lane bounce log of the two-sided lane machine
    // Launch scratch and render streams (capi_device.hip: begin_launch). An in-stream launch runs wholly on the caller's stream with
    // scratch[0]. An overlapped launch k runs its queue reset and render kernel on render_stream[k % 2] with scratch[k % 2]; only
    // gdpt_reduce_partials, which writes the images, stays on the caller's stream. scratch[1] is allocated by the second such launch.
    GdptLaunchScratch scratch[2];
    gdpt::Stream render_stream[2];
    gdpt::Event ev_entry[2];              // recorded on the caller's stream at the start of every launch call, alternating
    unsigned long long calls = 0;         // launch calls so far
    unsigned long long overlapped = 0;    // overlapped launches so far
    bool in_flight = false;               // a render stream may hold work the host has not waited for
    bool need_fence = true;               // the next overlapped launch makes both render streams wait for the caller's stream as it is at that call
    bool have_caller = false;
    hipStream_t last_caller = nullptr;    // the caller's stream of the last launch
    // wavefront pipeline (render_wavefront.h): path state, live list (one entry per slot), generation counters
    gdpt::DeviceBuffer<unsigned long long> d_wf_state;
    gdpt::DeviceBuffer<unsigned> d_wf_live, d_wf_counters;
    gdpt::PinnedBuffer<unsigned> h_wf_word;
    gdpt::DeviceBuffer<unsigned char> d_wf_aux;       // ray / hit records, sort keys and histogram, overflow stacks (render_kernels.hip: wf_aux_layout)
    gdpt::Event wf_event;
    int num_cus = 256;
    gdpt::Event ev0, ev1;

    void ensure_buffers(size_t elems) {
        for (auto &b : d_buf) b.grow(elems, "hipMalloc(image buffers)");
    }
    // Waits on the host for everything the render streams hold. (What a caller's stream still holds is that caller's, as before.)
    // No render of this handle is resident behind it: the solver's hint (render_kernels.h) goes with the wait.
    void join() {
        gdpt::clear_render_beside_hint(device, this);
        if (!in_flight) return;
        for (auto &st : render_stream) if (st) gdpt::ck(hipStreamSynchronize(st), "hipStreamSynchronize(render stream)");
        in_flight = false;
    }
    ~GdptScene() {                              // the members free themselves on the device: streams join and go before the buffers
        hipSetDevice(device);
        gdpt::clear_render_beside_hint(device, this);
        for (auto &st : render_stream) st.reset();
        for (auto &ss : scratch) if (ss.used) (void)hipEventSynchronize(ss.released);      // a caller's stream may still reduce from the set
    }
};


namespace gdpt {
// A scene upload (replaces Scene::Scene, src/scene.cpp:4-53) is two steps: prepare_scene (host/scene_prepare.h) makes the tables on
// the host, upload_scene copies them to `device` and creates the handle's scratch, streams and events there.
void upload_scene(const PreparedScene &ps, int device, GdptScene *sc);
// Both steps, with the upload knobs (presplit, sbvh) resolved: what gdpt_scene_upload does.
void build_scene(const GdptSceneDesc *desc, int device, GdptScene *sc);
// One scene per entry of `devices` (a device may be named twice), each with its scene_spp set: prepared once, uploaded by one thread
// per device. The first error of any upload is rethrown after all threads have ended.
std::vector<std::unique_ptr<GdptScene>> upload_scenes(const GdptSceneDesc *desc, const int32_t *devices, int n);
// Enqueues one five-buffer render of rows [params->row_begin, row_end) on `stream`; waits only when `stats` is given.
// `window` (nullable): the samples are a window of a larger stream block (include/gdpt.h: GdptSampleWindow).
void render_device_impl(GdptScene *sc, const GdptRenderParams *params, int scene_spp,
                        double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                        hipStream_t stream, GdptRenderStats *stats, const GdptSampleWindow *window = nullptr);
// The feature render (features.hip; include/gdpt.h: gdpt_features_render_device) on a handle, after the refusals that need no handle:
// enqueues the kernel on `stream`, with no claim on the handle's launch scratch; waits only when `stats` is given.
void features_launch(GdptScene *sc, const GdptRenderParams *params, const GdptSampleWindow *window, double *d_mean, double *d_var,
                     hipStream_t stream, GdptRenderStats *stats);
} // namespace gdpt
