// progressive_internal.h — the progressive session handle and the entry points shared by progressive.hip (sessions, the merge of
// sessions) and progressive_group.hip (one slice session per device, a merged total).
#pragma once
#include "image_kernels.h"
#include "scene_internal.h"

#include <algorithm>
#include <utility>
#include <vector>

struct GdptProgressive {
    GdptScene *scene = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    int mode = GDPT_PROGRESSIVE_GRADPATH, shift = GDPT_SHIFT_REFERENCE, max_depth_override = 0;
    int nbuf = 5, w = 0, h = 0;
    int block = 0;                   // size of every pixel's stream block: the stream_spp of every pass
    int first = 0, own = 0;          // the slice [first, first + own) of the block this session draws its passes from
    int own_done = 0;                // ... of which [first, first + own_done) has been drawn
    int merged = 0;                  // samples per pixel taken in by merges
    int done = 0, passes = 0;        // W and K of the statistics held: own passes and merged sessions
    int stop_reason = GDPT_STOP_NONE;
    bool group_total = false;        // the borrowed total of a GdptProgressiveGroup: the public add_pass / run / merge refuse it
    bool group_half = false;         // ... one of its two halves (group_total is set too): the refusals say so
    std::vector<std::pair<int, int>> merged_intervals;    // [begin, end) of the block, as taken in by merges
    size_t elems = 0;
    gdpt::DeviceBuffer<double> pass[5], mean[5], m2[5];
    gdpt::DeviceBuffer<double> stage[10];      // mean / M2 planes of a merge source on another device, allocated by the first such merge
    gdpt::DeviceBuffer<double> var[7];         // read-out scratch (5 buffers + assembled cx, cy), allocated by the first read
    gdpt::DeviceBuffer<double> asm_buf[4];     // c, cx, cy, reconstruction: allocated by the first reconstruct
    gdpt::DeviceBuffer<double> nlm_buf[2];     // filtered mean and its variance on their way to host memory: allocated by the first denoise
    gdpt::DeviceBuffer<double> feat_buf[2];    // feature planes and their variances of the guided denoise (8 W H doubles each): allocated by the first one
    bool feat_current = false;                 // feat_buf holds the planes the next guided denoise would render: it renders none (set and cleared by
                                               // gdpt_progressive_group_denoise_select alone, which renders once for its three sessions)
    gdpt::DeviceBuffer<double> smooth_buf;     // the smoothed variance of buffer 0 (gdpt_progressive_denoise_smoothed): allocated by the first one
    gdpt::DeviceBuffer<double> joint_buf[6];   // the jointly filtered c, cx, cy and their variances (gdpt_progressive_denoise_reconstruct): allocated by the first one
    gdpt::DeviceBuffer<double> partials;
    gdpt::DeviceBuffer<film::Estimate> d_est;
    gdpt::PinnedBuffer<film::Estimate> h_est;
    film::Estimate est{};             // of the last fold or merge (valid from 2 passes)
    gdpt::Event ev[2];               // around the fold / merge launches
    double fold_ms = 0;              // device time of the last fold (fold_kernel + finish_kernel) or merge (merge_kernel + finish_kernel)
    GdptRenderStats totals{};

    ~GdptProgressive() { hipSetDevice(device); }      // the members free themselves on it
};

namespace prg {
// What the C entry points of the same names do, without their guard against a group's total; they throw.
void add_pass(GdptProgressive &s, int spp, GdptRenderStats *stats);
void merge(GdptProgressive &dst, const GdptProgressive &src);
// Back to the state of a fresh accumulator: nothing held (the planes keep their bytes: the next merge overwrites them).
void reset(GdptProgressive &s);
double error_estimate(const GdptProgressive &s);
// What gdpt_progressive_reconstruct / _reconstruct_weighted do up to the copy-out: the image is left in s.asm_buf[3], enqueued on the
// session's stream (the weighted kinds and L1 have waited for it). They throw what the entry points report.
void reconstruct(GdptProgressive &s, double dataCost, const GdptReconParams *recon, GdptReconStats *stats);
void reconstruct_weighted(GdptProgressive &s, double dataCost, const GdptWeightedReconParams *params, double *const confidence[3],
                          GdptWeightedReconStats *stats);
void fill_status(const GdptProgressive &s, GdptProgressiveStatus *st);
} // namespace prg
