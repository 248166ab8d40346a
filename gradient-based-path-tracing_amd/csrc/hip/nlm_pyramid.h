// nlm_pyramid.h — the multi-scale (pyramid) form of the non-local-means filters (nlm_pyramid.hip; include/gdpt.h:
// gdpt_nlm_pyramid_down*, gdpt_nlm_pyramid_up*, gdpt_denoise_nlm_multiscale*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// The kind's blocks as a multi-scale call takes them, checked: what every entry point refuses in `kind`, `guide`, `demod` and
// `num_channels` against `planes` (whether feature planes are given); the message names the field. Host only.
struct NlmKindBlocks {
    int kind = GDPT_DENOISE_PLAIN, num_channels = 0;
    bool has_guide = false, has_demod = false;
    GdptNlmGuide guide{};
    GdptNlmDemod demod{};
};
NlmKindBlocks nlm_pyramid_check_kind(const std::string &who, int kind, const GdptNlmGuide *guide, const GdptNlmDemod *demod, int num_channels,
                                     bool planes);
void nlm_pyramid_check_levels(const std::string &who, int levels);

// The multi-scale filter on device pointers of the current device, every argument checked (the session's entry point). Enqueued on
// `stream`; waits for it if `stats` is asked for. Launch geometry of both kernels: film::tile_grid (image_kernels.h) over tiles of
// kNlmPyramidTile x kNlmPyramidTile pixels, of the coarse level (down) or of the fine level (up). The pyramid, the levels' outputs and
// the scratch of the two operators are kept per (device, stream), and dropped by forget_stream (device_mem.h).
void denoise_nlm_multiscale_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const NlmKindBlocks &kb, int levels, const GdptNlmParams &p, double *d_out, double *d_var_out,
                                   hipStream_t stream, GdptNlmPyramidStats *stats);

constexpr int kNlmPyramidTile = 16;

} // namespace gdpt
