// denoise_atrous.h — the edge-avoiding a-trous wavelet filter on a mean and the variance of that mean (denoise_atrous.hip;
// include/gdpt.h: gdpt_denoise_atrous*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void atrous_check_params(const std::string &who, const GdptAtrousParams &p);

// The filter on device pointers of the current device, every argument checked (the session's entry point). `g` nullable: no feature
// term; `d` nullable: no demodulation. One kernel per level, enqueued on `stream`; waits for it if `stats` is asked for. Launch
// geometry: film::tile_grid over tiles of kNlmTile x kNlmTile pixels (denoise_nlm.h); the scratch (the sums and the planes between
// the levels) is kept per (device, stream), and dropped by forget_stream (device_mem.h).
void denoise_atrous_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                           const GdptAtrousParams &p, const GdptNlmGuide *g, const GdptNlmDemod *d, double *d_out, double *d_var_out,
                           hipStream_t stream, GdptNlmStats *stats);

} // namespace gdpt
