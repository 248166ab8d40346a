// nlm_regress.h — a first-order feature regression on the non-local-means weights (nlm_regress.hip; include/gdpt.h:
// gdpt_denoise_nlm_regress*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a regression block beside a guide of `num_channels` planes; the message names the field. `who`
// names the caller. Host only.
void nlm_check_regress(const std::string &who, const GdptNlmRegress &r, int num_channels);

// The regression on device pointers of the current device, every argument checked (the session's entry point). Enqueued on `stream`;
// waits for it if `stats` is asked for. Launch geometry: film::tile_grid over tiles of kNlmTile x kNlmTile pixels (denoise_nlm.h);
// the scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
void denoise_nlm_regress_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                const GdptNlmParams &p, const GdptNlmGuide &g, const GdptNlmRegress &rg, double *d_out, double *d_var_out,
                                hipStream_t stream, GdptNlmStats *stats);

} // namespace gdpt
