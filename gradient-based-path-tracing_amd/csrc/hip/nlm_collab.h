// nlm_collab.h — the collaborative form of the first-order feature regression (nlm_collab.hip; include/gdpt.h:
// gdpt_denoise_nlm_collab*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

namespace gdpt {

// The collaborative regression on device pointers of the current device, every argument checked (the session's entry point): the fit
// into the coefficient film, then the gather into d_out. d_coef: 3 (1 + num_regressors) planes of w h doubles, or null for the film the
// library keeps per (device, stream), grown on demand and dropped by forget_stream (device_mem.h) with the rest of the scratch.
// Enqueued on `stream`; waits for it if `stats` is asked for. Launch geometry: film::tile_grid over tiles of kNlmTile x kNlmTile pixels.
void denoise_nlm_collab_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               const GdptNlmParams &p, const GdptNlmGuide &g, const GdptNlmRegress &rg, double *d_out, double *d_coef,
                               hipStream_t stream, GdptNlmStats *stats);

} // namespace gdpt
