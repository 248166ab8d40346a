// variance_smooth.h — the box mean of the variance of a mean over the valid pixels of a window, in the albedo-normalised domain when a
// demod block is given (variance_smooth.hip; include/gdpt.h: gdpt_variance_smooth*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void var_smooth_check_params(const std::string &who, const GdptVarSmoothParams &p);

// The smoothing on device pointers of the current device, every argument checked (the session's entry point); `demod` nullable: a~ = 1,
// and d_feat, d_feat_var are not read. Enqueued on `stream`; waits for it if `stats` is asked for. Launch geometry: film::tile_grid
// (image_kernels.h) over tiles of kVarSmoothTile x kVarSmoothTile pixels. Scratch is kept per (device, stream), and dropped by
// forget_stream (device_mem.h).
void variance_smooth_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                            const GdptVarSmoothParams &p, const GdptNlmDemod *demod, double *d_var_out, hipStream_t stream,
                            GdptVarSmoothStats *stats);

constexpr int kVarSmoothTile = 16;

} // namespace gdpt
