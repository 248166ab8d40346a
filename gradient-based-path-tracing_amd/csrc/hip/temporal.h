// temporal.h — temporal reprojection of an accumulated mean and its variance across a camera move (temporal.hip; include/gdpt.h:
// gdpt_temporal_*, where the definition stands).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void temporal_check_params(const std::string &who, const GdptTemporalParams &p);

// M(camera) of the definition, row-major; throws, naming the field, for a non-finite entry or a singular matrix. Host only.
void temporal_world_to_sample(const std::string &who, const GdptCamera &cam, double M[16]);

// One push on device pointers of the handle's device, every argument checked: one kernel on the handle's stream under the 16 x 16
// "nlm" grid rule (film::tile_grid over kNlmTile tiles, denoise_nlm.h); waits for the stream only if `stats` is asked for.
void temporal_push_launch(GdptTemporal *t, const GdptCamera &cam, const double *d_img, const double *d_var, const double *d_feat,
                          const GdptTemporalParams &p, double *d_out, double *d_var_out, double *d_len, GdptTemporalStats *stats);

// The gradient block's refusals (j_max, cos_min, reserved), as temporal_check_params. Host only.
void temporal_check_grad_params(const std::string &who, const GdptTemporalGradParams &p);

// The frame's assembled gradients with their variances, and where the accumulated ones go (gdpt_temporal_push_gradients_device).
struct TemporalGradIO {
    const double *gx, *gx_var, *gy, *gy_var;
    double *gx_out, *gx_var_out, *gy_out, *gy_var_out, *glen;      // glen nullable
};

// temporal_push_launch with the gradients carried along: the gradient kernel in place of the plain one, the same grid, the same
// stream; the gradient history is allocated by the first call.
void temporal_push_gradients_launch(GdptTemporal *t, const GdptCamera &cam, const double *d_img, const double *d_var, const double *d_feat,
                                    const TemporalGradIO &io, const GdptTemporalParams &p, const GdptTemporalGradParams &gp, double *d_out,
                                    double *d_var_out, double *d_len, GdptTemporalGradStats *stats);

} // namespace gdpt
