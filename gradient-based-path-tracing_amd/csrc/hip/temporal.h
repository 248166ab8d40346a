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

} // namespace gdpt
