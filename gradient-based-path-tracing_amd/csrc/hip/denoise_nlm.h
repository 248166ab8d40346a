// denoise_nlm.h — non-local means on a mean and the variance of that mean (denoise_nlm.hip; include/gdpt.h: gdpt_denoise_nlm*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void nlm_check_params(const std::string &who, const GdptNlmParams &p);

// Launch geometry of both kernel forms: film::tile_grid (image_kernels.h) over tiles of kNlmTile x kNlmTile pixels. The filter's
// scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
constexpr int kNlmTile = 16;

} // namespace gdpt
