// denoise_nlm.h — non-local means on a mean and the variance of that mean (denoise_nlm.hip; include/gdpt.h: gdpt_denoise_nlm*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void nlm_check_params(const std::string &who, const GdptNlmParams &p);

// Launch geometry of both kernel forms (gdpt_debug_image_grid reads it too): 16 x 16 tiles and the blocks that stride over them.
struct NlmGrid { int tiles_x, tiles, blocks; };
NlmGrid nlm_grid(int w, int h);

// Drops the (device, stream) pair's scratch; forget_stream (device_mem.h) calls it.
void denoise_nlm_forget_stream(int dev, hipStream_t stream);

} // namespace gdpt
