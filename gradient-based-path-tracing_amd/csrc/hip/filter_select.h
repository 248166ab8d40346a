// filter_select.h — the per-pixel choice among candidate filters by the two-half error estimate (filter_select.hip; include/gdpt.h:
// gdpt_filter_select*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void select_check_params(const std::string &who, const GdptSelectParams &p);

// The selection on device pointers of the current device, every argument checked. d_sel, d_mse, d_E nullable. Enqueued on `stream`;
// waits for it if `stats` is asked for. Launch geometry: film::tile_grid (image_kernels.h) over tiles of kSelectTile x kSelectTile
// pixels. Scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
void filter_select_launch(int w, int h, int n, const double *const *d_FA, const double *const *d_FB, const double *const *d_T,
                          const double *d_uA, const double *d_vA, const double *d_uB, const double *d_vB, const GdptSelectParams &p,
                          double *d_out, int32_t *d_sel, double *d_mse, double *d_E, hipStream_t stream, GdptSelectStats *stats);

constexpr int kSelectTile = 16;

} // namespace gdpt
