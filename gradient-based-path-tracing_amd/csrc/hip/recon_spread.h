// recon_spread.h — the spread of N weighted images of one film (recon_spread.hip): the weighted variance of their mean per
// component, its film sums, and the per-pixel error map (include/gdpt.h: gdpt_recon_spread*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

namespace gdpt {

struct ReconSpreadResult {
    double sum_var = 0, sum_sq = 0;   // over the pixels kept: sum of var, sum of the total's squares
    double left_out = 0;              // pixels left out of both sums
    double ms = 0;                    // device time of the launches, HIP events
};

// Device pointers on the current device, W*H*3 doubles each (d_map: W*H). weights[i] > 0; 2 <= n <= GDPT_MULTI_MAX_DEVICES;
// 0 <= radius <= 8; d_total == nullptr: the weighted mean takes its place; d_var, d_map nullable. The arguments are the caller's to
// check (gdpt_recon_spread_device does). Enqueued on `stream`, and waits for it (the sums come back to the host). Scratch is kept
// per (device, stream), and dropped by forget_stream (device_mem.h); the same call gives the same bits.
ReconSpreadResult recon_spread_device(int w, int h, int n, const double *const *d_images, const double *weights, const double *d_total,
                                      int radius, double *d_var, double *d_map, hipStream_t stream);

// Launch geometry (image_kernels.h). spread_kernel: film::stride_grid(W H, film::kMaxBlocks, 1), as the fold it mirrors; box_kernel:
// film::tile_grid over tiles of kSpreadTileW x kSpreadTileH pixels.
constexpr int kSpreadTileW = 32, kSpreadTileH = 8;

// members, radius, the sums, error_estimate = sqrt(sum_var / sum_sq), the count and the device time into *st (nullable)
void fill_spread_stats(GdptReconSpreadStats *st, int n, int radius, const ReconSpreadResult &r);

} // namespace gdpt
