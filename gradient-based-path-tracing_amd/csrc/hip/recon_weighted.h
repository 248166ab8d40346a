// recon_weighted.h — launch interface of the variance-weighted reconstruction (host side of recon_weighted.hip).
#pragma once
#include "recon_l1.h"

namespace gdpt {

struct ReconWeightedResult {
    ReconL1Result recon;                 // energies are sums of kappa |r|_2
    double scale_data, scale_grad;       // geometric means of the row variances: data rows / x- and y-edge rows together
    unsigned long long rows_dropped, pixels_isolated;
};

// Variance-weighted reconstruction (include/gdpt.h: gdpt_reconstruct_weighted) on device buffers: c, gx, gy and their variance
// planes, W*H*3 doubles each, interleaved RGB. p.irls_iters == 0: weighted least squares (one solve); > 0: weighted IRLS.
// d_conf (nullable, any entry nullable): receives the confidences of the data, x-edge and y-edge rows, W*H doubles each.
// d_out must not alias an input. Synchronises `stream` as recon_l1_device does, and uses the same per-(device, stream) scratch.
ReconWeightedResult recon_weighted_device(int w, int h, const double *d_c, const double *d_gx, const double *d_gy, const double *d_vc,
                                          const double *d_vgx, const double *d_vgy, double alpha, const ReconL1Params &p, double conf_floor,
                                          double *d_out, double *const d_conf[3], hipStream_t stream);

} // namespace gdpt
