// recon_l1.h — launch interface of the robust (L1) reconstruction (host side of recon_l1.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gdpt {

struct ReconL1Params { int irls_iters, cg_max_iters; double eps_init, eps_decay, eps_floor, cg_tol; };   // resolved: no defaults left
struct ReconL1Result { int irls_rounds, cg_iters_total, cg_iters_last; double energy_first, energy_last, rel_residual_last, solve_ms; };

// L1 reconstruction by IRLS over a weighted, Jacobi-preconditioned CG (include/gdpt.h: gdpt_reconstruct) on device buffers
// (W*H*3 doubles, interleaved RGB). d_out is the iterate itself and must not alias an input. Synchronises `stream`:
// convergence of every inner solve is checked on the host, one chunk of iterations behind. Scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
ReconL1Result recon_l1_device(int w, int h, const double *d_c, const double *d_gx, const double *d_gy, double alpha,
                              const ReconL1Params &p, double *d_out, hipStream_t stream);

} // namespace gdpt
