// recon_pcg.h — what the reconstructions built on recon_l1.hip's weighted PCG share: the tile geometry, the solver's state, the
// fixed-order reductions, the per-(device, stream) scratch and the host side of one inner solve. The PCG kernels themselves stay in
// recon_l1.hip; a translation unit that brings its own weights pass (recon_weighted.hip) fills wx, wy, diag, r and the partials as
// weights_kernel does and hands the round to recon_pcg_round.
#pragma once
#include "device_mem.h"
#include "recon_l1.h"

#include <mutex>

namespace rl1 {

constexpr int kBlock = 256, kTileW = 32, kTileH = 8, kPitch = kTileW + 2, kMaxBlocks = 1024;
static_assert(kTileW * kTileH == kBlock, "one thread per tile pixel");
constexpr int kHalo = 2 * kTileW + 2 * kTileH;       // the 5-tap needs no corners

struct State {
    double rz[2];         // <r,z> ping-pong by iteration parity
    double bb;            // <b,b>
    double tol;           // relative residual to stop at
    double rel;           // |r| / |b| of the iterate (pcg_residual_kernel)
    double energy;        // E(f) of the iterate the last weights pass read
    int iters;
    int converged;
};

struct Geo { int w, h, tiles_x, tiles; };

__device__ __forceinline__ double block_sum(double v, double *red) {
    // fixed order: xor tree inside each wave, then the wave totals in index order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < kBlock / 64; k++) s += red[k];
    return s;
}
__device__ __forceinline__ double reduce_partials(const double *part, int n, double *red) {
    double v = 0;
    for (int i = threadIdx.x; i < n; i += kBlock) v += part[i];
    return block_sum(v, red);
}
__device__ __forceinline__ double norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

} // namespace rl1

namespace gdpt {

// what the confidence pass of the variance-weighted reconstruction leaves in device memory (counts as doubles: exact below 2^53)
struct ConfStats { double scale_data, scale_grad, rows_data, rows_grad, rows_dropped, pixels_isolated; };
constexpr int kConfSlots = 6;         // block partials of the confidence pass, kMaxBlocks doubles each

struct ReconWorkspace {
    std::mutex mu;                    // held while a reconstruction runs on this (device, stream) pair
    DeviceBuffer<double> r, q, p0, p1;                                     // 3 npix each
    DeviceBuffer<double> wx, wy, diag;                                     // npix each
    DeviceBuffer<double> partials;
    DeviceBuffer<rl1::State> state;
    PinnedBuffer<rl1::State> h_state;
    Event ev[3];                                                           // timing pair + chunk marker
    // variance-weighted reconstruction only (ensure_confidence): row variances, confidences, their partials and scalars
    DeviceBuffer<double> var[3], conf[3];                                  // npix each: data, x-edge, y-edge rows
    DeviceBuffer<double> conf_partials;
    DeviceBuffer<ConfStats> conf_stats;
    PinnedBuffer<ConfStats> h_conf_stats;
    // room for npix pixels; earlier reconstructions on `stream` may still use smaller buffers
    void ensure(size_t npix, hipStream_t stream);
    void ensure_confidence(size_t npix, hipStream_t stream);
};

ReconWorkspace &recon_workspace(int dev, hipStream_t stream);

rl1::Geo recon_geo(int w, int h);
inline int recon_blocks(const rl1::Geo &g) { return g.tiles < rl1::kMaxBlocks ? g.tiles : rl1::kMaxBlocks; }
// pcg_step_b runs on the same grid, a thread per pixel: the groups of kBlock consecutive pixels its blocks stride over
inline int recon_pixel_groups(const rl1::Geo &g) { return (int)(((size_t)g.w * g.h + rl1::kBlock - 1) / rl1::kBlock); }

// round_init_kernel after a weights pass over `nb` blocks: the round's scalars (reset == 0: only the energy)
void recon_round_init(ReconWorkspace &ws, int nb, double tol, int reset, hipStream_t stream);
// ws.state -> ws.h_state behind ws.ev[2]
void recon_read_state(ReconWorkspace &ws, hipStream_t stream);
// One inner solve on ws.wx / wy / diag / r and the partials of the weights pass before it: chunks of PCG iterations with the
// convergence flag read one chunk behind, then the residual of the iterate; waits for `stream`. Adds round k to `res`.
void recon_pcg_round(ReconWorkspace &ws, const rl1::Geo &g, int nb, double *d_out, const ReconL1Params &p, hipStream_t stream, int k,
                     ReconL1Result &res);

} // namespace gdpt
