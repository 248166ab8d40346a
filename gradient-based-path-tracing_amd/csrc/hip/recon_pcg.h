// recon_pcg.h — what the reconstructions built on recon_l1.hip's weighted PCG share: the tile size, the solver's state, the
// per-(device, stream) scratch and the host side of one inner solve (grid rules and reductions: image_kernels.h). The PCG kernels
// themselves stay in recon_l1.hip; the weights pass (weights_kernel, here) is one kernel under two row policies, and whoever
// launches it hands the round to recon_pcg_round.
#pragma once
#include "device_mem.h"
#include "image_kernels.h"
#include "recon_l1.h"

#include <mutex>

namespace rl1 {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, block_sum, reduce_partials, leave_block_sum

constexpr int kTileW = 32, kTileH = 8, kPitch = kTileW + 2;
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

__device__ __forceinline__ double norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// ---- the weights pass of an IRLS round, once for both reconstructions ----------------------------------------------------------
// A pixel has five residual rows: its data row, and the edges to its left, upper, right and lower neighbour. A ROW POLICY says which
// of them count (a row that is `on` is loaded; the e* / g* of one that is not stay exact zeros, which is why it adds nothing to b,
// to the residual or to the energy, whatever its inputs hold), how a row's weight 1 or 1 / (eps + |r|_2) is scaled, and how the three
// rows a pixel owns add up to its energy. Both expressions stay whole inside the policy: with -ffp-contract=on a product is fused into
// a sum only where both stand in one expression, and the bits of either reconstruction depend on exactly which ones are.
enum Row { kData = 0, kLeft, kUp, kRight, kDown };

// L1 (recon_l1.hip): a row exists by the pixel's position; kappa is 1 where it exists. Loads no plane.
struct PositionalRows {
    struct Planes {};
    static constexpr bool kFixIsolated = false, kWritesInit = true;
    bool on[5];
    __device__ __forceinline__ PositionalRows(const Planes &, const TileGrid &g, int x, int y, int)
        : on{true, x > 0, y > 0, x + 1 < g.w, y + 1 < g.h} {}
    __device__ __forceinline__ double scaled(Row r, double w) const { return on[r] ? w : 0.0; }
    __device__ __forceinline__ double energy(double n_d, double n_l, double n_u) const { return n_d + (on[kLeft] ? n_l : 0.0) + (on[kUp] ? n_u : 0.0); }
};
// variance-weighted (recon_weighted.hip): kappa from the planes kd, kx, ky (0 on the film's first column / row); a row with kappa = 0
// is selected out, and a pixel all of whose rows are gets diagonal 1 and residual -f: 1 f = 0.
struct PlaneRows {
    struct Planes { const double *kd, *kx, *ky; };
    static constexpr bool kFixIsolated = true, kWritesInit = false;
    double k[5];
    bool on[5];
    __device__ __forceinline__ PlaneRows(const Planes &p, const TileGrid &g, int x, int y, int pix) {
        k[kData] = p.kd[pix]; k[kLeft] = p.kx[pix]; k[kUp] = p.ky[pix];
        k[kRight] = x + 1 < g.w ? p.kx[pix + 1] : 0.0; k[kDown] = y + 1 < g.h ? p.ky[pix + g.w] : 0.0;
#pragma unroll
        for (int r = 0; r < 5; r++) on[r] = k[r] > 0;
    }
    __device__ __forceinline__ double scaled(Row r, double w) const { return k[r] * w; }
    __device__ __forceinline__ double energy(double n_d, double n_l, double n_u) const { return k[kData] * n_d + k[kLeft] * n_l + k[kUp] * n_u; }
};

// partials layout: slot s of gridDim.x doubles: [0] <r,z>, [1] <r,r>, [2] <b,b>, [3] energy ([4] <p,q> belongs to the PCG).
// unit != 0: the rows' weights are their kappa alone (round 0). x_init (nullable; policies with kWritesInit): receives a copy of f
// (round 0 of L1: the iterate starts at u). WRITE = false: only the energy partials (the energy of the last iterate).
template <class Rows, bool WRITE>
__global__ __launch_bounds__(kBlock) void weights_kernel(TileGrid g, double alpha, double eps, int unit, const double *f, const double *u,
                                                         const double *gx, const double *gy, typename Rows::Planes planes, double *x_init,
                                                         double *wx, double *wy, double *diag, double *r, double *partials) {
    __shared__ double red[kBlock / 64];
    const int row = 3 * g.w;
    double s_rz = 0, s_rr = 0, s_bb = 0, s_e = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTileW, kTileH>(g, t);
        const int x = tp.x, y = tp.y;
        if (x >= g.w || y >= g.h) continue;
        const int pix = y * g.w + x, i = 3 * pix;
        const Rows rows(planes, g, x, y, pix);
        double fc[3], uc[3] = {0, 0, 0}, d[3] = {0, 0, 0}, el[3] = {0, 0, 0}, er[3] = {0, 0, 0}, eu[3] = {0, 0, 0}, ed[3] = {0, 0, 0};
        double gl[3] = {0, 0, 0}, gr[3] = {0, 0, 0}, gu[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            fc[c] = f[i + c];
            if (rows.on[kData]) { uc[c] = u[i + c]; d[c] = fc[c] - uc[c]; }
            if (rows.on[kLeft]) { gl[c] = gx[i + c]; el[c] = (fc[c] - f[i - 3 + c]) - gl[c]; }
            if (rows.on[kRight]) { gr[c] = gx[i + 3 + c]; er[c] = (f[i + 3 + c] - fc[c]) - gr[c]; }
            if (rows.on[kUp]) { gu[c] = gy[i + c]; eu[c] = (fc[c] - f[i - row + c]) - gu[c]; }
            if (rows.on[kDown]) { gd[c] = gy[i + row + c]; ed[c] = (f[i + row + c] - fc[c]) - gd[c]; }
        }
        const double n_d = sqrt(alpha) * norm3(d), n_l = norm3(el), n_u = norm3(eu);
        s_e += rows.energy(n_d, n_l, n_u);                                 // every row once: its data row and the two edges it owns
        if (!WRITE) continue;
        const double w_d = rows.scaled(kData, unit ? 1.0 : 1.0 / (eps + n_d));
        const double w_l = rows.scaled(kLeft, unit ? 1.0 : 1.0 / (eps + n_l));
        const double w_u = rows.scaled(kUp, unit ? 1.0 : 1.0 / (eps + n_u));
        const double w_r = rows.scaled(kRight, unit ? 1.0 : 1.0 / (eps + norm3(er)));
        const double w_dn = rows.scaled(kDown, unit ? 1.0 : 1.0 / (eps + norm3(ed)));
        double dg = alpha * w_d + ((w_l + w_r) + (w_u + w_dn));
        const bool isolated = Rows::kFixIsolated && !rows.on[kData] && !rows.on[kLeft] && !rows.on[kUp] && !rows.on[kRight] && !rows.on[kDown];
        if (Rows::kFixIsolated && !(dg > 0)) dg = 1.0;                     // isolated pixel: 1 f = 0
        wx[pix] = w_l; wy[pix] = w_u; diag[pix] = dg;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double b = alpha * w_d * uc[c] + ((w_l * gl[c] - w_r * gr[c]) + (w_u * gu[c] - w_dn * gd[c]));
            double ri = -(alpha * w_d * d[c] + ((w_l * el[c] - w_r * er[c]) + (w_u * eu[c] - w_dn * ed[c])));     // b - A f
            if (isolated) ri = -fc[c];
            r[i + c] = ri;
            if (Rows::kWritesInit && x_init) x_init[i + c] = fc[c];
            s_rr += ri * ri; s_rz += ri * ri / dg; s_bb += b * b;
        }
    }
    leave_block_sum(partials, 3, s_e, red);
    if (!WRITE) return;
    leave_block_sum(partials, 0, s_rz, red);
    leave_block_sum(partials, 1, s_rr, red);
    leave_block_sum(partials, 2, s_bb, red);
}

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

// Every kernel of a reconstruction runs on film::tile_grid(w, h, rl1::kTileW, rl1::kTileH): g.blocks blocks. pcg_step_b, a thread
// per pixel, strides the same blocks over groups of kBlock consecutive pixels.

// round_init_kernel after a weights pass over `nb` blocks: the round's scalars (reset == 0: only the energy)
void recon_round_init(ReconWorkspace &ws, int nb, double tol, int reset, hipStream_t stream);
// ws.state -> ws.h_state behind ws.ev[2]
void recon_read_state(ReconWorkspace &ws, hipStream_t stream);
// One inner solve over g.blocks blocks on ws.wx / wy / diag / r and the partials of the weights pass before it: chunks of PCG iterations with the
// convergence flag read one chunk behind, then the residual of the iterate; waits for `stream`. Adds round k to `res`.
void recon_pcg_round(ReconWorkspace &ws, const film::TileGrid &g, double *d_out, const ReconL1Params &p, hipStream_t stream, int k,
                     ReconL1Result &res);

} // namespace gdpt
