// recon_weighted.hip — variance-weighted reconstruction of a gradient-domain render for gfx950: generalised least squares (and its
// IRLS form) over the residual rows of recon_l1.hip, each row weighted by a confidence taken from the variance of its input.
//
// Definition (include/gdpt.h, gdpt_reconstruct_weighted). Rows as in recon_l1.hip: a data row per pixel, an x-edge row for x >= 1,
// a y-edge row for y >= 1. Variance planes vc, vgx, vgy beside c, gx, gy (H x W x 3 fp64). Per row:
//     v      = sum of the row's three channel variances; the row is VALID if they are finite and >= 0, v is finite and the
//              row's c / gx / gy triple is finite
//     s_d    = exp(mean log v) over the valid data rows with v > 0;  s_g likewise over the valid x- and y-edge rows together
//              (a family without such a row: 1)
//     kappa  = s / (v + delta s)   for a valid row (v = 0: 1 / delta),   0 for an invalid one
// Round 0 solves with row weights kappa; IRLS round k >= 1 with kappa / (eps_k + |r|_2). Rows with kappa = 0 are selected out of
// the right-hand side, the residual and the energy (their values may be NaN), and a pixel all of whose rows have kappa = 0 gets
// diagonal 1 and right-hand side 0. Energies are sums of kappa |r|_2. Everything else is recon_l1.hip's: the system, the Jacobi
// PCG (its kernels, through recon_pcg_round), the warm start, the stopping rule.
//
// Kernels. A thread owns a PIXEL, over the 32 x 8 tiles of film::tile_grid (consecutive threads read consecutive 24-byte triples).
//   confidence_stats_kernel    one pass over the six input planes: the row variances v_d, v_x, v_y (-1: no such row, or invalid)
//                              and the block partials of sum log v and of the row counts of the two families.
//   confidence_reduce_kernel   one block: the partials in a fixed order (xor tree in a wave, waves and blocks in index order) into
//                              s_d, s_g and the counts, in device memory.
//   confidence_kernel          kappa_d, kappa_x, kappa_y from the v planes and the scales; the start of the iterate (c where the
//                              data row is valid, 0 elsewhere: no NaN enters the solve); partials of the isolated pixels.
//   weights_kernel             (recon_pcg.h, with the plane row policy) the weights pass of recon_l1.hip with kappa multiplied into
//                              the five row weights of a pixel and into the energy: three more 8-byte planes per pixel (the right
//                              and lower neighbours' kappa are cache hits). f is the iterate (finite everywhere).
// All of them are memory bound, use only the 32 bytes of LDS of the block reduction and no scratch.
#include "recon_weighted.h"
#include "recon_pcg.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace rw {

using namespace rl1;

// conf_partials layout: slot s of gridDim.x doubles: [0] sum log v (data), [1] rows counted in it, [2] sum log v (edges),
// [3] rows counted in it, [4] invalid rows, [5] isolated pixels
__device__ __forceinline__ bool finite3(const double *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// variance of a row, -1 if the row is invalid
__device__ __forceinline__ double row_variance(const double *val, const double *var) {
    const double v = (var[0] + var[1]) + var[2];
    const bool ok = finite3(val) && var[0] >= 0 && var[1] >= 0 && var[2] >= 0 && isfinite(v);       // NaN fails >=
    return ok ? v : -1.0;
}
__device__ __forceinline__ double confidence(double v, double s, double delta) { return v < 0 ? 0.0 : s / (v + delta * s); }

__global__ __launch_bounds__(kBlock) void confidence_stats_kernel(TileGrid g, const double *c, const double *gx, const double *gy, const double *vc,
                                                                  const double *vgx, const double *vgy, double *vd, double *vx, double *vy,
                                                                  double *partials) {
    __shared__ double red[kBlock / 64];
    double s_ld = 0, s_nd = 0, s_lg = 0, s_ng = 0, s_bad = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTileW, kTileH>(g, t);
        const int x = tp.x, y = tp.y;
        if (x >= g.w || y >= g.h) continue;
        const int pix = y * g.w + x, i = 3 * pix;
        double val[3], var[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { val[k] = c[i + k]; var[k] = vc[i + k]; }
        const double v_d = row_variance(val, var);
        double v_x = -1.0, v_y = -1.0;
        if (x > 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) { val[k] = gx[i + k]; var[k] = vgx[i + k]; }
            v_x = row_variance(val, var);
        }
        if (y > 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) { val[k] = gy[i + k]; var[k] = vgy[i + k]; }
            v_y = row_variance(val, var);
        }
        vd[pix] = v_d; vx[pix] = v_x; vy[pix] = v_y;
        if (v_d > 0) { s_ld += log(v_d); s_nd += 1.0; }
        if (v_x > 0) { s_lg += log(v_x); s_ng += 1.0; }
        if (v_y > 0) { s_lg += log(v_y); s_ng += 1.0; }
        s_bad += (v_d < 0 ? 1.0 : 0.0) + (x > 0 && v_x < 0 ? 1.0 : 0.0) + (y > 0 && v_y < 0 ? 1.0 : 0.0);
    }
    leave_block_sum(partials, 0, s_ld, red);
    leave_block_sum(partials, 1, s_nd, red);
    leave_block_sum(partials, 2, s_lg, red);
    leave_block_sum(partials, 3, s_ng, red);
    leave_block_sum(partials, 4, s_bad, red);
}

// one block. phase 0 (after confidence_stats_kernel): scales and row counts; phase 1 (after confidence_kernel): isolated pixels
__global__ __launch_bounds__(kBlock) void confidence_reduce_kernel(int nb, const double *partials, gdpt::ConfStats *cs, int phase) {
    __shared__ double red[kBlock / 64];
    if (phase == 1) {
        const double iso = reduce_partials(partials + 5 * nb, nb, red);
        if (threadIdx.x == 0) cs->pixels_isolated = iso;
        return;
    }
    double s[5];
    for (int k = 0; k < 5; k++) s[k] = reduce_partials(partials + k * nb, nb, red);
    if (threadIdx.x == 0) {
        cs->scale_data = s[1] > 0 ? exp(s[0] / s[1]) : 1.0;
        cs->scale_grad = s[3] > 0 ? exp(s[2] / s[3]) : 1.0;
        cs->rows_data = s[1]; cs->rows_grad = s[3]; cs->rows_dropped = s[4]; cs->pixels_isolated = 0.0;
    }
}

__global__ __launch_bounds__(kBlock) void confidence_kernel(TileGrid g, double delta, const double *vd, const double *vx, const double *vy,
                                                            const gdpt::ConfStats *cs, const double *c, double *kd, double *kx, double *ky,
                                                            double *x_init, double *partials) {
    __shared__ double red[kBlock / 64];
    const double sd = cs->scale_data, sg = cs->scale_grad;
    double s_iso = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTileW, kTileH>(g, t);
        const int x = tp.x, y = tp.y;
        if (x >= g.w || y >= g.h) continue;
        const int pix = y * g.w + x, i = 3 * pix;
        const double k_d = confidence(vd[pix], sd, delta), k_l = confidence(vx[pix], sg, delta), k_u = confidence(vy[pix], sg, delta);
        const double k_r = x + 1 < g.w ? confidence(vx[pix + 1], sg, delta) : 0.0;
        const double k_dn = y + 1 < g.h ? confidence(vy[pix + g.w], sg, delta) : 0.0;
        kd[pix] = k_d; kx[pix] = k_l; ky[pix] = k_u;
#pragma unroll
        for (int k = 0; k < 3; k++) x_init[i + k] = k_d > 0 ? c[i + k] : 0.0;
        if (!(k_d > 0) && !(k_l > 0) && !(k_u > 0) && !(k_r > 0) && !(k_dn > 0)) s_iso += 1.0;
    }
    leave_block_sum(partials, 5, s_iso, red);
}

} // namespace rw

namespace gdpt {

ReconWeightedResult recon_weighted_device(int w, int h, const double *d_c, const double *d_gx, const double *d_gy, const double *d_vc,
                                          const double *d_vgx, const double *d_vgy, double alpha, const ReconL1Params &p, double conf_floor,
                                          double *d_out, double *const d_conf[3], hipStream_t stream) {
    if (w < 2 || h < 2) throw std::runtime_error("reconstruct_weighted: width and height must be >= 2");
    if (!(alpha > 0) || !std::isfinite(alpha)) throw std::runtime_error("reconstruct_weighted: dataCost must be finite and > 0");
    if (!(conf_floor > 0) || !std::isfinite(conf_floor)) throw std::runtime_error("reconstruct_weighted: conf_floor must be finite and > 0");
    if ((long long)w * h > (1LL << 29)) throw std::runtime_error("reconstruct_weighted: film too large");
    for (const double *in : {d_c, d_gx, d_gy, d_vc, d_vgx, d_vgy})
        if (d_out == in) throw std::runtime_error("reconstruct_weighted: the output must not alias an input");
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    ReconWorkspace &ws = recon_workspace(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    const size_t npix = (size_t)w * h;
    ws.ensure(npix, stream);
    ws.ensure_confidence(npix, stream);
    const film::TileGrid g = film::tile_grid(w, h, rl1::kTileW, rl1::kTileH);
    const int nb = g.blocks;
    const dim3 grid(nb), block(film::kBlock);
    ReconWeightedResult out{};
    ReconL1Result &res = out.recon;
    ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    hipLaunchKernelGGL(rw::confidence_stats_kernel, grid, block, 0, stream, g, d_c, d_gx, d_gy, d_vc, d_vgx, d_vgy, ws.var[0], ws.var[1], ws.var[2],
                       ws.conf_partials);
    hipLaunchKernelGGL(rw::confidence_reduce_kernel, dim3(1), block, 0, stream, nb, ws.conf_partials, ws.conf_stats, 0);
    hipLaunchKernelGGL(rw::confidence_kernel, grid, block, 0, stream, g, conf_floor, ws.var[0], ws.var[1], ws.var[2], ws.conf_stats, d_c, ws.conf[0],
                       ws.conf[1], ws.conf[2], d_out, ws.conf_partials);
    hipLaunchKernelGGL(rw::confidence_reduce_kernel, dim3(1), block, 0, stream, nb, ws.conf_partials, ws.conf_stats, 1);
    ck(hipGetLastError(), "recon confidence launch");
    ck(hipMemcpyAsync(ws.h_conf_stats, ws.conf_stats, sizeof(ConfStats), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(confidence scalars)");
    const rl1::PlaneRows::Planes kappa{ws.conf[0], ws.conf[1], ws.conf[2]};
    for (int k = 0; k <= p.irls_iters; k++) {
        const double eps = k == 0 ? 0.0 : std::max(p.eps_init * std::pow(p.eps_decay, k - 1), p.eps_floor);
        hipLaunchKernelGGL((rl1::weights_kernel<rl1::PlaneRows, true>), grid, block, 0, stream, g, alpha, eps, k == 0 ? 1 : 0, (const double *)d_out, d_c, d_gx, d_gy,
                           kappa, (double *)nullptr, ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
        recon_round_init(ws, nb, p.cg_tol, 1, stream);
        ck(hipGetLastError(), "recon round launch");
        recon_pcg_round(ws, g, d_out, p, stream, k, res);
    }
    hipLaunchKernelGGL((rl1::weights_kernel<rl1::PlaneRows, false>), grid, block, 0, stream, g, alpha, 0.0, 1, (const double *)d_out, d_c, d_gx, d_gy,
                       kappa, (double *)nullptr, ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
    recon_round_init(ws, nb, p.cg_tol, 0, stream);
    ck(hipGetLastError(), "recon energy launch");
    recon_read_state(ws, stream);
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    if (d_conf)
        for (int k = 0; k < 3; k++)
            if (d_conf[k]) ck(hipMemcpyAsync(d_conf[k], ws.conf[k], npix * sizeof(double), hipMemcpyDefault, stream), "hipMemcpyAsync(confidence planes)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize");
    res.energy_last = ws.h_state->energy;
    if (p.irls_iters == 0) res.energy_first = res.energy_last;
    float ms = 0;
    ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime");
    res.solve_ms = ms;
    out.scale_data = ws.h_conf_stats->scale_data; out.scale_grad = ws.h_conf_stats->scale_grad;
    out.rows_dropped = (unsigned long long)ws.h_conf_stats->rows_dropped;
    out.pixels_isolated = (unsigned long long)ws.h_conf_stats->pixels_isolated;
    return out;
}

} // namespace gdpt
