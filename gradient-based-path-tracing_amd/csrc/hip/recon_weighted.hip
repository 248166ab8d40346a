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
// Kernels. A thread owns a PIXEL, over the 32 x 8 tiles of rl1::Geo (consecutive threads read consecutive 24-byte triples).
//   confidence_stats_kernel    one pass over the six input planes: the row variances v_d, v_x, v_y (-1: no such row, or invalid)
//                              and the block partials of sum log v and of the row counts of the two families.
//   confidence_reduce_kernel   one block: the partials in a fixed order (xor tree in a wave, waves and blocks in index order) into
//                              s_d, s_g and the counts, in device memory.
//   confidence_kernel          kappa_d, kappa_x, kappa_y from the v planes and the scales; the start of the iterate (c where the
//                              data row is valid, 0 elsewhere: no NaN enters the solve); partials of the isolated pixels.
//   weighted_weights_kernel    weights_kernel's arithmetic with kappa multiplied into the five row weights of a pixel and into the
//                              energy: three more 8-byte planes per pixel (the right and lower neighbours' kappa are cache hits).
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

__global__ __launch_bounds__(kBlock) void confidence_stats_kernel(Geo g, const double *c, const double *gx, const double *gy, const double *vc,
                                                                  const double *vgx, const double *vgy, double *vd, double *vx, double *vy,
                                                                  double *partials) {
    __shared__ double red[kBlock / 64];
    double s_ld = 0, s_nd = 0, s_lg = 0, s_ng = 0, s_bad = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
        const int x = tx * kTileW + (threadIdx.x & (kTileW - 1)), y = ty * kTileH + (threadIdx.x / kTileW);
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
    const int nb = gridDim.x;
    double v;
    v = block_sum(s_ld, red); if (threadIdx.x == 0) partials[0 * nb + blockIdx.x] = v;
    v = block_sum(s_nd, red); if (threadIdx.x == 0) partials[1 * nb + blockIdx.x] = v;
    v = block_sum(s_lg, red); if (threadIdx.x == 0) partials[2 * nb + blockIdx.x] = v;
    v = block_sum(s_ng, red); if (threadIdx.x == 0) partials[3 * nb + blockIdx.x] = v;
    v = block_sum(s_bad, red); if (threadIdx.x == 0) partials[4 * nb + blockIdx.x] = v;
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

__global__ __launch_bounds__(kBlock) void confidence_kernel(Geo g, double delta, const double *vd, const double *vx, const double *vy,
                                                            const gdpt::ConfStats *cs, const double *c, double *kd, double *kx, double *ky,
                                                            double *x_init, double *partials) {
    __shared__ double red[kBlock / 64];
    const double sd = cs->scale_data, sg = cs->scale_grad;
    double s_iso = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
        const int x = tx * kTileW + (threadIdx.x & (kTileW - 1)), y = ty * kTileH + (threadIdx.x / kTileW);
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
    const double v = block_sum(s_iso, red);
    if (threadIdx.x == 0) partials[5 * gridDim.x + blockIdx.x] = v;
}

// partials as weights_kernel's: [0] <r,z>, [1] <r,r>, [2] <b,b>, [3] energy. unit != 0: row weights kappa (round 0);
// otherwise kappa / (eps + |r|_2). f is the iterate (finite everywhere). WRITE = false: only the energy partials.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void weighted_weights_kernel(Geo g, double alpha, double eps, int unit, const double *f, const double *u,
                                                                  const double *gx, const double *gy, const double *kd, const double *kx,
                                                                  const double *ky, double *wx, double *wy, double *diag, double *r,
                                                                  double *partials) {
    __shared__ double red[kBlock / 64];
    const int row = 3 * g.w;
    double s_rz = 0, s_rr = 0, s_bb = 0, s_e = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
        const int x = tx * kTileW + (threadIdx.x & (kTileW - 1)), y = ty * kTileH + (threadIdx.x / kTileW);
        if (x >= g.w || y >= g.h) continue;
        const int pix = y * g.w + x, i = 3 * pix;
        const double k_d = kd[pix], k_l = kx[pix], k_u = ky[pix];          // 0 on the film's first column / row
        const double k_r = x + 1 < g.w ? kx[pix + 1] : 0.0, k_dn = y + 1 < g.h ? ky[pix + g.w] : 0.0;
        // a row with kappa = 0 is selected out: its inputs are not read
        const bool on_d = k_d > 0, on_l = k_l > 0, on_u = k_u > 0, on_r = k_r > 0, on_dn = k_dn > 0;
        double fc[3], uc[3] = {0, 0, 0}, d[3] = {0, 0, 0}, el[3] = {0, 0, 0}, er[3] = {0, 0, 0}, eu[3] = {0, 0, 0}, ed[3] = {0, 0, 0};
        double gl[3] = {0, 0, 0}, gr[3] = {0, 0, 0}, gu[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            fc[c] = f[i + c];
            if (on_d) { uc[c] = u[i + c]; d[c] = fc[c] - uc[c]; }
            if (on_l) { gl[c] = gx[i + c]; el[c] = (fc[c] - f[i - 3 + c]) - gl[c]; }
            if (on_r) { gr[c] = gx[i + 3 + c]; er[c] = (f[i + 3 + c] - fc[c]) - gr[c]; }
            if (on_u) { gu[c] = gy[i + c]; eu[c] = (fc[c] - f[i - row + c]) - gu[c]; }
            if (on_dn) { gd[c] = gy[i + row + c]; ed[c] = (f[i + row + c] - fc[c]) - gd[c]; }
        }
        const double n_d = sqrt(alpha) * norm3(d), n_l = norm3(el), n_u = norm3(eu);
        s_e += k_d * n_d + k_l * n_l + k_u * n_u;                          // every row once: its data row and the two edges it owns
        if (!WRITE) continue;
        const double w_d = k_d * (unit ? 1.0 : 1.0 / (eps + n_d));
        const double w_l = k_l * (unit ? 1.0 : 1.0 / (eps + n_l));
        const double w_u = k_u * (unit ? 1.0 : 1.0 / (eps + n_u));
        const double w_r = k_r * (unit ? 1.0 : 1.0 / (eps + norm3(er)));
        const double w_dn = k_dn * (unit ? 1.0 : 1.0 / (eps + norm3(ed)));
        double dg = alpha * w_d + ((w_l + w_r) + (w_u + w_dn));
        if (!(dg > 0)) dg = 1.0;                                           // isolated pixel: 1 f = 0
        wx[pix] = w_l; wy[pix] = w_u; diag[pix] = dg;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double b = alpha * w_d * uc[c] + ((w_l * gl[c] - w_r * gr[c]) + (w_u * gu[c] - w_dn * gd[c]));
            double ri = -(alpha * w_d * d[c] + ((w_l * el[c] - w_r * er[c]) + (w_u * eu[c] - w_dn * ed[c])));     // b - A f
            if (!on_d && !on_l && !on_u && !on_r && !on_dn) ri = -fc[c];
            r[i + c] = ri;
            s_rr += ri * ri; s_rz += ri * ri / dg; s_bb += b * b;
        }
    }
    const int nb = gridDim.x;
    double v;
    v = block_sum(s_e, red); if (threadIdx.x == 0) partials[3 * nb + blockIdx.x] = v;
    if (!WRITE) return;
    v = block_sum(s_rz, red); if (threadIdx.x == 0) partials[0 * nb + blockIdx.x] = v;
    v = block_sum(s_rr, red); if (threadIdx.x == 0) partials[1 * nb + blockIdx.x] = v;
    v = block_sum(s_bb, red); if (threadIdx.x == 0) partials[2 * nb + blockIdx.x] = v;
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
    const rl1::Geo g = recon_geo(w, h);
    const int nb = recon_blocks(g);
    const dim3 grid(nb), block(rl1::kBlock);
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
    for (int k = 0; k <= p.irls_iters; k++) {
        const double eps = k == 0 ? 0.0 : std::max(p.eps_init * std::pow(p.eps_decay, k - 1), p.eps_floor);
        hipLaunchKernelGGL(rw::weighted_weights_kernel<true>, grid, block, 0, stream, g, alpha, eps, k == 0 ? 1 : 0, (const double *)d_out, d_c, d_gx, d_gy,
                           ws.conf[0], ws.conf[1], ws.conf[2], ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
        recon_round_init(ws, nb, p.cg_tol, 1, stream);
        ck(hipGetLastError(), "recon round launch");
        recon_pcg_round(ws, g, nb, d_out, p, stream, k, res);
    }
    hipLaunchKernelGGL(rw::weighted_weights_kernel<false>, grid, block, 0, stream, g, alpha, 0.0, 1, (const double *)d_out, d_c, d_gx, d_gy,
                       ws.conf[0], ws.conf[1], ws.conf[2], ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
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
