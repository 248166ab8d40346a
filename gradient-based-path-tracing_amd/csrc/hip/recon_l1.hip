// recon_l1.hip — robust (L1) reconstruction of a gradient-domain render for gfx950: iteratively reweighted least squares
// (IRLS) over a weighted screened-Poisson system solved by Jacobi-preconditioned conjugate gradients.
//
// Definition (include/gdpt.h, gdpt_reconstruct). Image f, primal u, gradients gx, gy: H x W x 3 fp64, interleaved RGB.
// Residual rows, three channels each:
//     data row of pixel (x,y):   r_d = sqrt(alpha) (f - u)
//     x-edge row, x >= 1:        r_x = f(x,y) - f(x-1,y) - gx(x,y)
//     y-edge row, y >= 1:        r_y = f(x,y) - f(x,y-1) - gy(x,y)
// Edges exist inside the film only (natural boundary; gx(0,.) and gy(.,0) are not read) — NOT the mirror operator of
// fourierSolve. One weight per row, shared by its channels (no colour shift): w = 1 / (eps_k + |r|_2). Round 0 has w = 1;
// round k = 1..K takes w from f_{k-1} with eps_k = max(eps_init eps_decay^(k-1), eps_floor) and solves, per channel,
//     (alpha diag(w_d) + Dx^T diag(w_x) Dx + Dy^T diag(w_y) Dy) f = alpha w_d u + Dx^T (w_x gx) + Dy^T (w_y gy)
// warm-started from f_{k-1} (round 0: from u), until |r| <= cg_tol |b| or cg_max_iters. Energy E(f) = sum over rows of |r|_2.
//
// Kernels. A thread owns a PIXEL (its three channels), so every weight is loaded once for three unknowns.
//   weights_kernel   (recon_pcg.h, with the positional row policy) one pass over f, u, gx, gy per round: the two edge-weight planes wx(x,y) (edge x-1|x; 0 at x = 0) and
//                    wy(x,y), the diagonal alpha w_d + sum of the four edge weights (the Jacobi preconditioner AND the
//                    centre tap: w_d itself is never needed again, so it is not stored), the initial residual b - A f
//                    (formed from the residual rows, not as a difference of two large numbers) and the block partials of
//                    <r,z>, <r,r>, <b,b> and the energy E(f) of the iterate the weights were taken from.
//   pcg_step_a       p' = z + beta p with z = r / diag, staged for a 32 x 8 pixel tile and its one-pixel halo in LDS
//                    (planar per channel: a half-wave reads 32 consecutive doubles, conflict-free); q = A p' from the LDS
//                    tile; partial <p',q>.
//   pcg_step_b       x += a p', r -= a q; partials <r,z>, <r,r>.
// Two launches per iteration and no host round trip: scalars are reduced from per-block partials by every block in the
// same fixed order, so the same inputs give the same bits. The host reads the convergence flag one chunk of iterations
// behind the launches, as the CG of poisson_kernels.hip does; kernels of a converged solve return at once.
// Grid: film::tile_grid (image_kernels.h), one block of 256 threads per tile, at most kMaxBlocks blocks striding over the tiles; 8 KB of LDS, 50 VGPRs and no scratch, i.e. occupancy is bound by neither.
#include "recon_l1.h"
#include "recon_pcg.h"
#include "../capi_common.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <stdexcept>
#include <string>

namespace rl1 {

// partials layout (recon_pcg.h: weights_kernel): slot s of gridDim.x doubles: [0] <r,z>, [1] <r,r>, [2] <b,b>, [3] energy, [4] <p,q>

// one block, after a weights pass: the round's scalars. reset == 0: only the energy (after weights_kernel<false>).
__global__ __launch_bounds__(kBlock) void round_init_kernel(int nb, const double *partials, State *st, double tol, int reset) {
    __shared__ double red[kBlock / 64];
    const double e = reduce_partials(partials + 3 * nb, nb, red);
    double bb = 0;
    if (reset) bb = reduce_partials(partials + 2 * nb, nb, red);
    if (threadIdx.x == 0) {
        st->energy = e;
        if (reset) { st->bb = bb; st->rz[0] = 1.0; st->rz[1] = 1.0; st->tol = tol; st->rel = 0.0; st->iters = 0; st->converged = 0; }
    }
}

// iteration `it` of a round (parity selects the p buffers; it == 0 reads no p_in): p_out = z + beta p_in, q = A p_out, partial <p_out,q>
__global__ __launch_bounds__(kBlock) void pcg_step_a(TileGrid g, int it, const double *r, const double *p_in, double *p_out, double *q,
                                                     const double *wx, const double *wy, const double *diag,
                                                     const double *part_rz, const double *part_rr, double *part_pq, State *st) {
    __shared__ double sp[3][kTileH + 2][kPitch];
    __shared__ double red[kBlock / 64];
    if (st->converged) return;
    const int nb = gridDim.x;
    const double rz_new = reduce_partials(part_rz, nb, red);
    const double rr_new = reduce_partials(part_rr, nb, red);
    const double bb = st->bb;
    const double rel = bb > 0 ? sqrt(rr_new / bb) : 0.0;
    if (rel <= st->tol) {                                  // uniform over the whole grid: same inputs in every block
        if (blockIdx.x == 0 && threadIdx.x == 0) st->converged = 1;
        return;
    }
    const double beta = it == 0 ? 0.0 : rz_new / st->rz[(it + 1) & 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) st->rz[it & 1] = rz_new;
    // p' of pixel (x,y), 0 outside the film
    auto direction = [&](int x, int y, double *pv, double &dg) {
        pv[0] = pv[1] = pv[2] = 0.0; dg = 0.0;
        if (x < 0 || y < 0 || x >= g.w || y >= g.h) return;
        const int pix = y * g.w + x, i = 3 * pix;
        dg = diag[pix];
        const double inv = 1.0 / dg;
#pragma unroll
        for (int c = 0; c < 3; c++) pv[c] = it == 0 ? r[i + c] * inv : r[i + c] * inv + beta * p_in[i + c];
    };
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    double s = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTileW, kTileH>(g, t);
        const int x0 = tp.x0, y0 = tp.y0, x = tp.x, y = tp.y;
        double pv[3], dg;
        direction(x, y, pv, dg);
        __syncthreads();                                   // the previous tile's taps have been read
#pragma unroll
        for (int c = 0; c < 3; c++) sp[c][ly + 1][lx + 1] = pv[c];
        if (threadIdx.x < kHalo) {
            const int k = threadIdx.x;
            int hx, hy;                                    // tile-local, -1 .. kTileW / kTileH
            if (k < kTileW) { hx = k; hy = -1; }
            else if (k < 2 * kTileW) { hx = k - kTileW; hy = kTileH; }
            else if (k < 2 * kTileW + kTileH) { hx = -1; hy = k - 2 * kTileW; }
            else { hx = kTileW; hy = k - 2 * kTileW - kTileH; }
            double hv[3], hd;
            direction(x0 + hx, y0 + hy, hv, hd);
#pragma unroll
            for (int c = 0; c < 3; c++) sp[c][hy + 1][hx + 1] = hv[c];
        }
        __syncthreads();
        if (x < g.w && y < g.h) {
            const int pix = y * g.w + x, i = 3 * pix;
            const double w_l = wx[pix], w_u = wy[pix];     // 0 on the film's first column / row
            const double w_r = x + 1 < g.w ? wx[pix + 1] : 0.0, w_d = y + 1 < g.h ? wy[pix + g.w] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double qi = dg * pv[c] - ((w_l * sp[c][ly + 1][lx] + w_r * sp[c][ly + 1][lx + 2]) + (w_u * sp[c][ly][lx + 1] + w_d * sp[c][ly + 2][lx + 1]));
                p_out[i + c] = pv[c]; q[i + c] = qi;
                s += pv[c] * qi;
            }
        }
    }
    leave_block_sum(part_pq, 0, s, red);
}

__global__ __launch_bounds__(kBlock) void pcg_step_b(int npix, int it, const double *p, const double *q, const double *diag, double *x, double *r,
                                                     const double *part_pq, double *part_rz, double *part_rr, State *st) {
    __shared__ double red[kBlock / 64];
    if (st->converged) return;
    const int nb = gridDim.x;
    const double pq = reduce_partials(part_pq, nb, red);
    const double a = st->rz[it & 1] / pq;
    double s_rr = 0, s_rz = 0;
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < npix; pix += gridDim.x * kBlock) {
        const double dg = diag[pix];
        const int i = 3 * pix;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[i + c] += a * p[i + c];
            const double ri = r[i + c] - a * q[i + c];
            r[i + c] = ri;
            s_rr += ri * ri; s_rz += ri * ri / dg;
        }
    }
    leave_block_sum(part_rz, 0, s_rz, red);
    leave_block_sum(part_rr, 0, s_rr, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) st->iters = it + 1;
}

// one block, at the end of a round: |r| / |b| of the iterate as it stands
__global__ __launch_bounds__(kBlock) void pcg_residual_kernel(int nb, const double *part_rr, State *st) {
    __shared__ double red[kBlock / 64];
    const double rr = reduce_partials(part_rr, nb, red);
    if (threadIdx.x == 0) st->rel = st->bb > 0 ? sqrt(rr / st->bb) : 0.0;
}

} // namespace rl1

namespace gdpt {

namespace {

// leaked on purpose: no HIP call is made from a static destructor (as the solver's registry, poisson_kernels.hip); a pair's entry
// goes with forget_stream (device_mem.h)
PerStream<ReconWorkspace> &g_workspaces = *new PerStream<ReconWorkspace>();

} // namespace

void ReconWorkspace::ensure(size_t npix, hipStream_t stream) {
    for (auto *b : {&r, &q, &p0, &p1}) b->grow(3 * npix, stream, "hipMalloc(recon workspace)");
    for (auto *b : {&wx, &wy, &diag}) b->grow(npix, stream, "hipMalloc(recon weights)");
    if (ev[2]) return;                    // the rest has one size, and is made once
    partials.alloc(5 * film::kMaxBlocks, "hipMalloc(recon partials)");
    state.alloc(1, "hipMalloc(recon state)");
    h_state.alloc(1, "hipHostMalloc");
    for (auto &e : ev) e.create();
}
void ReconWorkspace::ensure_confidence(size_t npix, hipStream_t stream) {
    for (auto &b : var) b.grow(npix, stream, "hipMalloc(recon row variances)");
    for (auto &b : conf) b.grow(npix, stream, "hipMalloc(recon confidences)");
    if (!conf_partials) conf_partials.alloc(kConfSlots * film::kMaxBlocks, "hipMalloc(recon confidence partials)");
    if (!conf_stats) conf_stats.alloc(1, "hipMalloc(recon confidence scalars)");
    if (!h_conf_stats) h_conf_stats.alloc(1, "hipHostMalloc");
}

ReconWorkspace &recon_workspace(int dev, hipStream_t stream) { return g_workspaces.get(dev, stream); }

void recon_round_init(ReconWorkspace &ws, int nb, double tol, int reset, hipStream_t stream) {
    hipLaunchKernelGGL(rl1::round_init_kernel, dim3(1), dim3(film::kBlock), 0, stream, nb, ws.partials, ws.state, tol, reset);
}

void recon_read_state(ReconWorkspace &ws, hipStream_t stream) {
    ck(hipMemcpyAsync(ws.h_state, ws.state, sizeof(rl1::State), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(state)");
    ck(hipEventRecord(ws.ev[2], stream), "hipEventRecord");
}

void recon_pcg_round(ReconWorkspace &ws, const film::TileGrid &g, double *d_out, const ReconL1Params &p, hipStream_t stream, int k,
                     ReconL1Result &res) {
    const int nb = g.blocks;
    double *part_rz = ws.partials, *part_rr = ws.partials + nb, *part_pq = ws.partials + 4 * (size_t)nb;
    const dim3 grid(nb), block(film::kBlock);
    const int npix = g.w * g.h, chunk = 32;
    int launched = 0;
    auto enqueue_chunk = [&]() {
        const int n = std::min(chunk, p.cg_max_iters - launched);
        for (int j = 0; j < n; j++) {
            const int it = launched + j;
            const double *pin = (it & 1) ? ws.p1 : ws.p0;
            double *pout = (it & 1) ? ws.p0 : ws.p1;
            hipLaunchKernelGGL(rl1::pcg_step_a, grid, block, 0, stream, g, it, ws.r, pin, pout, ws.q, ws.wx, ws.wy, ws.diag, part_rz, part_rr, part_pq, ws.state);
            hipLaunchKernelGGL(rl1::pcg_step_b, grid, block, 0, stream, npix, it, pout, ws.q, ws.diag, d_out, ws.r, part_pq, part_rz, part_rr, ws.state);
        }
        launched += n;
        ck(hipGetLastError(), "recon chunk launch");
    };
    // one chunk is always in flight ahead of the status check of the previous one; its kernels return at once if converged
    enqueue_chunk();
    for (bool done = false; !done;) {
        recon_read_state(ws, stream);
        const bool more = launched < p.cg_max_iters;
        if (more) enqueue_chunk();
        ck(hipEventSynchronize(ws.ev[2]), "hipEventSynchronize");
        if (ws.h_state->converged || !more) done = true;
    }
    hipLaunchKernelGGL(rl1::pcg_residual_kernel, dim3(1), block, 0, stream, nb, part_rr, ws.state);
    ck(hipGetLastError(), "recon residual launch");
    recon_read_state(ws, stream);
    ck(hipEventSynchronize(ws.ev[2]), "hipEventSynchronize");
    if (k == 1) res.energy_first = ws.h_state->energy;       // the weights of round 1 were taken from f_0
    res.cg_iters_last = ws.h_state->iters; res.cg_iters_total += ws.h_state->iters;
    res.rel_residual_last = ws.h_state->rel;
    res.irls_rounds = k + 1;
}

ReconL1Result recon_l1_device(int w, int h, const double *d_c, const double *d_gx, const double *d_gy, double alpha,
                              const ReconL1Params &p, double *d_out, hipStream_t stream) {
    if (w < 2 || h < 2) throw std::runtime_error("reconstruct: width and height must be >= 2");
    if (!(alpha > 0) || !std::isfinite(alpha)) throw std::runtime_error("reconstruct: dataCost must be > 0");
    if ((long long)w * h > (1LL << 29)) throw std::runtime_error("reconstruct: film too large");
    if (d_out == d_c || d_out == d_gx || d_out == d_gy) throw std::runtime_error("reconstruct: the output must not alias an input");
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    ReconWorkspace &ws = recon_workspace(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    ws.ensure((size_t)w * h, stream);
    const film::TileGrid g = film::tile_grid(w, h, rl1::kTileW, rl1::kTileH);
    const int nb = g.blocks;
    const dim3 grid(nb), block(film::kBlock);
    ReconL1Result res{};
    ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    for (int k = 0; k <= p.irls_iters; k++) {
        const double eps = k == 0 ? 0.0 : std::max(p.eps_init * std::pow(p.eps_decay, k - 1), p.eps_floor);
        hipLaunchKernelGGL((rl1::weights_kernel<rl1::PositionalRows, true>), grid, block, 0, stream, g, alpha, eps, k == 0 ? 1 : 0,
                           k == 0 ? d_c : (const double *)d_out, d_c, d_gx, d_gy, rl1::PositionalRows::Planes{}, k == 0 ? d_out : (double *)nullptr,
                           ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
        recon_round_init(ws, nb, p.cg_tol, 1, stream);
        ck(hipGetLastError(), "recon round launch");
        recon_pcg_round(ws, g, d_out, p, stream, k, res);
    }
    hipLaunchKernelGGL((rl1::weights_kernel<rl1::PositionalRows, false>), grid, block, 0, stream, g, alpha, 0.0, 1, (const double *)d_out, d_c, d_gx, d_gy,
                       rl1::PositionalRows::Planes{}, (double *)nullptr, ws.wx, ws.wy, ws.diag, ws.r, ws.partials);
    recon_round_init(ws, nb, p.cg_tol, 0, stream);
    ck(hipGetLastError(), "recon energy launch");
    recon_read_state(ws, stream);
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipEventSynchronize(ws.ev[1]), "hipEventSynchronize");
    res.energy_last = ws.h_state->energy;
    if (p.irls_iters == 0) res.energy_first = res.energy_last;
    float ms = 0;
    ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime");
    res.solve_ms = ms;
    return res;
}

} // namespace gdpt
