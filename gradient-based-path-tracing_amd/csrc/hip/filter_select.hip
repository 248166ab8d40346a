// filter_select.hip — the per-pixel choice among up to 8 candidate filters, by the error estimate two independent half sessions give
// of each (include/gdpt.h: gdpt_filter_select*, where the definition stands), for gfx950.
//
// Kernel: select_kernel. Blocks loop over 16 x 16 tiles as the filters' kernels do, a thread on a pixel of the tile, and leave block
// partials through leave_block_sum for finish_runs_kernel (image_kernels.h): a fixed order, the same bits every time.
//   flags   the validity of the tile with a halo of `radius` pixels, a plane of ints staged once per tile (out of the film: 0), its row
//           sums of 2s + 1 taps (a plane of int counts, (16 + 2s) rows of pitch 16) and each thread's own column sum C, kept in a register.
//   then, candidate by candidate (the loop is unrolled over the 8 slots, so the running best, the per-candidate partial sums and the
//   candidates' pointers are all named statically: registers and scalar loads from the argument block, no scratch):
//   stage   e_j of every staged point, computed from the six planes it needs on the fly; 0.0 where the flag is 0. (16 + 2s) rows of
//           pitch 16 (s = 0) or 48.
//   rows    sums of 2s + 1 taps in increasing x for the 16 columns of every staged row, (16 + 2s) rows of pitch 16. At most
//           32 x 16 = 512 outputs: a thread takes at most two.
//   columns each thread sums 2s + 1 row sums of its own column in increasing y, divides by C, writes E_j if asked and compares with
//           the best so far (strict <, so the lowest index wins a tie).
//   After the last candidate the thread gathers its triple from T[sel] and writes out, sel and mse.
// LDS is sized by the call's radius, 12 (pitch + 16)(16 + 2s) bytes: 6 144 at s = 0, 18 432 at s = 4, 24 576 at s = 8.
// LDS banking: as smooth_kernel's (variance_smooth.hip). Every plane is a plane of doubles or of ints, so consecutive lanes read
// consecutive elements in both passes. In the row pass a half-wave covers two rows of 16 outputs; the stage's pitch of 48 doubles,
// = 16 mod 32, puts the second row's 16 doubles on the other half of the 64 banks for every tap (the pitch 16 + 2s itself would overlap
// them by 2s doubles, and at s = 8 a pitch of 32 would put both rows on the same banks). In the column pass a half-wave reads 32
// consecutive doubles of the row sums (pitch 16).
// The halo is computed again by every tile that holds it: (16 + 2s)^2 / 256 error terms per pixel and candidate, 2.25 at s = 4 and 4 at
// s = 8, of 12 doubles each. The flags read all 3n + 4 triples of every staged point and the error terms then read their six planes
// again: deliberate, as keeping them would take 9n + 12 doubles of LDS per staged point, and at 0.15 ms for six candidates the reads
// (mostly L2 hits within a tile's trip) are not what a filter bank's time goes to. No launch writes a plane it reads.
#include "../../../include/gdpt.h"
#include "../capi_common.h"
#include "image_kernels.h"
#include "filter_select.h"

#include <cmath>
#include <cstdint>
#include <limits>
#include <mutex>
#include <vector>

namespace fsel {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, leave_block_sum

constexpr int kTile = gdpt::kSelectTile;
constexpr int kMaxS = GDPT_SELECT_MAX_RADIUS;
constexpr int kMaxN = GDPT_SELECT_MAX_CANDIDATES;
static_assert(kTile * kTile == kBlock, "one thread per tile pixel");
static_assert((kTile + 2 * kMaxS) * kTile <= 2 * kBlock, "a thread computes at most two row sums");
static_assert(kTile + 2 * kMaxS <= 48, "a staged row fits the pitch");

// runs of the partials, gridDim.x doubles each
constexpr int kRunLeftOut = 0, kRunMse = 1, kRunSqOut = 2, kRunChosen = 3;       // chosen[j] at 3 + j, sum_e[j] at 3 + n + j
constexpr int kMaxRuns = 2 * kMaxN + 3;

struct Args {
    TileGrid g;                  // 16 x 16 tiles
    int s, n;
    const double *FA[kMaxN], *FB[kMaxN], *T[kMaxN];
    const double *uA, *vA, *uB, *vB;
    double *out;
    int32_t *sel;                // nullable
    double *mse, *E;             // nullable
    double *partials;
};

// pitch of the stage for rows of 16 + 2s points
__host__ __device__ inline int stage_pitch(int s) { return s == 0 ? kTile : 48; }
// bytes of the kernel's LDS: a plane of doubles and a plane of ints for the stage and for the row sums
__host__ __device__ inline size_t lds_bytes(int s) { return (size_t)(sizeof(double) + sizeof(int)) * (stage_pitch(s) + kTile) * (kTile + 2 * s); }

__device__ __forceinline__ bool finite3(const double *a, size_t p) { return isfinite(a[3 * p]) && isfinite(a[3 * p + 1]) && isfinite(a[3 * p + 2]); }
__device__ __forceinline__ bool variance3(const double *a, size_t p) {
    return finite3(a, p) && a[3 * p] >= 0.0 && a[3 * p + 1] >= 0.0 && a[3 * p + 2] >= 0.0;
}

// whether film pixel p is valid: every triple finite, the two variances >= 0
__device__ __forceinline__ bool pixel_valid(const Args &a, size_t p) {
    bool ok = finite3(a.uA, p) && finite3(a.uB, p) && variance3(a.vA, p) && variance3(a.vB, p);
#pragma unroll
    for (int j = 0; j < kMaxN; j++)
        if (j < a.n) ok = ok && finite3(a.FA[j], p) && finite3(a.FB[j], p) && finite3(a.T[j], p);
    return ok;
}

// e_j of film pixel p, every operation rounded on its own, in the order of include/gdpt.h
__device__ __forceinline__ double error_term(const double *FA, const double *FB, const Args &a, size_t p) {
#pragma clang fp contract(off)
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double dA = FA[3 * p + c] - a.uB[3 * p + c], dB = FB[3 * p + c] - a.uA[3 * p + c];
        const double qA = dA * dA, qB = dB * dB;
        t[c] = 0.5 * ((qA - a.vB[3 * p + c]) + (qB - a.vA[3 * p + c]));
    }
    return ((t[0] + t[1]) + t[2]) / 3.0;
}

__global__ __launch_bounds__(kBlock) void select_kernel(Args a) {
    extern __shared__ double lds[];
    __shared__ double red[kBlock / 64];
    const int s = a.s, taps = 2 * s + 1;
    const int sw = kTile + 2 * s, sp = stage_pitch(s), sn = sp * sw;      // the stage: sw rows of sw points, pitch sp
    const int hn = kTile * sw;                                           // the row sums: sw rows of 16
    double *const pe = lds;
    double *const ph = lds + sn;
    int *const sflag = (int *)(ph + hn);
    int *const ch = sflag + sn;
    const int tid = threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;
    const int pc = (ly + s) * sp + lx + s;              // the thread's own pixel in the stage
    const size_t plane = (size_t)a.g.w * a.g.h;
    double left_out = 0.0, sum_mse = 0.0, sum_sq = 0.0;
    double chosen[kMaxN], sum_e[kMaxN];
#pragma unroll
    for (int j = 0; j < kMaxN; j++) chosen[j] = sum_e[j] = 0.0;
    for (int t = blockIdx.x; t < a.g.tiles; t += gridDim.x) {
        const TilePixel tp = tile_pixel<kTile, kTile>(a.g, t);
        __syncthreads();                                // the previous tile's stage and row sums have been read
        for (int k = tid; k < sw * sw; k += kBlock) {
            const int ry = k / sw, rx = k - ry * sw;
            const int gx = tp.x0 - s + rx, gy = tp.y0 - s + ry;
            bool ok = false;
            if (gx >= 0 && gy >= 0 && gx < a.g.w && gy < a.g.h) ok = pixel_valid(a, (size_t)gy * a.g.w + gx);
            sflag[ry * sp + rx] = ok ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int q = tid + k * kBlock;             // row q / 16 of the stage, column q % 16 of the tile
            if (q >= hn) continue;
            const int i = (q / kTile) * sp + (q & (kTile - 1));
            int C = 0;
            for (int m = 0; m < taps; m++) C += sflag[i + m];
            ch[q] = C;
        }
        __syncthreads();
        const int x = tp.x, y = tp.y;
        const bool inside = x < a.g.w && y < a.g.h;
        const size_t p = inside ? (size_t)y * a.g.w + x : 0;
        const bool valid = inside && sflag[pc] != 0;
        int C = 0;
        for (int m = 0; m < taps; m++) C += ch[tid + m * kTile];
        const double count = (double)C;                 // (>= 1 for a valid pixel: it counts itself)
        double best_e = 0.0;
        int best = -1;
#pragma unroll
        for (int j = 0; j < kMaxN; j++) {
            if (j >= a.n) break;
            if (j > 0) __syncthreads();                 // the previous candidate's stage and row sums have been read
            for (int k = tid; k < sw * sw; k += kBlock) {
                const int ry = k / sw, rx = k - ry * sw;
                const int i = ry * sp + rx;
                double e = 0.0;
                if (sflag[i] != 0) e = error_term(a.FA[j], a.FB[j], a, (size_t)(tp.y0 - s + ry) * a.g.w + (tp.x0 - s + rx));
                pe[i] = e;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int q = tid + k * kBlock;
                if (q >= hn) continue;
                const int i = (q / kTile) * sp + (q & (kTile - 1));
                double S = 0.0;
                for (int m = 0; m < taps; m++) S += pe[i + m];
                ph[q] = S;
            }
            __syncthreads();
            if (valid) {
                double S = 0.0;
                for (int m = 0; m < taps; m++) S += ph[tid + m * kTile];
                const double E = S / count;
                if (a.E) a.E[j * plane + p] = E;
                if (j == 0 || E < best_e) { best_e = E; best = j; }
                sum_e[j] += pe[pc];
            } else if (inside && a.E) a.E[j * plane + p] = __longlong_as_double(0x7ff8000000000000LL);
        }
        if (!inside) continue;
        double o[3] = {0.0, 0.0, 0.0};
        const int from = valid ? best : 0;
#pragma unroll
        for (int j = 0; j < kMaxN; j++) {
            if (j >= a.n) break;
            if (j == from) {
#pragma unroll
                for (int c = 0; c < 3; c++) o[c] = a.T[j][3 * p + c];
            }
            chosen[j] += (valid && j == best) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) a.out[3 * p + c] = o[c];
        if (a.sel) a.sel[p] = valid ? best : -1;
        if (a.mse) a.mse[p] = valid ? best_e : __longlong_as_double(0x7ff8000000000000LL);
        if (valid) {
            sum_mse += best_e;
            sum_sq += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
        } else left_out += 1.0;
    }
    leave_block_sum(a.partials, kRunLeftOut, left_out, red);
    leave_block_sum(a.partials, kRunMse, sum_mse, red);
    leave_block_sum(a.partials, kRunSqOut, sum_sq, red);
#pragma unroll
    for (int j = 0; j < kMaxN; j++) {
        if (j >= a.n) break;
        leave_block_sum(a.partials, kRunChosen + j, chosen[j], red);
        leave_block_sum(a.partials, kRunChosen + a.n + j, sum_e[j], red);
    }
}

} // namespace fsel

namespace gdpt {

namespace {

struct SelectWorkspace {
    std::mutex mu;                    // held while a call runs on this (device, stream) pair
    DeviceBuffer<double> partials;    // kMaxRuns runs of kMaxBlocks
    DeviceBuffer<double> d_sums;      // kMaxRuns
    PinnedBuffer<double> h_sums;
    Event ev[2];
};

// leaked on purpose, as the filter's registry (denoise_nlm.hip); a pair's entry goes with forget_stream (device_mem.h)
PerStream<SelectWorkspace> &g_workspaces = *new PerStream<SelectWorkspace>();

} // namespace

void select_check_params(const std::string &who, const GdptSelectParams &p) {
    if (p.radius < 0 || p.radius > fsel::kMaxS) throw std::runtime_error(who + ": radius must be in [0, " + std::to_string(fsel::kMaxS) + "]");
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) throw std::runtime_error(who + ": select reserved must be 0");
}

void filter_select_launch(int w, int h, int n, const double *const *d_FA, const double *const *d_FB, const double *const *d_T,
                          const double *d_uA, const double *d_vA, const double *d_uB, const double *d_vB, const GdptSelectParams &p,
                          double *d_out, int32_t *d_sel, double *d_mse, double *d_E, hipStream_t stream, GdptSelectStats *stats) {
    int dev = 0;
    ck(hipGetDevice(&dev), "hipGetDevice");
    SelectWorkspace &ws = g_workspaces.get(dev, stream);
    std::lock_guard<std::mutex> lk(ws.mu);
    if (!ws.partials) ws.partials.alloc((size_t)fsel::kMaxRuns * film::kMaxBlocks, "hipMalloc(filter select partials)");
    if (!ws.d_sums) ws.d_sums.alloc(fsel::kMaxRuns, "hipMalloc(filter select sums)");
    if (!ws.h_sums) ws.h_sums.alloc(fsel::kMaxRuns, "hipHostMalloc(filter select sums)");
    for (auto &e : ws.ev) if (!e) e.create();

    fsel::Args a{};
    a.g = film::tile_grid(w, h, kSelectTile, kSelectTile); a.s = p.radius; a.n = n;
    for (int j = 0; j < n; j++) { a.FA[j] = d_FA[j]; a.FB[j] = d_FB[j]; a.T[j] = d_T[j]; }
    a.uA = d_uA; a.vA = d_vA; a.uB = d_uB; a.vB = d_vB;
    a.out = d_out; a.sel = d_sel; a.mse = d_mse; a.E = d_E; a.partials = ws.partials;
    const int nb = a.g.blocks, runs = 2 * n + 3;
    if (stats) ck(hipEventRecord(ws.ev[0], stream), "hipEventRecord");
    hipLaunchKernelGGL(fsel::select_kernel, dim3(nb), dim3(film::kBlock), fsel::lds_bytes(a.s), stream, a);
    ck(hipGetLastError(), "filter select launch");
    if (!stats) return;
    film::launch_finish_runs(nb, runs, ws.partials, ws.d_sums, stream);
    ck(hipGetLastError(), "filter select reduction launch");
    ck(hipEventRecord(ws.ev[1], stream), "hipEventRecord");
    ck(hipMemcpyAsync(ws.h_sums, ws.d_sums, runs * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(filter select sums)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(filter select)");
    *stats = GdptSelectStats{};
    const double *sums = ws.h_sums.data();
    stats->pixels_left_out = (uint64_t)sums[fsel::kRunLeftOut];
    stats->sum_mse = sums[fsel::kRunMse]; stats->sum_sq_out = sums[fsel::kRunSqOut];
    for (int j = 0; j < n; j++) {
        stats->chosen[j] = (uint64_t)sums[fsel::kRunChosen + j];
        stats->sum_e[j] = sums[fsel::kRunChosen + n + j];
    }
    { float ms = 0; ck(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]), "hipEventElapsedTime"); stats->select_ms = ms; }
    stats->radius = p.radius; stats->num_candidates = n;
}

} // namespace gdpt

namespace {

using gdpt::ck;
using gdpt::need_a_device;

// what both entry points refuse; `who` names the caller. Returns the parameters in force.
GdptSelectParams check_arguments(const std::string &who, int width, int height, int n, const double *const *FA, const double *const *FB,
                                 const double *const *T, const double *uA, const double *vA, const double *uB, const double *vB,
                                 const GdptSelectParams *params, const double *out, const int32_t *sel, const double *mse, const double *E) {
    if (n < 1 || n > GDPT_SELECT_MAX_CANDIDATES)
        throw std::runtime_error(who + ": n must be in [1, " + std::to_string(GDPT_SELECT_MAX_CANDIDATES) + "]");
    if (!FA) throw std::runtime_error(who + ": FA is null");
    if (!FB) throw std::runtime_error(who + ": FB is null");
    if (!T) throw std::runtime_error(who + ": T is null");
    std::vector<const void *> in;
    for (int j = 0; j < n; j++) {
        if (!FA[j]) throw std::runtime_error(who + ": FA[" + std::to_string(j) + "] is null");
        if (!FB[j]) throw std::runtime_error(who + ": FB[" + std::to_string(j) + "] is null");
        if (!T[j]) throw std::runtime_error(who + ": T[" + std::to_string(j) + "] is null");
        in.push_back(FA[j]); in.push_back(FB[j]); in.push_back(T[j]);
    }
    if (!uA) throw std::runtime_error(who + ": uA is null");
    if (!vA) throw std::runtime_error(who + ": vA is null");
    if (!uB) throw std::runtime_error(who + ": uB is null");
    if (!vB) throw std::runtime_error(who + ": vB is null");
    for (const void *q : {(const void *)uA, (const void *)vA, (const void *)uB, (const void *)vB}) in.push_back(q);
    if (!out) throw std::runtime_error(who + ": out is null");
    if (width < 1 || height < 1) throw std::runtime_error(who + ": width and height must be >= 1");
    if ((long long)width * height > (1LL << 29)) throw std::runtime_error(who + ": width * height: film too large");
    // byte ranges: an output must not overlap an input or another output anywhere (every input is a W H 3 plane of doubles)
    const size_t px = (size_t)width * height, plane = px * 3 * sizeof(double);
    struct Range { const char *name; const void *p; size_t bytes; };
    const Range outs[4] = {{"out", out, plane}, {"sel", sel, px * sizeof(int32_t)}, {"mse", mse, px * sizeof(double)}, {"E", E, px * n * sizeof(double)}};
    auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    for (int i = 0; i < 4; i++) {
        if (!outs[i].p) continue;
        for (const void *q : in)
            if (overlap(outs[i].p, outs[i].bytes, q, plane)) throw std::runtime_error(who + ": " + outs[i].name + " must not alias an input");
        for (int k = 0; k < i; k++)
            if (outs[k].p && overlap(outs[i].p, outs[i].bytes, outs[k].p, outs[k].bytes))
                throw std::runtime_error(who + ": " + outs[i].name + " must not alias " + outs[k].name);
    }
    GdptSelectParams p;
    if (params) p = *params;
    else gdpt_select_default_params(&p);
    gdpt::select_check_params(who, p);
    return p;
}

} // namespace

extern "C" {

void gdpt_select_default_params(GdptSelectParams *p) {
    if (!p) return;
    *p = GdptSelectParams{};
    p->radius = 4;
}

int gdpt_filter_select_device(int width, int height, int n, const double *const *d_FA, const double *const *d_FB, const double *const *d_T,
                              const double *d_uA, const double *d_vA, const double *d_uB, const double *d_vB, const GdptSelectParams *params,
                              double *d_out, int32_t *d_sel, double *d_mse, double *d_E, void *stream, GdptSelectStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_filter_select_device";
        const GdptSelectParams p = check_arguments(who, width, height, n, d_FA, d_FB, d_T, d_uA, d_vA, d_uB, d_vB, params, d_out, d_sel, d_mse, d_E);
        need_a_device(who);
        gdpt::filter_select_launch(width, height, n, d_FA, d_FB, d_T, d_uA, d_vA, d_uB, d_vB, p, d_out, d_sel, d_mse, d_E, (hipStream_t)stream, stats);
    });
}

int gdpt_filter_select(int width, int height, int n, const double *const *FA, const double *const *FB, const double *const *T, const double *uA,
                       const double *vA, const double *uB, const double *vB, const GdptSelectParams *params, double *out, int32_t *sel, double *mse,
                       double *E, GdptSelectStats *stats) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_filter_select";
        const GdptSelectParams p = check_arguments(who, width, height, n, FA, FB, T, uA, vA, uB, vB, params, out, sel, mse, E);
        need_a_device(who);
        const size_t px = (size_t)width * height, elems = px * 3, bytes = elems * sizeof(double);
        const char *what = "hipMalloc(filter select io)";
        std::vector<gdpt::DeviceBuffer<double>> planes(3 * n + 4);
        const double *d_FA[GDPT_SELECT_MAX_CANDIDATES], *d_FB[GDPT_SELECT_MAX_CANDIDATES], *d_T[GDPT_SELECT_MAX_CANDIDATES];
        auto up = [&](gdpt::DeviceBuffer<double> &b, const double *src) {
            b.alloc(elems, what);
            ck(hipMemcpy(b, src, bytes, hipMemcpyHostToDevice), "hipMemcpy(H2D)");
            return (const double *)b;
        };
        for (int j = 0; j < n; j++) { d_FA[j] = up(planes[3 * j], FA[j]); d_FB[j] = up(planes[3 * j + 1], FB[j]); d_T[j] = up(planes[3 * j + 2], T[j]); }
        const double *d_uA = up(planes[3 * n], uA), *d_vA = up(planes[3 * n + 1], vA), *d_uB = up(planes[3 * n + 2], uB), *d_vB = up(planes[3 * n + 3], vB);
        gdpt::DeviceBuffer<double> d_out, d_mse, d_E;
        gdpt::DeviceBuffer<int32_t> d_sel;
        d_out.alloc(elems, what);
        if (sel) d_sel.alloc(px, what);
        if (mse) d_mse.alloc(px, what);
        if (E) d_E.alloc(px * n, what);
        gdpt::filter_select_launch(width, height, n, d_FA, d_FB, d_T, d_uA, d_vA, d_uB, d_vB, p, d_out, sel ? d_sel.data() : nullptr,
                                   mse ? d_mse.data() : nullptr, E ? d_E.data() : nullptr, nullptr, stats);
        ck(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (sel) ck(hipMemcpy(sel, d_sel, px * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (mse) ck(hipMemcpy(mse, d_mse, px * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
        if (E) ck(hipMemcpy(E, d_E, px * n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    });
}

} // extern "C"
