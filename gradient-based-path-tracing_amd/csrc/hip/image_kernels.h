// image_kernels.h — what the image-space kernels share (poisson_kernels.hip, recon_l1.hip, recon_weighted.hip, recon_spread.hip,
// denoise_nlm.hip, progressive.hip): the block size, the fixed-order block reduction, the two grid rules and the reduction of a
// film's three sums.
//
// Every sum these modules report is the same bits run after run because it is formed in one fixed order: a thread's own terms in
// loop order, the xor tree inside a wave (wave_sum), the wave totals in index order (block_sum), and the blocks' partials strided
// over the threads of one block in index order (reduce_partials), then block_sum again. There is one copy of each step, here (but for
// the xor tree in dct_fold_gemm_f64's 512-thread epilogue, poisson_kernels.hip, which says why it keeps its own).
//
// Grid rules. A launch is either over GROUPS of kBlock consecutive elements (stride_grid: at most `cap` blocks striding over them)
// or over TW x TH pixel TILES with TW TH = kBlock (tile_grid: at most kMaxBlocks blocks striding over them). The caps keep the
// partial arrays that every block re-reduces short. The launches and gdpt_debug_image_grid (include/gdpt_debug.h) both take their
// numbers from these two functions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace film {

constexpr int kBlock = 256, kMaxBlocks = 1024;

// the xor tree inside a wave: every lane ends with the wave's total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the total of a kBlock-thread block in every thread, fixed order: xor tree inside each wave, then the wave totals in index order.
// red: kBlock / 64 doubles of LDS; may be reused at once (the first barrier stands before the write).
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < kBlock / 64; k++) s += red[k];
    return s;
}
// the total of n block partials, in every thread of a kBlock-thread block
__device__ __forceinline__ double reduce_partials(const double *part, int n, double *red) {
    double v = 0;
    for (int i = threadIdx.x; i < n; i += kBlock) v += part[i];
    return block_sum(v, red);
}
// this block's total of v into its place in run `slot` of the partials (gridDim.x doubles a run)
__device__ __forceinline__ void leave_block_sum(double *partials, int slot, double v, double *red) {
    const int nb = gridDim.x;         // (read in front of the barriers: behind them the compiler fetches it again, per call)
    const double s = block_sum(v, red);
    if (threadIdx.x == 0) partials[slot * nb + blockIdx.x] = s;
}

// n elements in groups of kBlock consecutive ones; min(cap, groups) blocks stride over the groups, at least `floor` of them
struct StrideGrid { int groups, blocks; };
inline StrideGrid stride_grid(size_t n, int cap, int floor = 0) {
    const int groups = (int)((n + kBlock - 1) / kBlock);
    return {groups, std::max(floor, std::min(cap, groups))};
}

// a w x h film in tiles of tw x th pixels, row-major; min(kMaxBlocks, tiles) blocks stride over the tiles
struct TileGrid { int w, h, tiles_x, tiles, blocks; };
inline TileGrid tile_grid(int w, int h, int tw, int th) {
    TileGrid g{w, h, (w + tw - 1) / tw, 0, 0};
    g.tiles = g.tiles_x * ((h + th - 1) / th);
    g.blocks = std::min(g.tiles, kMaxBlocks);
    return g;
}
// tile t of the grid: its origin (x0, y0) and the pixel (x, y) of this thread, which may lie outside a ragged film
struct TilePixel { int x0, y0, x, y; };
template <int TW, int TH>
__device__ __forceinline__ TilePixel tile_pixel(const TileGrid &g, int t) {
    static_assert(TW * TH == kBlock && (TW & (TW - 1)) == 0, "one thread per tile pixel");
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;
    return {x0, y0, x0 + (int)(threadIdx.x & (TW - 1)), y0 + (int)(threadIdx.x / TW)};
}

// The film sums of an error estimate: sum of variances, sum of squared means, pixels left out of both. A kernel leaves them as
// runs 0, 1, 2 of its partials (leave_block_sum); finish_kernel (image_kernels.hip), one block on `stream`, reduces the three runs
// of nb partials into *est.
struct Estimate { double sum_var, sum_mean2, left_out; };
void launch_finish(int nb, const double *partials, Estimate *est, hipStream_t stream);
// The same for a kernel that leaves `runs` runs of nb partials: finish_runs_kernel, one block on `stream`, reduces run k into sums[k],
// each in the order above.
void launch_finish_runs(int nb, int runs, const double *partials, double *sums, hipStream_t stream);

} // namespace film
