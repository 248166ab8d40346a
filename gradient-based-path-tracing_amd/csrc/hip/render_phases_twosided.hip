// GradPath lane machine for scenes with two-sided lobes (DisneyGlass, DisneyBSDF): offsets replayed from a bounce log.
// The full material switch lives here; scenes whose materials fit one of the small sets go to the kernels built for it
// (render_phases_twosided_sets.hip; HBM scenes only — an LDS-sized scene with a Disney lobe has not been met yet).
#include "render_twosided.h"
namespace gdpt {
size_t twosided_log_bytes(unsigned blocks) { return (size_t)blocks * gd::kBlock * gd::kLogCap * sizeof(gd::BounceLog); }
// A path is logged for its first kLogCap bounce iterations. maxDepth D allows D - 1 of them. Otherwise every iteration
// from about rrDepth on passes a roulette draw that survives with probability <= 0.95, so a path outruns the log only
// after kLogCap - rrDepth such draws: the machine is kept where that takes at least kRouletteMargin of them (a
// probability below 0.95^800 = 1.6e-18 per path).
constexpr int kRouletteMargin = 800;
bool twosided_log_covers(int max_depth, int rr_depth) {
    if (max_depth >= 0 && max_depth - 1 <= gd::kLogCap) return true;
    return rr_depth <= gd::kLogCap - kRouletteMargin;
}
void launch_phases_twosided(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool lds, void *bounce_log, hipStream_t stream) {
    if (lds) hipLaunchKernelGGL((gd::gdpt_render_twosided<true>), grid, dim3(gd::kBlock), 0, stream, sv, a, (gd::BounceLog *)bounce_log);
    else hipLaunchKernelGGL((gd::gdpt_render_twosided<false>), grid, dim3(gd::kBlock), gd::hbm_dynamic_lds(a), stream, sv, a, (gd::BounceLog *)bounce_log);
}
} // namespace gdpt
