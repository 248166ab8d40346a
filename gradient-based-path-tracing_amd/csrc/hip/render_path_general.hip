// Integrator::Path lane machine, full material switch.
#include "render_path.h"
namespace gdpt {
template <bool LDS>
static void launch_env(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool env, hipStream_t stream) {
    if (env) hipLaunchKernelGGL((gd::gdpt_path_persistent<false, LDS, true>), grid, dim3(gd::kBlock), 0, stream, sv, a);
    else hipLaunchKernelGGL((gd::gdpt_path_persistent<false, LDS, false>), grid, dim3(gd::kBlock), 0, stream, sv, a);
}
void launch_path_persistent_general(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool lds, bool env, hipStream_t stream) {
    if (lds) launch_env<true>(sv, a, grid, env, stream); else launch_env<false>(sv, a, grid, env, stream);
}
} // namespace gdpt
