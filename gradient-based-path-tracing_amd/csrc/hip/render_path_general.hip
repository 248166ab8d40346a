// Integrator::Path lane machine, full material switch.
#include "render_path.h"
namespace gdpt {
template <bool LDS>
static void launch_env(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, hipStream_t stream) {
    if (sv.has_envmap) hipLaunchKernelGGL((gd::gdpt_path_persistent<false, LDS, true>), grid, dim3(gd::kBlock), 0, stream, sv, a);
    else hipLaunchKernelGGL((gd::gdpt_path_persistent<false, LDS, false>), grid, dim3(gd::kBlock), 0, stream, sv, a);
}
void launch_path_persistent_general(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool lds, hipStream_t stream) {
    set_route(lds ? (sv.has_envmap ? "path_persistent/lds_general_env" : "path_persistent/lds_general")
                  : (sv.has_envmap ? "path_persistent/hbm_general_env" : "path_persistent/hbm_general"));
    if (lds) launch_env<true>(sv, a, grid, stream); else launch_env<false>(sv, a, grid, stream);
}
} // namespace gdpt
