// Diagnostic build of the Lambertian lane machine with in-kernel cycle stamps (render_device.h: Stamps<true>). Selected
// only by the test-only knob "stamps" (include/gdpt_debug.h); its run time is never quoted — its segment SHARES are.
#include "render_device.h"
namespace gdpt {
void launch_phases_lambert_stamped(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool lds, bool plain, bool whole_leaf, bool setup, hipStream_t stream) {
    // setup: as in render_phases_lambert_plain.hip, so that the stamps measure what ships
    if (lds && plain && whole_leaf && setup) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true, gd::kPlainBoth, 0, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && plain && setup) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true, gd::kPlainBoth, gd::kPhasesLdsLeafK, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else
    if (lds && plain && whole_leaf) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true, gd::kPlainBoth, 0>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && plain) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true, gd::kPlainBoth>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && whole_leaf) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true, 0, 0>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else hipLaunchKernelGGL((gd::gdpt_render_phases<true, false, true, true, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
}
} // namespace gdpt
