// Lambertian-only scenes made of triangles: the lane machine built without the sphere test and the sphere shading frame
// and, where every texture is constant (cbox), without the image / checkerboard lookups (device_trace.h: PLAIN). Same
// arithmetic on every path such a scene can take; the LDS variant for cbox needs 217 instead of 254 VGPRs and spills 34
// instead of 87 SGPRs.
#include "render_device.h"
namespace gdpt {
void launch_phases_lambert_plain(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, bool lds, bool const_tex, bool whole_leaf, bool setup, hipStream_t stream) {
    // setup (default; knob no_setup_batch clears it): the LDS kernels for constant textures with the batched sample set-up (render_device.h:
    // SETUP). Their textured twins keep lane_camera: built with it they spill 3 and 5 SGPRs they did not spill before.
    if (lds && const_tex && whole_leaf && setup) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainBoth, 0, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && const_tex && setup) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainBoth, gd::kPhasesLdsLeafK, true>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else
    if (lds && const_tex && whole_leaf) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainBoth, 0>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && const_tex) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainBoth>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds && whole_leaf) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainNoSpheres, 0>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (lds) hipLaunchKernelGGL((gd::gdpt_render_phases<true, true, true, true, false, gd::kPlainNoSpheres>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else if (const_tex) hipLaunchKernelGGL((gd::gdpt_render_phases<true, false, true, true, false, gd::kPlainBoth>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
    else hipLaunchKernelGGL((gd::gdpt_render_phases<true, false, true, true, false, gd::kPlainNoSpheres>), grid, dim3(gd::kBlock), gd::phases_dynamic_lds(a), stream, sv, a);
}
} // namespace gdpt
