// {Lambertian, DisneyDiffuse} and {Lambertian, DisneyMetal}: see render_phases_general_sets.h
#include "render_phases_general_sets.h"
namespace gdpt {
void launch_phases_general_set_a(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, int lobe, hipStream_t stream) {
    if (lobe == GDPT_MAT_DISNEY_DIFFUSE) launch_phases_set<kSetDisneyDiffuse>(sv, a, grid, stream);
    else launch_phases_set<kSetDisneyMetal>(sv, a, grid, stream);
}
} // namespace gdpt
