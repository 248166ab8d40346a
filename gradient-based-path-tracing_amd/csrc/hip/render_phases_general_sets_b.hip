// {Lambertian, DisneyClearcoat} and {Lambertian, DisneySheen}: see render_phases_general_sets.h
#include "render_phases_general_sets.h"
namespace gdpt {
void launch_phases_general_set_b(const DevSceneView &sv, const gd::KernelArgs &a, dim3 grid, int lobe, hipStream_t stream) {
    if (lobe == GDPT_MAT_DISNEY_CLEARCOAT) launch_phases_set<kSetDisneyClearcoat>(sv, a, grid, stream);
    else launch_phases_set<kSetDisneySheen>(sv, a, grid, stream);
}
} // namespace gdpt
