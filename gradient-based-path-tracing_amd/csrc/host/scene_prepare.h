// scene_prepare.h — the host half of a scene upload: a description becomes the tables a device walks (flattened primitives, the
// trees, fp64 mip chains, the emitter tables of Integrator::Path, the environment map's 2-D table) and the traits that choose a
// render's route. prepare_scene makes no HIP call, reads no knob of its own and touches no global state (the tree builders it calls
// read theirs: host/bvh.cpp, sbvh.cpp, presplit.cpp); one PreparedScene serves any number of devices (hip/capi_device.hip:
// upload_scene, upload_scenes).
#pragma once
#include "../../../include/gdpt.h"
#include "../device_scene.h"

#include <vector>

namespace gdpt {

// What begin_launch (hip/capi_device.hip) needs to know about a scene beyond the view.
struct SceneTraits {
    int bvh_depth = 0;
    int leaf_hist[4] = {0, 0, 0, 0};   // leaves of 1..4 primitive records (gdpt_debug_leaf_histogram)
    int wide_stack_need = 0;       // stack bound of the BVH4 (LDS-resident scenes)
    int wide8_stack_need = 0;      // stack bound of the BVH8 (scenes walked from HBM)
    bool one_sided = true, lambert_only = true;
    bool has_rough = false;        // RoughPlastic / RoughDielectric present: GradPath uses the evaluator built with those lobes
    unsigned material_mask = 0;    // bit t = a material of type t is present
    int plan_take_pct = 0;         // work-item plan: share of the unassigned samples a chunk takes (0 = default 55; 40 where a refractive lobe is present)
    float bounds[6] = {0, 0, 0, 0, 0, 0};   // fp32 scene bounds (min xyz, max xyz), as get_intersection_epsilon sees them
    float pad_extent = 0;          // the extent the box padding was derived from (build_tree): what gdpt_scene_set_camera compares against
};

struct PreparedScene {
    DevSceneView view{};           // the camera and every scalar member; the table pointers stay null until upload_scene sets them
    std::vector<DevBvhNode> nodes; std::vector<DevBvh4Node> nodes4; std::vector<DevBvh8Node> nodes8; std::vector<DevBvh4QNode> nodes4q;
    std::vector<DevPrim> prims;    // BVH leaf order
    std::vector<DevTriShade> tris; std::vector<DevSphere> spheres;
    std::vector<GdptMaterial> materials; std::vector<double> light_intensity;
    std::vector<DevImage> images; std::vector<double> texels;
    std::vector<DevLight> lights; std::vector<double> light_pmf, light_cdf, light_tri_cdf, light_tri_pos, light_tri_nrm;
    std::vector<double> env_cdf_rows, env_pdf_rows, env_cdf_marginals, env_pdf_marginals;
    SceneTraits traits;
};

// presplit / sbvh: extra references per primitive the pre-split / the spatial-split build may add; a negative budget selects the
// default rule (meshes of >= 4096 triangles only). with_bvh8 / with_q4: also the quantised 8-wide / 4-wide forms of the tree; the
// caller decides (GDPT_HBM_BVH8 and GDPT_HBM_Q4 reach only the A/B translation units, never a host object).
struct PrepareOptions { double presplit = -1.0, sbvh = -1.0; bool with_bvh8 = false, with_q4 = true; };

// Everything a view derives from the camera (org, pow2_film, inv_width, ...): the one copy, for prepare_scene and for
// gdpt_scene_set_camera (hip/capi_device.hip).
void fill_camera(const GdptCamera &cam, DevCamera *out);
// The camera position's term of the extent from which build_tree derives the box padding.
float camera_extent(const GdptCamera &cam);

// Throws std::runtime_error for a description no scene can be made of.
PreparedScene prepare_scene(const GdptSceneDesc &desc, const PrepareOptions &opt);

} // namespace gdpt
