"""ctypes mirrors of the structs in include/gdpt.h (kept field-for-field in sync with the header)."""
import ctypes as C

GDPT_MAT_MAX_TEX = 12

TEX_CONSTANT, TEX_IMAGE, TEX_CHECKERBOARD = 0, 1, 2
(MAT_LAMBERTIAN, MAT_ROUGHPLASTIC, MAT_ROUGHDIELECTRIC, MAT_DISNEY_DIFFUSE, MAT_DISNEY_METAL,
 MAT_DISNEY_GLASS, MAT_DISNEY_CLEARCOAT, MAT_DISNEY_SHEEN, MAT_DISNEY_BSDF) = range(9)
SHAPE_SPHERE, SHAPE_TRIMESH = 0, 1
FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN = 0, 1, 2
INTEGRATOR_PATH, INTEGRATOR_GRADPATH, INTEGRATOR_OTHER = 5, 7, -1
RNG_TILE, RNG_SAMPLE = 0, 2
SHIFT_REFERENCE, SHIFT_RECONNECT = 0, 1
SOLVER_CG, SOLVER_DCT, SOLVER_DCT_MFMA = 0, 1, 2
SOLVER_DEFAULT = SOLVER_DCT_MFMA      # GDPT_SOLVER_DEFAULT (include/gdpt.h)


class GdptTexture(C.Structure):
    _fields_ = [("type", C.c_int32), ("image_id", C.c_int32),
                ("v0", C.c_double * 3), ("v1", C.c_double * 3),
                ("uscale", C.c_double), ("vscale", C.c_double), ("uoffset", C.c_double), ("voffset", C.c_double)]


class GdptMaterial(C.Structure):
    _fields_ = [("type", C.c_int32), ("_pad", C.c_int32), ("eta", C.c_double),
                ("tex", GdptTexture * GDPT_MAT_MAX_TEX)]


class GdptImage(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("_pad", C.c_int32),
                ("texels", C.POINTER(C.c_double))]


class GdptShape(C.Structure):
    _fields_ = [("type", C.c_int32), ("material_id", C.c_int32), ("area_light_id", C.c_int32),
                ("num_vertices", C.c_int32), ("num_triangles", C.c_int32), ("_pad", C.c_int32),
                ("center", C.c_double * 3), ("radius", C.c_double),
                ("positions", C.POINTER(C.c_double)), ("indices", C.POINTER(C.c_int32)),
                ("normals", C.POINTER(C.c_double)), ("uvs", C.POINTER(C.c_double))]


class GdptLight(C.Structure):
    _fields_ = [("shape_id", C.c_int32), ("_pad", C.c_int32), ("intensity", C.c_double * 3)]


class GdptCamera(C.Structure):
    _fields_ = [("sample_to_cam", C.c_double * 16), ("cam_to_world", C.c_double * 16),
                ("width", C.c_int32), ("height", C.c_int32), ("filter_type", C.c_int32), ("_pad", C.c_int32),
                ("filter_param", C.c_double)]


class GdptEnvmap(C.Structure):
    _fields_ = [("light_id", C.c_int32), ("image_id", C.c_int32), ("scale", C.c_double),
                ("to_world", C.c_double * 16), ("to_local", C.c_double * 16)]


class GdptSceneDesc(C.Structure):
    _fields_ = [("camera", GdptCamera),
                ("integrator", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("rr_depth", C.c_int32),
                ("num_materials", C.c_int32), ("num_shapes", C.c_int32),
                ("num_lights", C.c_int32), ("num_images", C.c_int32),
                ("materials", C.POINTER(GdptMaterial)), ("shapes", C.POINTER(GdptShape)),
                ("lights", C.POINTER(GdptLight)), ("images", C.POINTER(GdptImage)),
                ("output_filename", C.c_char * 256), ("has_envmap", C.c_int32), ("_pad", C.c_int32),
                ("envmap", GdptEnvmap)]


class GdptRenderParams(C.Structure):
    _fields_ = [("spp", C.c_int32), ("rng_scheme", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("max_depth_override", C.c_int32), ("shift_mode", C.c_int32), ("plan_rows", C.c_int32), ("reserved", C.c_int32)]


class GdptRenderStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("bounces", C.c_uint64),
                ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("nonfinite_samples", C.c_uint64),
                ("render_ms", C.c_double), ("node_bytes", C.c_uint64),
                ("wave_node_trips", C.c_uint64), ("wave_leaf_trips", C.c_uint64), ("wave_steps", C.c_uint64), ("lane_steps", C.c_uint64)]


class GdptSampleWindow(C.Structure):
    _fields_ = [("stream_spp", C.c_int32), ("first_sample", C.c_int32)]


class GdptPoissonStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("solver", C.c_int32), ("rel_residual", C.c_double), ("solve_ms", C.c_double)]


RECON_L2, RECON_L1 = 0, 1


class GdptReconParams(C.Structure):
    _fields_ = [("norm", C.c_int32), ("irls_iters", C.c_int32), ("cg_max_iters", C.c_int32), ("reserved", C.c_int32),
                ("eps_init", C.c_double), ("eps_decay", C.c_double), ("eps_floor", C.c_double), ("cg_tol", C.c_double)]


class GdptReconStats(C.Structure):
    _fields_ = [("norm", C.c_int32), ("irls_rounds", C.c_int32), ("cg_iters_total", C.c_int32), ("cg_iters_last", C.c_int32),
                ("energy_first", C.c_double), ("energy_last", C.c_double), ("rel_residual_last", C.c_double), ("solve_ms", C.c_double)]


class GdptWeightedReconParams(C.Structure):
    _fields_ = [("recon", GdptReconParams), ("conf_floor", C.c_double), ("reserved", C.c_int32 * 2)]


class GdptWeightedReconStats(C.Structure):
    _fields_ = [("recon", GdptReconStats), ("scale_data", C.c_double), ("scale_grad", C.c_double),
                ("rows_dropped", C.c_uint64), ("pixels_isolated", C.c_uint64)]


PROGRESSIVE_GRADPATH, PROGRESSIVE_PATH = 0, 1
STOP_NONE, STOP_TARGET, STOP_BUDGET, STOP_MAX_PASSES = 0, 1, 2, 3
STOP_NAMES = {STOP_NONE: "none", STOP_TARGET: "target", STOP_BUDGET: "budget", STOP_MAX_PASSES: "max_passes"}


class GdptProgressiveConfig(C.Structure):
    _fields_ = [("mode", C.c_int32), ("shift_mode", C.c_int32), ("budget_spp", C.c_int32), ("max_depth_override", C.c_int32)]


class GdptProgressiveStatus(C.Structure):
    _fields_ = [("passes", C.c_int32), ("spp_done", C.c_int32), ("budget_spp", C.c_int32), ("stop_reason", C.c_int32),
                ("error_estimate", C.c_double), ("pixels_left_out", C.c_uint64), ("fold_ms", C.c_double), ("totals", GdptRenderStats)]


class GdptReconSpreadStats(C.Structure):
    _fields_ = [("members", C.c_int32), ("radius", C.c_int32), ("error_estimate", C.c_double), ("sum_var", C.c_double),
                ("sum_sq", C.c_double), ("pixels_left_out", C.c_uint64), ("spread_ms", C.c_double)]


class GdptNlmParams(C.Structure):
    _fields_ = [("window_radius", C.c_int32), ("patch_radius", C.c_int32), ("k", C.c_double), ("alpha", C.c_double), ("epsilon", C.c_double),
                ("reserved", C.c_int32 * 2)]


class GdptNlmStats(C.Structure):
    _fields_ = [("pixels_left_out", C.c_uint64), ("sum_var_in", C.c_double), ("sum_sq_in", C.c_double), ("sum_var_out", C.c_double),
                ("sum_sq_out", C.c_double), ("error_in", C.c_double), ("error_out", C.c_double), ("filter_ms", C.c_double),
                ("window_radius", C.c_int32), ("patch_radius", C.c_int32)]


FEATURE_CHANNELS = 8             # planes of a feature render: 0-2 albedo, 3-5 shading normal, 6 depth, 7 coverage
NLM_MAX_GROUPS, NLM_MAX_CHANNELS = 4, 16


class GdptNlmFeatureGroup(C.Structure):
    _fields_ = [("first_channel", C.c_int32), ("num_channels", C.c_int32), ("tau", C.c_double)]


class GdptNlmGuide(C.Structure):
    _fields_ = [("num_channels", C.c_int32), ("num_groups", C.c_int32), ("groups", GdptNlmFeatureGroup * NLM_MAX_GROUPS),
                ("k_f", C.c_double), ("alpha_f", C.c_double), ("reserved", C.c_int32 * 2)]


NLM_JOINT_MAX = 4


class GdptNlmJointStats(C.Structure):
    _fields_ = [("guide", GdptNlmStats), ("sum_var_in", C.c_double * NLM_JOINT_MAX), ("sum_var_out", C.c_double * NLM_JOINT_MAX)]


NLM_MAX_REGRESSORS = 7


class GdptNlmRegress(C.Structure):
    _fields_ = [("num_regressors", C.c_int32), ("channel", C.c_int32 * NLM_MAX_REGRESSORS), ("scale", C.c_double * NLM_MAX_REGRESSORS),
                ("ridge", C.c_double), ("reserved", C.c_int32 * 2)]


class GdptNlmDemod(C.Structure):
    _fields_ = [("albedo_channel", C.c_int32), ("coverage_channel", C.c_int32), ("floor", C.c_double), ("reserved", C.c_int32 * 2)]


ATROUS_MAX_LEVELS = 6


class GdptAtrousParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("first_level", C.c_int32), ("k", C.c_double), ("alpha", C.c_double), ("epsilon", C.c_double),
                ("reserved", C.c_int32 * 2)]


class GdptTemporalParams(C.Structure):
    _fields_ = [("tau_z", C.c_double), ("tau_n", C.c_double), ("s_min", C.c_double), ("max_history", C.c_int32), ("reserved", C.c_int32 * 3)]


class GdptTemporalStats(C.Structure):
    _fields_ = [("pixels_left_out", C.c_uint64), ("pixels_background", C.c_uint64), ("pixels_reset", C.c_uint64),
                ("sum_history", C.c_double), ("push_ms", C.c_double)]


class GdptTemporalGradParams(C.Structure):
    _fields_ = [("j_max", C.c_double), ("cos_min", C.c_double), ("reserved", C.c_int32 * 4)]


class GdptTemporalGradStats(C.Structure):
    _fields_ = [("base", GdptTemporalStats), ("pixels_gradient_reset", C.c_uint64), ("sum_gradient_history", C.c_double)]


VAR_SMOOTH_MAX_RADIUS = 4
DENOISE_PLAIN, DENOISE_GUIDED, DENOISE_DEMOD = 0, 1, 2


class GdptVarSmoothParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("reserved", C.c_int32 * 3)]


class GdptVarSmoothStats(C.Structure):
    _fields_ = [("pixels_left_out", C.c_uint64), ("sum_var_in", C.c_double), ("sum_var_out", C.c_double), ("smooth_ms", C.c_double),
                ("radius", C.c_int32)]


SELECT_MAX_CANDIDATES, SELECT_MAX_RADIUS = 8, 8


class GdptSelectParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("reserved", C.c_int32 * 3)]


class GdptSelectStats(C.Structure):
    _fields_ = [("pixels_left_out", C.c_uint64), ("chosen", C.c_uint64 * SELECT_MAX_CANDIDATES), ("sum_e", C.c_double * SELECT_MAX_CANDIDATES),
                ("sum_mse", C.c_double), ("sum_sq_out", C.c_double), ("select_ms", C.c_double), ("radius", C.c_int32), ("num_candidates", C.c_int32)]


SELECT_MEAN, SELECT_NLM, SELECT_NLM_GUIDED, SELECT_NLM_DEMOD, SELECT_NLM_REGRESS, SELECT_ATROUS, SELECT_NLM_COLLAB = range(7)


class GdptSelectCandidate(C.Structure):
    _fields_ = [("filter", C.c_int32), ("var_smooth_radius", C.c_int32), ("nlm", C.POINTER(GdptNlmParams)), ("atrous", C.POINTER(GdptAtrousParams)),
                ("guide", C.POINTER(GdptNlmGuide)), ("demod", C.POINTER(GdptNlmDemod)), ("regress", C.POINTER(GdptNlmRegress))]


NLM_MAX_LEVELS = 4


class GdptNlmPyramidOpStats(C.Structure):
    _fields_ = [("pixels_left_out", C.c_uint64), ("cells_empty", C.c_uint64), ("op_ms", C.c_double), ("coarse_width", C.c_int32),
                ("coarse_height", C.c_int32)]


class GdptNlmPyramidStats(C.Structure):
    _fields_ = [("levels", C.c_int32), ("reserved", C.c_int32), ("width", C.c_int32 * NLM_MAX_LEVELS), ("height", C.c_int32 * NLM_MAX_LEVELS),
                ("level", GdptNlmStats * NLM_MAX_LEVELS), ("total_ms", C.c_double)]


class GdptGroupReconParams(C.Structure):
    _fields_ = [("dataCost", C.c_double), ("weighted", C.c_int32), ("map_radius", C.c_int32),
                ("recon", GdptReconParams), ("wrecon", GdptWeightedReconParams)]


GDPT_MULTI_MAX_DEVICES = 16
EXCHANGE_RCCL, EXCHANGE_PEER_COPY = 0, 1


class GdptMultiConfig(C.Structure):
    _fields_ = [("num_devices", C.c_int32), ("exchange", C.c_int32), ("devices", C.c_int32 * GDPT_MULTI_MAX_DEVICES),
                ("balance", C.c_int32), ("reserved", C.c_int32)]


class GdptMultiStats(C.Structure):
    _fields_ = [("num_devices", C.c_int32), ("exchange", C.c_int32),
                ("row_begin", C.c_int32 * GDPT_MULTI_MAX_DEVICES), ("row_end", C.c_int32 * GDPT_MULTI_MAX_DEVICES),
                ("render_ms", C.c_double * GDPT_MULTI_MAX_DEVICES), ("render_ms_max", C.c_double),
                ("exchange_ms", C.c_double), ("solve_ms", C.c_double), ("wall_ms", C.c_double)]


# include/gdpt_debug.h: gdpt_debug_prepare_scene
PREPARED_TABLES = ("nodes", "nodes4", "nodes8", "nodes4q", "prims", "tris", "spheres", "materials", "light_intensity", "images", "texels",
                   "lights", "light_pmf", "light_cdf", "light_tri_cdf", "light_tri_pos", "light_tri_nrm", "env_cdf_rows", "env_pdf_rows",
                   "env_cdf_marginals", "env_pdf_marginals")


class GdptPreparedInfo(C.Structure):
    _fields_ = [("count", C.c_int64 * len(PREPARED_TABLES)), ("digest", C.c_uint64 * len(PREPARED_TABLES)), ("isect_eps", C.c_double),
                ("bounds", C.c_float * 6), ("bvh_depth", C.c_int32), ("leaf_hist", C.c_int32 * 4), ("wide_stack_need", C.c_int32),
                ("wide8_stack_need", C.c_int32), ("one_sided", C.c_int32), ("lambert_only", C.c_int32), ("has_rough", C.c_int32),
                ("plan_take_pct", C.c_int32), ("material_mask", C.c_uint32), ("has_envmap", C.c_int32), ("env_w", C.c_int32),
                ("env_h", C.c_int32), ("all_textures_constant", C.c_int32)]


# include/gdpt_debug.h: gdpt_debug_kat_* (the per-vertex device functions on arrays of cases)
KAT_FAMILIES = ("bsdf", "texture", "filter", "primary", "shading", "light", "envmap")


class GdptKatVariant(C.Structure):
    _fields_ = [("name", C.c_char_p), ("mask", C.c_uint32), ("rough", C.c_int32), ("twosided", C.c_int32), ("inline_lambert", C.c_int32),
                ("plain", C.c_int32)]


class GdptKatVertex(C.Structure):
    _fields_ = [("gn", C.c_double * 3), ("fx", C.c_double * 3), ("fy", C.c_double * 3), ("fn", C.c_double * 3), ("uv", C.c_double * 2),
                ("uv_screen_size", C.c_double)]


class GdptKatBsdfQuery(C.Structure):
    _fields_ = [("material_id", C.c_int32), ("pad", C.c_int32), ("vertex", GdptKatVertex), ("dir_in", C.c_double * 3),
                ("dir_out2", C.c_double * 3), ("ruv", C.c_double * 2), ("rw", C.c_double)]


class GdptKatBsdfResult(C.Structure):
    _fields_ = [("sample_valid", C.c_int32), ("pad", C.c_int32), ("s_dir", C.c_double * 3), ("s_eta", C.c_double), ("s_rough", C.c_double),
                ("f", (C.c_double * 3) * 2), ("pdf", C.c_double * 2), ("fused_f", (C.c_double * 3) * 2), ("fused_pdf", C.c_double * 2)]


class GdptKatTextureQuery(C.Structure):
    _fields_ = [("material_id", C.c_int32), ("slot", C.c_int32), ("uv", C.c_double * 2), ("uv_screen_size", C.c_double)]


class GdptKatTextureResult(C.Structure):
    _fields_ = [("tex3", C.c_double * 3), ("tex1", C.c_double)]


class GdptKatFilterQuery(C.Structure):
    _fields_ = [("type", C.c_int32), ("pad", C.c_int32), ("param", C.c_double), ("u", C.c_double * 2)]


class GdptKatFilterResult(C.Structure):
    _fields_ = [("out", C.c_double * 2)]


class GdptKatPrimaryQuery(C.Structure):
    _fields_ = [("s", C.c_double * 2)]


class GdptKatPrimaryResult(C.Structure):
    _fields_ = [("org", C.c_double * 3), ("dir", C.c_double * 3)]


class GdptKatShadingQuery(C.Structure):
    _fields_ = [("is_sphere", C.c_int32), ("index", C.c_int32), ("need_uv", C.c_int32), ("pad", C.c_int32), ("st", C.c_double * 2),
                ("gn", C.c_double * 3)]


class GdptKatShadingResult(C.Structure):
    _fields_ = [("uv", C.c_double * 2), ("fx", C.c_double * 3), ("fy", C.c_double * 3), ("fn", C.c_double * 3), ("inv_uv_size", C.c_double)]


class GdptKatLightQuery(C.Structure):
    _fields_ = [("light_id", C.c_int32), ("pad", C.c_int32), ("ref", C.c_double * 3), ("uv", C.c_double * 2), ("w", C.c_double)]


class GdptKatLightResult(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("normal", C.c_double * 3), ("pdf", C.c_double)]


class GdptKatEnvmapQuery(C.Structure):
    _fields_ = [("rnd", C.c_double * 2), ("dir", C.c_double * 3)]


class GdptKatEnvmapResult(C.Structure):
    _fields_ = [("sample_uv", C.c_double * 2), ("sample_dir", C.c_double * 3), ("sample_pdf", C.c_double), ("sample_emission", C.c_double * 3),
                ("dir_uv", C.c_double * 2), ("dir_pdf", C.c_double), ("dir_emission", C.c_double * 3)]


class GdptKatTraceVariant(C.Structure):
    _fields_ = [("name", C.c_char_p)] + [(k, C.c_int32) for k in ("ww", "wide", "flat", "spheres", "spec", "leaf_k", "lds_scene", "wavefront",
                                                                  "lds_stack_levels")]


class GdptKatTraceQuery(C.Structure):
    _fields_ = [("org", C.c_double * 3), ("dir", C.c_double * 3), ("tnear", C.c_double), ("tfar", C.c_double), ("any_hit", C.c_int32),
                ("pad", C.c_int32)]


class GdptKatTraceResult(C.Structure):
    _fields_ = [("gid", C.c_int32), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("ng", C.c_float * 3)]


KAT_STRUCTS = {"bsdf": (GdptKatBsdfQuery, GdptKatBsdfResult), "texture": (GdptKatTextureQuery, GdptKatTextureResult),
               "filter": (GdptKatFilterQuery, GdptKatFilterResult), "primary": (GdptKatPrimaryQuery, GdptKatPrimaryResult),
               "shading": (GdptKatShadingQuery, GdptKatShadingResult), "light": (GdptKatLightQuery, GdptKatLightResult),
               "envmap": (GdptKatEnvmapQuery, GdptKatEnvmapResult)}
