"""gdpt_amd — MI355X-native drop-in for LaJolla's Integrator::GradPath hot path.

Thin Python mirror of the reference's operator-level entry points over the C ABI in include/gdpt.h
(libgdpt.so: host ingest in C++, kernels in HIP for gfx950). Names follow the reference:

    parse_scene(path)                     src/parsers/parse_scene.h:9
    Scene(desc) / render(...)             gradient_path_render tile loop, src/render.cpp:257-333
    fourierSolve(w, h, c, gx, gy, alpha)  src/render.cpp:172-254
    gradient_path_render(scene, ...)      src/render.cpp:257-370
    imwrite(filename, image)              src/image.cpp:135-173

There is no CPU fallback: every compute call goes to the HIP library and raises if it is missing
or no GPU is visible. (The directory name contains hyphens; import it through the top-level
`gdpt_amd.py` shim.)
"""
import ctypes as C
import os

import numpy as np

from ._ctypes_defs import *  # noqa: F401,F403
from . import _ctypes_defs as defs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgdpt.so")
_LIB = None


class GdptError(RuntimeError):
    """Raised for a non-zero status from the C ABI (the reference throws fl_exception, src/flexception.h)."""


def library_path():
    return LIB_PATH


def lib():
    """Loads libgdpt.so; fails loudly when the HIP extension has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GdptError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                            f"(make -C gradient-based-path-tracing_amd/csrc); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double)
        vp = C.c_void_p
        L.gdpt_last_error.restype = C.c_char_p
        L.gdpt_build_arch.restype = C.c_char_p
        L.gdpt_parse_scene.argtypes = [C.c_char_p, C.POINTER(C.POINTER(defs.GdptSceneDesc))]
        L.gdpt_parse_scene_film.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.POINTER(defs.GdptSceneDesc))]
        L.gdpt_free_scene_desc.argtypes = [C.POINTER(defs.GdptSceneDesc)]
        L.gdpt_scene_upload.argtypes = [C.POINTER(defs.GdptSceneDesc), C.c_int, C.POINTER(vp)]
        L.gdpt_scene_free.argtypes = [vp]
        L.gdpt_scene_info.argtypes = [vp] + [C.POINTER(C.c_int32)] * 4
        L.gdpt_render.argtypes = [vp, C.POINTER(defs.GdptRenderParams), dp, dp, dp, dp, dp, C.POINTER(defs.GdptRenderStats)]
        L.gdpt_render_device.argtypes = [vp, C.POINTER(defs.GdptRenderParams), vp, vp, vp, vp, vp, vp, C.POINTER(defs.GdptRenderStats)]
        L.gdpt_path_render.argtypes = [vp, C.POINTER(defs.GdptRenderParams), dp, C.POINTER(defs.GdptRenderStats)]
        L.gdpt_path_render_device.argtypes = [vp, C.POINTER(defs.GdptRenderParams), vp, vp, C.POINTER(defs.GdptRenderStats)]
        L.gdpt_render_window_device.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.POINTER(defs.GdptSampleWindow), vp, vp, vp, vp, vp, vp,
                                                C.POINTER(defs.GdptRenderStats)]
        L.gdpt_path_render_window_device.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.POINTER(defs.GdptSampleWindow), vp, vp,
                                                     C.POINTER(defs.GdptRenderStats)]
        L.gdpt_progressive_create.argtypes = [vp, C.POINTER(defs.GdptProgressiveConfig), vp, C.POINTER(vp)]
        L.gdpt_progressive_free.argtypes = [vp]
        L.gdpt_progressive_free.restype = None
        L.gdpt_progressive_add_pass.argtypes = [vp, C.c_int, C.POINTER(defs.GdptRenderStats)]
        L.gdpt_progressive_status.argtypes = [vp, C.POINTER(defs.GdptProgressiveStatus)]
        L.gdpt_progressive_read.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.gdpt_progressive_reconstruct.argtypes = [vp, C.c_double, C.POINTER(defs.GdptReconParams), C.c_int, vp, C.POINTER(defs.GdptReconStats)]
        L.gdpt_progressive_run.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.POINTER(defs.GdptProgressiveStatus)]
        L.gdpt_progressive_create_slice.argtypes = [vp, C.POINTER(defs.GdptProgressiveConfig), C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.gdpt_progressive_merge.argtypes = [vp, vp]
        L.gdpt_progressive_group_create.argtypes = [C.POINTER(defs.GdptSceneDesc), C.POINTER(C.c_int32), C.c_int,
                                                    C.POINTER(defs.GdptProgressiveConfig), C.POINTER(vp)]
        L.gdpt_progressive_group_free.argtypes = [vp]
        L.gdpt_progressive_group_free.restype = None
        L.gdpt_progressive_group_run.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.POINTER(defs.GdptProgressiveStatus)]
        L.gdpt_progressive_group_total.argtypes = [vp]
        L.gdpt_progressive_group_total.restype = vp
        L.gdpt_progressive_group_halves.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.gdpt_progressive_group_member_status.argtypes = [vp, C.c_int, C.POINTER(defs.GdptProgressiveStatus)]
        sst, grp = C.POINTER(defs.GdptReconSpreadStats), C.POINTER(defs.GdptGroupReconParams)
        L.gdpt_recon_spread_device.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp), dp, vp, C.c_int, vp, vp, vp, sst]
        L.gdpt_recon_spread.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp), dp, vp, C.c_int, vp, vp, sst]
        L.gdpt_progressive_group_reconstruct_error.argtypes = [vp, grp, C.c_int, vp, vp, vp, sst, C.POINTER(defs.GdptReconStats)]
        L.gdpt_progressive_group_run_recon.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, grp,
                                                       C.POINTER(defs.GdptProgressiveStatus), sst]
        nlp, nls = C.POINTER(defs.GdptNlmParams), C.POINTER(defs.GdptNlmStats)
        L.gdpt_nlm_default_params.argtypes = [nlp]
        L.gdpt_nlm_default_params.restype = None
        L.gdpt_denoise_nlm_device.argtypes = [C.c_int, C.c_int, vp, vp, nlp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm.argtypes = [C.c_int, C.c_int, vp, vp, nlp, vp, vp, nls]
        L.gdpt_progressive_denoise.argtypes = [vp, nlp, C.c_int, vp, vp, nls]
        ngp = C.POINTER(defs.GdptNlmGuide)
        L.gdpt_nlm_default_guide.argtypes = [ngp]
        L.gdpt_nlm_default_guide.restype = None
        L.gdpt_denoise_nlm_guided_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm_guided.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, vp, vp, nls]
        L.gdpt_progressive_denoise_guided.argtypes = [vp, nlp, ngp, C.c_int, C.c_int, vp, vp, vp, vp, nls]
        njs, vpp_ = C.POINTER(defs.GdptNlmJointStats), C.POINTER(vp)
        L.gdpt_denoise_nlm_joint_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vpp_, vpp_, nlp, ngp, vp, vp, vpp_, vpp_, vp, njs]
        L.gdpt_denoise_nlm_joint.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vpp_, vpp_, nlp, ngp, vp, vp, vpp_, vpp_, njs]
        L.gdpt_progressive_denoise_reconstruct.argtypes = [vp, nlp, ngp, C.c_int, C.POINTER(defs.GdptVarSmoothParams), C.c_double,
                                                           C.POINTER(defs.GdptWeightedReconParams), C.c_int, vp, vpp_, vpp_, njs,
                                                           C.POINTER(defs.GdptWeightedReconStats)]
        nrp = C.POINTER(defs.GdptNlmRegress)
        L.gdpt_nlm_default_regress.argtypes = [nrp]
        L.gdpt_nlm_default_regress.restype = None
        L.gdpt_denoise_nlm_regress_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, nrp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm_regress.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, nrp, vp, vp, nls]
        L.gdpt_progressive_denoise_regress.argtypes = [vp, nlp, ngp, nrp, C.c_int, C.c_int, vp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm_collab_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, nrp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm_collab.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, nlp, ngp, nrp, vp, vp, nls]
        L.gdpt_progressive_denoise_collab.argtypes = [vp, nlp, ngp, nrp, C.c_int, C.c_int, vp, vp, vp, nls]
        ndp = C.POINTER(defs.GdptNlmDemod)
        L.gdpt_nlm_default_demod.argtypes = [ndp]
        L.gdpt_nlm_default_demod.restype = None
        L.gdpt_denoise_nlm_demod_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, nlp, ngp, ndp, vp, vp, vp, nls]
        L.gdpt_denoise_nlm_demod.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, nlp, ngp, ndp, vp, vp, nls]
        L.gdpt_progressive_denoise_demod.argtypes = [vp, nlp, ngp, ndp, C.c_int, C.c_int, vp, vp, vp, vp, nls]
        atp = C.POINTER(defs.GdptAtrousParams)
        L.gdpt_atrous_default_params.argtypes = [atp]
        L.gdpt_atrous_default_params.restype = None
        L.gdpt_denoise_atrous_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, atp, ngp, ndp, vp, vp, vp, nls]
        L.gdpt_denoise_atrous.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, atp, ngp, ndp, vp, vp, nls]
        L.gdpt_progressive_denoise_atrous.argtypes = [vp, atp, ngp, ndp, C.c_int, C.c_int, vp, vp, vp, vp, nls]
        camp, tpp, tsp = C.POINTER(defs.GdptCamera), C.POINTER(defs.GdptTemporalParams), C.POINTER(defs.GdptTemporalStats)
        L.gdpt_scene_set_camera.argtypes = [vp, camp]
        L.gdpt_temporal_default_params.argtypes = [tpp]
        L.gdpt_temporal_default_params.restype = None
        L.gdpt_temporal_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.gdpt_temporal_free.argtypes = [vp]
        L.gdpt_temporal_free.restype = None
        L.gdpt_temporal_reset.argtypes = [vp]
        L.gdpt_temporal_world_to_sample.argtypes = [camp, dp]
        L.gdpt_temporal_push_device.argtypes = [vp, camp, vp, vp, vp, tpp, vp, vp, vp, tsp]
        L.gdpt_temporal_push.argtypes = [vp, camp, vp, vp, vp, tpp, vp, vp, vp, tsp]
        tgp, tgs = C.POINTER(defs.GdptTemporalGradParams), C.POINTER(defs.GdptTemporalGradStats)
        L.gdpt_temporal_default_grad_params.argtypes = [tgp]
        L.gdpt_temporal_default_grad_params.restype = None
        L.gdpt_temporal_push_gradients_device.argtypes = [vp, camp] + [vp] * 7 + [tpp, tgp] + [vp] * 8 + [tgs]
        L.gdpt_temporal_push_gradients.argtypes = [vp, camp] + [vp] * 7 + [tpp, tgp] + [vp] * 8 + [tgs]
        vsp, vss = C.POINTER(defs.GdptVarSmoothParams), C.POINTER(defs.GdptVarSmoothStats)
        L.gdpt_var_smooth_default_params.argtypes = [vsp]
        L.gdpt_var_smooth_default_params.restype = None
        L.gdpt_variance_smooth_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vsp, ndp, vp, vp, vss]
        L.gdpt_variance_smooth.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vsp, ndp, vp, vss]
        L.gdpt_progressive_denoise_smoothed.argtypes = [vp, C.c_int, vsp, nlp, ngp, ndp, C.c_int, C.c_int, vp, vp, vp, vp, vp, nls, vss]
        slp, sls, vpp = C.POINTER(defs.GdptSelectParams), C.POINTER(defs.GdptSelectStats), C.POINTER(vp)
        L.gdpt_select_default_params.argtypes = [slp]
        L.gdpt_select_default_params.restype = None
        L.gdpt_filter_select_device.argtypes = [C.c_int, C.c_int, C.c_int, vpp, vpp, vpp, vp, vp, vp, vp, slp, vp, vp, vp, vp, vp, sls]
        L.gdpt_progressive_group_denoise_select.argtypes = [vp, C.POINTER(defs.GdptSelectCandidate), C.c_int, slp, C.c_int, C.c_int, vp, vp, vp, vp, vp, sls, nls]
        L.gdpt_filter_select.argtypes = [C.c_int, C.c_int, C.c_int, vpp, vpp, vpp, vp, vp, vp, vp, slp, vp, vp, vp, vp, sls]
        pos, pys = C.POINTER(defs.GdptNlmPyramidOpStats), C.POINTER(defs.GdptNlmPyramidStats)
        L.gdpt_nlm_pyramid_down_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, ngp, ndp, vp, vp, vp, vp, vp, pos]
        L.gdpt_nlm_pyramid_down.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, ngp, ndp, vp, vp, vp, vp, pos]
        L.gdpt_nlm_pyramid_up_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, ngp, ndp, vp, vp, vp, vp, pos]
        L.gdpt_nlm_pyramid_up.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, ngp, ndp, vp, vp, vp, pos]
        L.gdpt_denoise_nlm_multiscale_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, nlp, ngp, ndp, vp, vp, vp, pys]
        L.gdpt_denoise_nlm_multiscale.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, nlp, ngp, ndp, vp, vp, pys]
        L.gdpt_progressive_denoise_multiscale.argtypes = [vp, C.c_int, C.c_int, vsp, nlp, ngp, ndp, C.c_int, C.c_int, vp, vp, vp, vp, pys]
        L.gdpt_features_render_device.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.POINTER(defs.GdptSampleWindow), vp, vp, vp,
                                                  C.POINTER(defs.GdptRenderStats)]
        L.gdpt_features_render.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.POINTER(defs.GdptSampleWindow), vp, vp,
                                           C.POINTER(defs.GdptRenderStats)]
        L.gdpt_assemble_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.gdpt_poisson_solve.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_double, dp]
        L.gdpt_poisson_solve_ex.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_double, dp, C.c_int, C.c_double, C.c_int,
                                            C.POINTER(defs.GdptPoissonStats)]
        L.gdpt_poisson_solve_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, vp, C.c_int, C.c_double, C.c_int,
                                                vp, C.POINTER(defs.GdptPoissonStats)]
        L.gdpt_assemble_solve_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, C.c_int, C.c_double, C.c_int,
                                                 vp, C.POINTER(defs.GdptPoissonStats)]
        L.gdpt_gradient_path_render.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.c_double, dp, dp, dp, dp, dp, dp,
                                                C.POINTER(defs.GdptRenderStats), C.POINTER(defs.GdptPoissonStats)]
        L.gdpt_reconstruct.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_double, C.POINTER(defs.GdptReconParams), dp,
                                       C.POINTER(defs.GdptReconStats)]
        L.gdpt_reconstruct_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, C.POINTER(defs.GdptReconParams), vp, vp,
                                              C.POINTER(defs.GdptReconStats)]
        L.gdpt_gradient_path_render_recon.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.c_double, C.POINTER(defs.GdptReconParams),
                                                      dp, dp, dp, dp, dp, dp, C.POINTER(defs.GdptRenderStats), C.POINTER(defs.GdptReconStats)]
        wp, wst = C.POINTER(defs.GdptWeightedReconParams), C.POINTER(defs.GdptWeightedReconStats)
        L.gdpt_reconstruct_weighted.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, C.c_double, wp, dp, C.POINTER(vp), wst]
        L.gdpt_reconstruct_weighted_device.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, wp, vp, C.POINTER(vp), vp, wst]
        L.gdpt_progressive_reconstruct_weighted.argtypes = [vp, C.c_double, wp, C.c_int, vp, C.POINTER(vp), wst]
        L.gdpt_imwrite.argtypes = [C.c_char_p, C.c_int, C.c_int, dp]
        L.gdpt_imread.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(dp)]
        L.gdpt_image_free.argtypes = [dp]
        L.gdpt_bvh_check.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int32)]
        L.gdpt_sbvh_check.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int32)]
        L.gdpt_assemble_rows_device.argtypes = [C.c_int] * 4 + [vp] * 9
        L.gdpt_band_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.gdpt_band_rows_weighted.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.gdpt_tile_row_costs.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int]
        L.gdpt_poisson_forget_stream.argtypes = [vp]
        L.gdpt_band_rows_from_row_costs.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.gdpt_multi_rebalance.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
        L.gdpt_multi_create.argtypes = [C.POINTER(defs.GdptSceneDesc), C.POINTER(defs.GdptMultiConfig), C.POINTER(vp)]
        L.gdpt_multi_free.argtypes = [vp]
        L.gdpt_multi_free.restype = None
        L.gdpt_multi_gradient_path_render.argtypes = [vp, C.POINTER(defs.GdptRenderParams), C.c_double, dp, dp, dp, dp, dp, dp,
                                                      C.POINTER(defs.GdptRenderStats), C.POINTER(defs.GdptMultiStats)]
        L.gdpt_debug_knob_set.argtypes = [C.c_char_p, C.c_double]
        L.gdpt_debug_knobs_reset.restype = None
        L.gdpt_debug_chunk_plan.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.POINTER(C.c_int32), C.c_int]
        L.gdpt_debug_get_stamps.argtypes = [C.POINTER(C.c_double)]
        L.gdpt_debug_get_stamps.restype = None
        L.gdpt_debug_last_route.restype = C.c_char_p
        L.gdpt_debug_last_dct_shape.restype = C.c_char_p
        L.gdpt_debug_overlapped_launches.argtypes = [vp]
        L.gdpt_debug_overlapped_launches.restype = C.c_longlong
        L.gdpt_debug_leaf_histogram.argtypes = [vp, C.POINTER(C.c_int32)]
        L.gdpt_debug_route_names.argtypes = [C.POINTER(C.c_char_p), C.c_int]
        L.gdpt_debug_image_grid.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.gdpt_debug_prepare_scene.argtypes = [C.POINTER(defs.GdptSceneDesc), C.POINTER(defs.GdptPreparedInfo), dp, dp, C.c_int]
        L.gdpt_debug_kat_variants.argtypes = [C.c_char_p, C.POINTER(defs.GdptKatVariant), C.c_int]
        for family, (query, result) in defs.KAT_STRUCTS.items():
            getattr(L, "gdpt_debug_kat_" + family).argtypes = [vp, C.c_int, C.c_int, C.POINTER(query), C.POINTER(result)]
        L.gdpt_debug_kat_trace_variants.argtypes = [C.POINTER(defs.GdptKatTraceVariant), C.c_int]
        L.gdpt_debug_kat_trace.argtypes = [vp, C.c_int, C.c_int, C.POINTER(defs.GdptKatTraceQuery), C.POINTER(defs.GdptKatTraceResult)]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise GdptError(lib().gdpt_last_error().decode("utf-8", "replace"))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class SceneDesc:
    """Host-side flattened scene (owner of a GdptSceneDesc*), the result of parse_scene()."""

    def __init__(self, ptr):
        self.ptr = ptr

    @property
    def desc(self):
        return self.ptr.contents

    @property
    def width(self):
        return self.ptr.contents.camera.width

    @property
    def height(self):
        return self.ptr.contents.camera.height

    def close(self):
        if self.ptr:
            lib().gdpt_free_scene_desc(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_scene(filename, film=(0, 0)):
    """Mitsuba-0.x XML subset -> SceneDesc (reference: parse_scene, src/parsers/parse_scene.cpp:1615-1630).
    `film` = (width, height) replaces the <film> extent of the file (0 keeps it)."""
    p = C.POINTER(defs.GdptSceneDesc)()
    _check(lib().gdpt_parse_scene_film(os.fsencode(filename), int(film[0]), int(film[1]), C.byref(p)))
    return SceneDesc(p)


def _params(spp, rng_scheme, rows, max_depth_override=0, shift=0, plan_rows=0):
    p = defs.GdptRenderParams()
    p.shift_mode = int(shift)
    p.plan_rows = int(plan_rows)
    p.spp, p.rng_scheme = int(spp), int(rng_scheme)
    p.row_begin, p.row_end = int(rows[0]), int(rows[1])
    p.max_depth_override = int(max_depth_override)
    return p


class Scene:
    """Device-resident scene: own BVH2 + fp32 traversal records + fp64 shading tables in HBM
    (replaces Scene::Scene's Embree build, src/scene.cpp:4-53)."""

    def __init__(self, scene_desc, device=0):
        self.desc = scene_desc
        self.width, self.height = scene_desc.width, scene_desc.height
        h = C.c_void_p()
        _check(lib().gdpt_scene_upload(scene_desc.ptr, int(device), C.byref(h)))
        self.handle = h

    def info(self):
        v = [C.c_int32() for _ in range(4)]
        _check(lib().gdpt_scene_info(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("num_nodes", "num_tris", "num_spheres", "bvh_depth"), [x.value for x in v]))

    def render(self, spp=0, rng_scheme=defs.RNG_SAMPLE, rows=(0, 0), shift=defs.SHIFT_REFERENCE, plan_rows=0):
        """Five-buffer render to host arrays (HxWx3 float64). Returns (buffers, GdptRenderStats).
        `shift`: SHIFT_REFERENCE (the reference's offsets) or SHIFT_RECONNECT (include/gdpt.h).
        `plan_rows`: GdptRenderParams.plan_rows (0 = work items cut for the whole film)."""
        shape = (self.height, self.width, 3)
        bufs = {k: np.zeros(shape, dtype=np.float64) for k in ("img", "cx0", "cy0", "cx1", "cy1")}
        st = defs.GdptRenderStats()
        p = _params(spp, rng_scheme, rows, shift=shift, plan_rows=plan_rows)
        _check(lib().gdpt_render(self.handle, C.byref(p), _dp(bufs["img"]), _dp(bufs["cx0"]), _dp(bufs["cy0"]),
                                 _dp(bufs["cx1"]), _dp(bufs["cy1"]), C.byref(st)))
        return bufs, st

    def render_device(self, ptrs, spp=0, rng_scheme=defs.RNG_SAMPLE, rows=(0, 0), stream=None, want_stats=False,
                      shift=defs.SHIFT_REFERENCE, plan_rows=0, window=None):
        """Five-buffer render into device memory; `ptrs` = 5 device addresses (e.g. torch tensor.data_ptr()).
        `window` = (stream_spp, first_sample): the spp samples are streams [first_sample, first_sample + spp) of every pixel's
        block of stream_spp streams (GdptSampleWindow, gdpt_render_window_device)."""
        st = defs.GdptRenderStats() if want_stats else None
        p = _params(spp, rng_scheme, rows, shift=shift, plan_rows=plan_rows)
        tail = [C.c_void_p(int(x)) for x in ptrs] + [C.c_void_p(int(stream) if stream else 0), C.byref(st) if st is not None else None]
        if window is None:
            _check(lib().gdpt_render_device(self.handle, C.byref(p), *tail))
        else:
            win = defs.GdptSampleWindow(int(window[0]), int(window[1]))
            _check(lib().gdpt_render_window_device(self.handle, C.byref(p), C.byref(win), *tail))
        return st

    def path_render(self, spp=0, rng_scheme=defs.RNG_SAMPLE, rows=(0, 0), want_counts=False):
        """Integrator::Path (path_render, src/render.cpp:74-117): HxWx3 float64 image + GdptRenderStats."""
        img = np.zeros((self.height, self.width, 3), dtype=np.float64)
        st = defs.GdptRenderStats()
        if want_counts:
            st.nodes_visited = 2 ** 64 - 1
        p = _params(spp, rng_scheme, rows)
        _check(lib().gdpt_path_render(self.handle, C.byref(p), _dp(img), C.byref(st)))
        return img, st

    def path_render_device(self, ptr, spp=0, rng_scheme=defs.RNG_SAMPLE, rows=(0, 0), stream=None, window=None, want_stats=False):
        """`window` as in render_device (gdpt_path_render_window_device)."""
        st = defs.GdptRenderStats() if want_stats else None
        p = _params(spp, rng_scheme, rows)
        tail = [C.c_void_p(int(ptr)), C.c_void_p(int(stream) if stream else 0), C.byref(st) if st is not None else None]
        if window is None:
            _check(lib().gdpt_path_render_device(self.handle, C.byref(p), *tail))
        else:
            win = defs.GdptSampleWindow(int(window[0]), int(window[1]))
            _check(lib().gdpt_path_render_window_device(self.handle, C.byref(p), C.byref(win), *tail))
        return st

    def gradient_path_render(self, spp=0, rng_scheme=defs.RNG_SAMPLE, alpha=0.04, return_buffers=False,
                             shift=defs.SHIFT_REFERENCE, plan_rows=0, reconstruct=None):
        """Whole Integrator::GradPath: render + assembly + screened-Poisson solve (src/render.cpp:257-370).
        `reconstruct`: None = that solve; recon_params(...) = gdpt_gradient_path_render_recon (the last element returned with
        return_buffers is then a GdptReconStats)."""
        shape = (self.height, self.width, 3)
        out = np.zeros(shape, dtype=np.float64)
        bufs = {k: np.zeros(shape, dtype=np.float64) for k in ("img", "cx0", "cy0", "cx1", "cy1")}
        rs = defs.GdptRenderStats()
        p = _params(spp, rng_scheme, (0, 0), shift=shift, plan_rows=plan_rows)
        raw = [_dp(bufs[k]) for k in ("img", "cx0", "cy0", "cx1", "cy1")]
        if reconstruct is None:
            ps = defs.GdptPoissonStats()
            _check(lib().gdpt_gradient_path_render(self.handle, C.byref(p), float(alpha), _dp(out), *raw, C.byref(rs), C.byref(ps)))
        else:
            ps = defs.GdptReconStats()
            _check(lib().gdpt_gradient_path_render_recon(self.handle, C.byref(p), float(alpha), C.byref(reconstruct), _dp(out), *raw,
                                                         C.byref(rs), C.byref(ps)))
        return (out, bufs, rs, ps) if return_buffers else out

    def features(self, spp, window=None, rows=None, out=None, want_stats=False):
        """First-hit feature buffers of the film (gdpt_features_render): two (8, H, W) float64 arrays, the per-pixel means over `spp`
        samples and the variances of those means; planes 0-2 albedo, 3-5 shading normal, 6 depth, 7 coverage. The camera rays are the
        render's own: `window` = (stream_spp, first_sample) as in render_device. `rows` = (begin, end) renders that band alone and
        leaves the other rows of `out` = (mean, var) as they are (zeros without `out`). With `want_stats` the GdptRenderStats follow."""
        shape = (defs.FEATURE_CHANNELS, self.height, self.width)
        if out is None:
            mean, var = np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.float64)
        else:
            mean, var = out
            if any(a.shape != shape or a.dtype != np.float64 or not a.flags.c_contiguous for a in (mean, var)):
                raise GdptError("features: out must be two C-contiguous float64 arrays of shape (8, H, W)")
        st = defs.GdptRenderStats()
        p = _params(spp, defs.RNG_SAMPLE, rows if rows is not None else (0, 0))
        win = defs.GdptSampleWindow(int(window[0]), int(window[1])) if window is not None else None
        _check(lib().gdpt_features_render(self.handle, C.byref(p), C.byref(win) if win is not None else None, C.c_void_p(mean.ctypes.data),
                                          C.c_void_p(var.ctypes.data), C.byref(st)))
        return (mean, var, st) if want_stats else (mean, var)

    def features_device(self, mean_ptr, var_ptr, spp, window=None, rows=None, stream=None, want_stats=False):
        """features() into device memory (gdpt_features_render_device): two device addresses of 8 H W doubles each. Enqueue-only
        unless `want_stats`."""
        st = defs.GdptRenderStats() if want_stats else None
        p = _params(spp, defs.RNG_SAMPLE, rows if rows is not None else (0, 0))
        win = defs.GdptSampleWindow(int(window[0]), int(window[1])) if window is not None else None
        _check(lib().gdpt_features_render_device(self.handle, C.byref(p), C.byref(win) if win is not None else None,
                                                 C.c_void_p(int(mean_ptr)) if mean_ptr else None, C.c_void_p(int(var_ptr)) if var_ptr else None,
                                                 C.c_void_p(int(stream) if stream else 0), C.byref(st) if st is not None else None))
        return st

    def set_camera(self, camera):
        """A new camera on the uploaded scene (gdpt_scene_set_camera): a GdptCamera with the uploaded film and pixel filter, whose
        position stays inside the extent the scene was uploaded with. Renders enqueued before the call keep the old camera; every
        later render returns the bits of a fresh upload with this camera. The description (`self.desc`) is not changed."""
        _check(lib().gdpt_scene_set_camera(self.handle, C.byref(camera) if camera is not None else None))

    def tile_row_costs(self, spp=1):
        """Rays of a pilot render of every 16-pixel tile row (gdpt_tile_row_costs): what sharding.bands_weighted balances by."""
        T = (self.height + 15) // 16
        buf = (C.c_double * T)()
        _check(lib().gdpt_tile_row_costs(self.handle, int(spp), buf, T))
        return [float(x) for x in buf]

    def leaf_histogram(self):
        """Leaves of the uploaded tree by size: [leaves of 1, 2, 3, 4 primitive records] (include/gdpt_debug.h)."""
        h = (C.c_int32 * 4)()
        _check(lib().gdpt_debug_leaf_histogram(self.handle, h))
        return list(h)

    def overlapped_launches(self):
        """Renders so far whose kernel ran on one of the handle's own render streams (include/gdpt_debug.h)."""
        return int(lib().gdpt_debug_overlapped_launches(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            lib().gdpt_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BUFFERS = ("img", "cx0", "cy0", "cx1", "cy1")


class Progressive:
    """A progressive render session on the device (include/gdpt.h, gdpt_progressive_*): passes over disjoint sample windows of
    every pixel's block of `budget_spp` PCG streams, folded into running means and per-pixel variances of the mean.
    `path=True`: Integrator::Path (the img plane alone). `stream`: a hipStream_t address carrying all of the session's work.
    `slice=(first, n)`: the session draws its passes from streams [first, first + n) of the block alone (gdpt_progressive_create_slice;
    n = 0: an accumulator that only receives merges); sessions over disjoint slices combine exactly with merge()."""

    def __init__(self, scene, budget_spp, shift=defs.SHIFT_REFERENCE, path=False, stream=None, max_depth_override=0, slice=None):
        self.scene = scene                       # keeps the scene handle alive
        self._owned = True
        self.path = bool(path)
        self.names = BUFFERS[:1] if self.path else BUFFERS
        self.shape = (scene.height, scene.width, 3)
        cfg = defs.GdptProgressiveConfig(defs.PROGRESSIVE_PATH if self.path else defs.PROGRESSIVE_GRADPATH, int(shift), int(budget_spp),
                                         int(max_depth_override))
        h = C.c_void_p()
        if slice is None:
            _check(lib().gdpt_progressive_create(scene.handle, C.byref(cfg), C.c_void_p(int(stream) if stream else 0), C.byref(h)))
        else:
            _check(lib().gdpt_progressive_create_slice(scene.handle, C.byref(cfg), int(slice[0]), int(slice[1]),
                                                       C.c_void_p(int(stream) if stream else 0), C.byref(h)))
        self.handle = h

    @classmethod
    def _view(cls, owner, handle, shape, path):
        """A session handle owned by someone else (a ProgressiveGroup's total): every call works, close() does not free."""
        self = cls.__new__(cls)
        self.scene, self._owned = owner, False   # keeps the owner alive
        self.path = bool(path)
        self.names = BUFFERS[:1] if self.path else BUFFERS
        self.shape = shape
        self.handle = C.c_void_p(handle)
        return self

    def merge(self, other):
        """Takes in `other`'s statistics (gdpt_progressive_merge): afterwards this session is the one that folded the passes of both.
        `other` is unchanged. The sessions must hold disjoint samples of one stream block. Returns status()."""
        _check(lib().gdpt_progressive_merge(self.handle, other.handle))
        return self.status()

    def add_pass(self, spp):
        """Renders and folds in the next `spp` samples of every pixel; returns the pass's GdptRenderStats."""
        st = defs.GdptRenderStats()
        _check(lib().gdpt_progressive_add_pass(self.handle, int(spp), C.byref(st)))
        return st

    @staticmethod
    def _status_dict(st):
        return dict(passes=st.passes, spp=st.spp_done, budget_spp=st.budget_spp, error=st.error_estimate,
                    pixels_left_out=st.pixels_left_out, fold_ms=st.fold_ms, stop_reason=defs.STOP_NAMES[st.stop_reason], totals=st.totals)

    def status(self):
        """dict: passes, spp (so far), budget_spp, error (estimated relative RMSE of the primal mean; NaN before 2 passes),
        pixels_left_out (of the estimate), fold_ms (device time of the last fold), stop_reason (of the last run), totals (GdptRenderStats summed over the passes)."""
        st = defs.GdptProgressiveStatus()
        _check(lib().gdpt_progressive_status(self.handle, C.byref(st)))
        return self._status_dict(st)

    def read(self, variances=True):
        """Host copies, HxWx3 float64: (means, vars, assembled_vars). means / vars: dicts over the session's buffers (running mean,
        variance of the mean); assembled_vars: dict of the variances of the assembled c, cx, cy (GradPath). With `variances=False`, and before the
        second pass (no variance is defined yet), the means alone: (means, None, None)."""
        variances = bool(variances) and self.status()["passes"] >= 2
        means = {k: np.empty(self.shape, dtype=np.float64) for k in self.names}
        vars_ = {k: np.empty(self.shape, dtype=np.float64) for k in self.names} if variances else None
        asm = {k: np.empty(self.shape, dtype=np.float64) for k in ("c", "cx", "cy")} if variances and not self.path else None

        def table(d, keys):
            arr = (C.c_void_p * len(keys))()
            for i, k in enumerate(keys):
                arr[i] = d[k].ctypes.data if d is not None and k in d else None
            return arr
        _check(lib().gdpt_progressive_read(self.handle, 0, table(means, BUFFERS), table(vars_, BUFFERS), table(asm, ("c", "cx", "cy"))))
        return means, vars_, asm

    def read_device(self, mean_ptrs=None, var_ptrs=None, assembled_var_ptrs=None):
        """read() into device memory: lists of 5 / 5 / 3 device addresses (None or 0 entries are skipped)."""
        def table(ptrs, n):
            arr = (C.c_void_p * n)()
            for i in range(n):
                arr[i] = int(ptrs[i]) if ptrs is not None and i < len(ptrs) and ptrs[i] else None
            return arr
        _check(lib().gdpt_progressive_read(self.handle, 1, table(mean_ptrs, 5), table(var_ptrs, 5), table(assembled_var_ptrs, 3)))

    def reconstruct(self, alpha=0.04, norm=defs.RECON_L2, out_ptr=None, **params):
        """The reconstruction of the running means (a preview after any pass): RECON_L2 = fourierSolve, RECON_L1 = IRLS (`params`: the
        keywords of recon_params). Returns (HxWx3 image, GdptReconStats), or the stats alone when `out_ptr` names device memory."""
        p, st = recon_params(norm, **params), defs.GdptReconStats()
        if out_ptr is not None:
            _check(lib().gdpt_progressive_reconstruct(self.handle, float(alpha), C.byref(p), 1, C.c_void_p(int(out_ptr)), C.byref(st)))
            return st
        out = np.empty(self.shape, dtype=np.float64)
        _check(lib().gdpt_progressive_reconstruct(self.handle, float(alpha), C.byref(p), 0, C.c_void_p(out.ctypes.data), C.byref(st)))
        return out, st

    def reconstruct_weighted(self, alpha=0.04, norm=defs.RECON_L2, conf_floor=0.0, confidence=False, out_ptr=None, confidence_ptrs=None,
                             **params):
        """The variance-weighted reconstruction of the running means on the session's assembled variances
        (gdpt_progressive_reconstruct_weighted; from 2 passes on, GradPath): RECON_L2 = generalised least squares, RECON_L1 = its
        IRLS form (`params`: the keywords of recon_params). Returns (HxWx3 image, GdptWeightedReconStats), with `confidence=True`
        (image, HxWx3 confidences of the data, x-edge and y-edge rows, stats); with `out_ptr` (and `confidence_ptrs`, 3 device
        addresses) everything stays in device memory and the stats alone are returned."""
        p, st = weighted_recon_params(norm, conf_floor, **params), defs.GdptWeightedReconStats()
        if out_ptr is not None:
            _check(lib().gdpt_progressive_reconstruct_weighted(self.handle, float(alpha), C.byref(p), 1, C.c_void_p(int(out_ptr)),
                                                               _ptr_table(confidence_ptrs), C.byref(st)))
            return st
        out = np.empty(self.shape, dtype=np.float64)
        planes = [np.empty(self.shape[:2], dtype=np.float64) for _ in range(3)] if confidence else None
        _check(lib().gdpt_progressive_reconstruct_weighted(self.handle, float(alpha), C.byref(p), 0, C.c_void_p(out.ctypes.data),
                                                           _ptr_table([a.ctypes.data for a in planes] if confidence else None), C.byref(st)))
        return (out, np.stack(planes, axis=2), st) if confidence else (out, st)

    def denoise(self, out_ptr=None, var_out_ptr=None, **params):
        """The non-local-means filter on buffer 0 (gdpt_progressive_denoise; from 2 passes on): the running mean of the image of a Path
        session, or of the primal of a GradPath session, with the variance of that mean (`params`: the keywords of nlm_params).
        Returns (HxWx3 filtered mean, HxWx3 variance of it, GdptNlmStats); with `out_ptr` (and `var_out_ptr`) everything stays in
        device memory and the stats alone are returned."""
        p, st = nlm_params(**params), defs.GdptNlmStats()
        if out_ptr is not None:
            _check(lib().gdpt_progressive_denoise(self.handle, C.byref(p), 1, C.c_void_p(int(out_ptr)),
                                                  C.c_void_p(int(var_out_ptr)) if var_out_ptr else None, C.byref(st)))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        _check(lib().gdpt_progressive_denoise(self.handle, C.byref(p), 0, C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data), C.byref(st)))
        return out, var_out, st

    def denoise_reconstruct(self, alpha=0.04, guide=None, feature_spp=0, var_smooth_radius=None, weighted=None, conf_floor=0.0, recon=None,
                            filtered=False, out_ptr=None, filtered_ptrs=None, filtered_var_ptrs=None, **params):
        """The joint filter and the reconstruction of what it wrote (gdpt_progressive_denoise_reconstruct; GradPath, from 2 passes on):
        the non-local-means weights of the assembled primal c (with `guide`, a GdptNlmGuide, capped by `feature_spp` samples of the
        session's first-hit features; None = unguided) filter c, cx, cy and their variances alike, and the filtered triple is
        reconstructed. `var_smooth_radius`: None = the primal's variance as estimated, else it is smoothed over that radius first (the
        weights' variance only). `weighted`: None = the L2 reconstruction; RECON_L2 / RECON_L1 = reconstruct_weighted's two forms on
        the FILTERED variances, with `conf_floor` and `recon` (a dict of the keywords of recon_params). `params`: the keywords of
        nlm_params. Returns (HxWx3 image, GdptNlmJointStats, GdptWeightedReconStats), with `filtered=True` (image, [c, cx, cy]
        filtered, [their variances], the two stats); with `out_ptr` (and `filtered_ptrs`, `filtered_var_ptrs`: 3 device addresses
        each) everything stays in device memory and the two stats alone are returned."""
        p, st, rst = nlm_params(**params), defs.GdptNlmJointStats(), defs.GdptWeightedReconStats()
        g = C.byref(guide) if guide is not None else None
        sp = C.byref(var_smooth_params(var_smooth_radius)) if var_smooth_radius is not None else None
        wp = C.byref(weighted_recon_params(weighted, conf_floor, **(recon or {}))) if weighted is not None else None
        call = lambda *tail: _check(lib().gdpt_progressive_denoise_reconstruct(self.handle, C.byref(p), g, int(feature_spp), sp, float(alpha), wp,      # noqa: E731
                                                                               *tail, C.byref(st), C.byref(rst)))
        if out_ptr is not None:
            call(1, C.c_void_p(int(out_ptr)), _ptr_table(filtered_ptrs), _ptr_table(filtered_var_ptrs))
            return st, rst
        out = np.empty(self.shape, dtype=np.float64)
        fl = [np.empty(self.shape, dtype=np.float64) for _ in range(3)] if filtered else None
        fv = [np.empty(self.shape, dtype=np.float64) for _ in range(3)] if filtered else None
        call(0, C.c_void_p(out.ctypes.data), _ptr_table([a.ctypes.data for a in fl] if filtered else None),
             _ptr_table([a.ctypes.data for a in fv] if filtered else None))
        return (out, fl, fv, st, rst) if filtered else (out, st, rst)

    def denoise_guided(self, feature_spp, guide=None, features=False, out_ptr=None, var_out_ptr=None, features_ptrs=None, **params):
        """The feature-guided non-local-means filter on buffer 0 (gdpt_progressive_denoise_guided; from 2 passes on): the session
        renders `feature_spp` samples of first-hit features along the camera rays of its own first samples and lets them cap the
        colour weights. `guide`: a GdptNlmGuide (nlm_guide(...)), None = the library's default; `params`: the keywords of nlm_params.
        Returns (HxWx3 filtered mean, HxWx3 variance of it, GdptNlmStats), with `features=True` also the two (8, H, W) feature arrays
        before the stats; with `out_ptr` (and `var_out_ptr`, `features_ptrs` = 2 device addresses) everything stays in device memory
        and the stats alone are returned."""
        p, st = nlm_params(**params), defs.GdptNlmStats()
        g = guide if guide is not None else nlm_guide()
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            _check(lib().gdpt_progressive_denoise_guided(self.handle, C.byref(p), C.byref(g), int(feature_spp), 1, opt(out_ptr), opt(var_out_ptr),
                                                         opt(fp[0]), opt(fp[1]), C.byref(st)))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        _check(lib().gdpt_progressive_denoise_guided(self.handle, C.byref(p), C.byref(g), int(feature_spp), 0, C.c_void_p(out.ctypes.data),
                                                     C.c_void_p(var_out.ctypes.data), C.c_void_p(fm.ctypes.data) if features else None,
                                                     C.c_void_p(fv.ctypes.data) if features else None, C.byref(st)))
        return (out, var_out, fm, fv, st) if features else (out, var_out, st)

    def denoise_regress(self, feature_spp, guide=None, regress=None, features=False, out_ptr=None, var_out_ptr=None, features_ptrs=None, **params):
        """The first-order feature regression on buffer 0 (gdpt_progressive_denoise_regress; from 2 passes on): the session renders
        `feature_spp` samples of first-hit features as denoise_guided does, and fits the colour linearly on the regressor planes under
        the guided filter's weights. `guide`: a GdptNlmGuide (nlm_guide(...)), `regress`: a GdptNlmRegress (nlm_regress(...)), None =
        the library's defaults; `params`: the keywords of nlm_params. Returns and device-memory form as denoise_guided."""
        p, st = nlm_params(**params), defs.GdptNlmStats()
        g = guide if guide is not None else nlm_guide()
        rg = regress if regress is not None else nlm_regress()
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            _check(lib().gdpt_progressive_denoise_regress(self.handle, C.byref(p), C.byref(g), C.byref(rg), int(feature_spp), 1, opt(out_ptr),
                                                          opt(var_out_ptr), opt(fp[0]), opt(fp[1]), C.byref(st)))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        _check(lib().gdpt_progressive_denoise_regress(self.handle, C.byref(p), C.byref(g), C.byref(rg), int(feature_spp), 0,
                                                      C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data),
                                                      C.c_void_p(fm.ctypes.data) if features else None,
                                                      C.c_void_p(fv.ctypes.data) if features else None, C.byref(st)))
        return (out, var_out, fm, fv, st) if features else (out, var_out, st)

    def denoise_collab(self, feature_spp, guide=None, regress=None, features=False, out_ptr=None, features_ptrs=None, **params):
        """The collaborative form of denoise_regress on buffer 0 (gdpt_progressive_denoise_collab; from 2 passes on): every pixel takes
        the weighted average of all fits whose windows cover it. Arguments as denoise_regress, without a variance of the result:
        returns (HxWx3 image, GdptNlmStats), with `features=True` the two (8, H, W) feature arrays before the stats; with `out_ptr`
        (and `features_ptrs`) everything stays in device memory and the stats alone are returned."""
        p, st = nlm_params(**params), defs.GdptNlmStats()
        g = guide if guide is not None else nlm_guide()
        rg = regress if regress is not None else nlm_regress()
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            _check(lib().gdpt_progressive_denoise_collab(self.handle, C.byref(p), C.byref(g), C.byref(rg), int(feature_spp), 1, opt(out_ptr),
                                                         opt(fp[0]), opt(fp[1]), C.byref(st)))
            return st
        out = np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        _check(lib().gdpt_progressive_denoise_collab(self.handle, C.byref(p), C.byref(g), C.byref(rg), int(feature_spp), 0,
                                                     C.c_void_p(out.ctypes.data), C.c_void_p(fm.ctypes.data) if features else None,
                                                     C.c_void_p(fv.ctypes.data) if features else None, C.byref(st)))
        return (out, fm, fv, st) if features else (out, st)

    def denoise_demod(self, feature_spp, guide=None, demod=None, features=False, out_ptr=None, var_out_ptr=None, features_ptrs=None, **params):
        """The albedo-demodulated non-local-means filter on buffer 0 (gdpt_progressive_denoise_demod; from 2 passes on): the session
        renders `feature_spp` samples of first-hit features along the camera rays of its own first samples, divides its mean by their
        effective albedo, filters the quotient and multiplies the albedo back. `guide`: a GdptNlmGuide (nlm_guide(...)) over the 8
        planes, None = NO feature term (not the default guide); `demod`: a GdptNlmDemod (nlm_demod(...)), None = the library's
        default; `params`: the keywords of nlm_params. Returns and device-memory form as denoise_guided."""
        p, st = nlm_params(**params), defs.GdptNlmStats()
        g = C.byref(guide) if guide is not None else None
        d = demod if demod is not None else nlm_demod()
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            _check(lib().gdpt_progressive_denoise_demod(self.handle, C.byref(p), g, C.byref(d), int(feature_spp), 1, opt(out_ptr), opt(var_out_ptr),
                                                        opt(fp[0]), opt(fp[1]), C.byref(st)))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        _check(lib().gdpt_progressive_denoise_demod(self.handle, C.byref(p), g, C.byref(d), int(feature_spp), 0, C.c_void_p(out.ctypes.data),
                                                    C.c_void_p(var_out.ctypes.data), C.c_void_p(fm.ctypes.data) if features else None,
                                                    C.c_void_p(fv.ctypes.data) if features else None, C.byref(st)))
        return (out, var_out, fm, fv, st) if features else (out, var_out, st)

    def denoise_atrous(self, feature_spp=0, guide=None, demod=None, features=False, out_ptr=None, var_out_ptr=None, features_ptrs=None, **params):
        """The edge-avoiding a-trous wavelet filter on buffer 0 (gdpt_progressive_denoise_atrous; from 2 passes on), the cheap filter:
        `guide`: a GdptNlmGuide (nlm_guide(...)) over the 8 planes, None = NO feature term; `demod`: a GdptNlmDemod (nlm_demod(...)),
        None = NO demodulation; with either the session renders `feature_spp` samples of first-hit features as denoise_guided does,
        with neither it renders none and `feature_spp` is ignored (`features` must be False then). `params`: the keywords of
        atrous_params. Returns and device-memory form as denoise_guided."""
        p, st = atrous_params(**params), defs.GdptNlmStats()
        g = C.byref(guide) if guide is not None else None
        d = C.byref(demod) if demod is not None else None
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            _check(lib().gdpt_progressive_denoise_atrous(self.handle, C.byref(p), g, d, int(feature_spp), 1, opt(out_ptr), opt(var_out_ptr),
                                                         opt(fp[0]), opt(fp[1]), C.byref(st)))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        _check(lib().gdpt_progressive_denoise_atrous(self.handle, C.byref(p), g, d, int(feature_spp), 0, C.c_void_p(out.ctypes.data),
                                                     C.c_void_p(var_out.ctypes.data), C.c_void_p(fm.ctypes.data) if features else None,
                                                     C.c_void_p(fv.ctypes.data) if features else None, C.byref(st)))
        return (out, var_out, fm, fv, st) if features else (out, var_out, st)

    def denoise_smoothed(self, kind="plain", radius=None, feature_spp=0, guide=None, demod=None, features=False, out_ptr=None, var_out_ptr=None,
                         smoothed_var_ptr=None, features_ptrs=None, **params):
        """One of the three filters above on the SMOOTHED variance of buffer 0 (gdpt_progressive_denoise_smoothed; from 2 passes on):
        the session replaces its variance with the box mean over a (2 radius + 1)^2 window (variance_smooth; `radius` None = the
        library's default, 2) and runs denoise (`kind` "plain"), denoise_guided ("guided") or denoise_demod ("demod") on it; for
        "demod" the mean is taken in the albedo-normalised domain, with the filter's own `demod` block. `guide`, `demod`,
        `feature_spp`, `params` as those three take them ("plain" takes none of the first three). Returns (HxWx3 filtered mean, HxWx3
        variance of it, HxWx3 smoothed variance, GdptNlmStats, GdptVarSmoothStats), with `features=True` the two (8, H, W) feature
        arrays before the stats; with `out_ptr` (and `var_out_ptr`, `smoothed_var_ptr`, `features_ptrs` = 2 device addresses)
        everything stays in device memory and the two stats alone are returned. The variance and the stats of the filter are those
        of the smoothed variance."""
        kinds = {"plain": defs.DENOISE_PLAIN, "guided": defs.DENOISE_GUIDED, "demod": defs.DENOISE_DEMOD}
        if kind not in kinds:
            raise GdptError('denoise_smoothed: kind must be "plain", "guided" or "demod"')
        sp, p, st, sst = var_smooth_params(radius), nlm_params(**params), defs.GdptNlmStats(), defs.GdptVarSmoothStats()
        g = C.byref(guide) if guide is not None else None
        d = C.byref(demod) if demod is not None else None
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        call = lambda *tail: _check(lib().gdpt_progressive_denoise_smoothed(self.handle, kinds[kind], C.byref(sp), C.byref(p), g, d,      # noqa: E731
                                                                            int(feature_spp), *tail, C.byref(st), C.byref(sst)))
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            call(1, opt(out_ptr), opt(var_out_ptr), opt(smoothed_var_ptr), opt(fp[0]), opt(fp[1]))
            return st, sst
        out, var_out, sm = (np.empty(self.shape, dtype=np.float64) for _ in range(3))
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        call(0, C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data), C.c_void_p(sm.ctypes.data),
             C.c_void_p(fm.ctypes.data) if features else None, C.c_void_p(fv.ctypes.data) if features else None)
        return (out, var_out, sm, fm, fv, st, sst) if features else (out, var_out, sm, st, sst)

    def denoise_multiscale(self, kind="plain", levels=2, radius=None, feature_spp=0, guide=None, demod=None, features=False, out_ptr=None,
                           var_out_ptr=None, features_ptrs=None, **params):
        """The multi-scale (pyramid) form of one of the three filters above on buffer 0 (gdpt_progressive_denoise_multiscale; from 2
        passes on): denoise_nlm_multiscale with `levels` (1 - 4) levels on the session's mean, its variance and, for "guided" and
        "demod", the features it renders. `radius`: None = the variance as estimated, else it is first smoothed over that radius as
        denoise_smoothed does. `guide`, `demod`, `feature_spp`, `params` as denoise_smoothed takes them. Returns (HxWx3 filtered mean,
        HxWx3 variance of the finest level's filter, GdptNlmPyramidStats), with `features=True` the two (8, H, W) feature arrays before
        the stats; with `out_ptr` (and `var_out_ptr`, `features_ptrs` = 2 device addresses) everything stays in device memory and the
        stats alone are returned."""
        k = _kind("denoise_multiscale", kind)
        sp = C.byref(var_smooth_params(radius)) if radius is not None else None
        p, st = nlm_params(**params), defs.GdptNlmPyramidStats()
        g = C.byref(guide) if guide is not None else None
        d = C.byref(demod) if demod is not None else None
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        call = lambda *tail: _check(lib().gdpt_progressive_denoise_multiscale(self.handle, k, int(levels), sp, C.byref(p), g, d,      # noqa: E731
                                                                              int(feature_spp), *tail, C.byref(st)))
        if out_ptr is not None:
            fp = list(features_ptrs) if features_ptrs is not None else [None, None]
            call(1, opt(out_ptr), opt(var_out_ptr), opt(fp[0]), opt(fp[1]))
            return st
        out, var_out = np.empty(self.shape, dtype=np.float64), np.empty(self.shape, dtype=np.float64)
        fshape = (defs.FEATURE_CHANNELS,) + tuple(self.shape[:2])
        fm, fv = (np.empty(fshape, dtype=np.float64), np.empty(fshape, dtype=np.float64)) if features else (None, None)
        call(0, C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data), C.c_void_p(fm.ctypes.data) if features else None,
             C.c_void_p(fv.ctypes.data) if features else None)
        return (out, var_out, fm, fv, st) if features else (out, var_out, st)

    def run(self, target_error=0.0, pass_spp=16, max_passes=0):
        """Adds passes until the budget is spent, `max_passes` were added (0: no limit) or, from 2 passes on, the error estimate is
        <= target_error (0: no target). Returns status(); its stop_reason is "budget", "max_passes" or "target"."""
        st = defs.GdptProgressiveStatus()
        _check(lib().gdpt_progressive_run(self.handle, float(target_error), int(pass_spp), int(max_passes), C.byref(st)))
        return self._status_dict(st)

    def close(self):
        if getattr(self, "handle", None):
            if self._owned:
                lib().gdpt_progressive_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveGroup:
    """One progressive session split over devices on the sample axis (gdpt_progressive_group_*): `devices` lists HIP ordinals (a
    device may appear more than once); member i draws streams [i B / N, (i+1) B / N) of every pixel's block of B = `budget_spp`.
    `total` is a Progressive view of the merged state: read(), reconstruct(), reconstruct_weighted() and status() work on it."""

    def __init__(self, scene_desc, devices, budget_spp, shift=defs.SHIFT_REFERENCE, path=False, max_depth_override=0):
        self.desc = scene_desc
        self.num_members = len(devices)
        cfg = defs.GdptProgressiveConfig(defs.PROGRESSIVE_PATH if path else defs.PROGRESSIVE_GRADPATH, int(shift), int(budget_spp),
                                         int(max_depth_override))
        dev = (C.c_int32 * max(1, len(devices)))(*[int(d) for d in devices])
        h = C.c_void_p()
        _check(lib().gdpt_progressive_group_create(scene_desc.ptr, dev, len(devices), C.byref(cfg), C.byref(h)))
        self.handle = h
        self.total = Progressive._view(self, lib().gdpt_progressive_group_total(h), (scene_desc.height, scene_desc.width, 3), path)

    def run(self, target_error=0.0, pass_spp=16, max_rounds=0, target_recon_error=None, check_every=1, alpha=0.04, norm=defs.RECON_L2,
            weighted=False, conf_floor=0.0, **params):
        """Rounds of one pass per member until all slices are spent, `max_rounds` were done (0: no limit) or, from 2 passes on, the
        total's error estimate is <= target_error (0: no target). Returns the total's status().
        With `target_recon_error` (gdpt_progressive_group_run_recon) the target is the error estimate of the RECONSTRUCTION
        (reconstruct_error(); the kind chosen by alpha, norm, weighted, conf_floor and the keywords of recon_params), taken after every
        `check_every`-th round and once before returning: the status then carries it as "recon_error", with "recon_spread"
        (GdptReconSpreadStats). `target_error` and `target_recon_error` together are refused."""
        st = defs.GdptProgressiveStatus()
        if target_recon_error is None:
            _check(lib().gdpt_progressive_group_run(self.handle, float(target_error), int(pass_spp), int(max_rounds), C.byref(st)))
            return Progressive._status_dict(st)
        if target_error:
            raise GdptError("ProgressiveGroup.run: target_error and target_recon_error exclude each other")
        p, sp = group_recon_params(alpha, norm, weighted, 0, conf_floor, **params), defs.GdptReconSpreadStats()
        _check(lib().gdpt_progressive_group_run_recon(self.handle, float(target_recon_error), int(pass_spp), int(max_rounds), int(check_every),
                                                      C.byref(p), C.byref(st), C.byref(sp)))
        d = Progressive._status_dict(st)
        d["recon_error"] = sp.error_estimate if sp.members else float("nan")
        d["recon_spread"] = sp
        return d

    def reconstruct_error(self, alpha=0.04, norm=defs.RECON_L2, weighted=False, radius=0, conf_floor=0.0, variance=False,
                          out_ptrs=None, **params):
        """The group's image with the error estimate of that image (gdpt_progressive_group_reconstruct_error): every member that holds
        samples reconstructs its own means, and the weighted spread of those reconstructions estimates the variance of the
        reconstruction of the total. `weighted`: the variance-weighted kinds (every member needs 2 passes); `radius`: the error map's
        window (0..8). Returns (HxWx3 image, HxW error map, GdptReconSpreadStats, GdptReconStats of the total), with `variance=True`
        (image, map, HxWx3 variance, spread stats, recon stats); with `out_ptrs` = (image, map or None, variance or None) device
        addresses on devices[0] everything stays there and (spread stats, recon stats) are returned. The L2 kind is linear, so the
        estimate is that of the image returned; for L1 and the weighted kinds it measures the members' spread, not their common bias."""
        p = group_recon_params(alpha, norm, weighted, radius, conf_floor, **params)
        sp, rs = defs.GdptReconSpreadStats(), defs.GdptReconStats()
        if out_ptrs is not None:
            ptrs = [C.c_void_p(int(x)) if x else None for x in (list(out_ptrs) + [None, None])[:3]]
            _check(lib().gdpt_progressive_group_reconstruct_error(self.handle, C.byref(p), 1, *ptrs, C.byref(sp), C.byref(rs)))
            return sp, rs
        shape = self.total.shape
        img, emap = np.empty(shape, dtype=np.float64), np.empty(shape[:2], dtype=np.float64)
        var = np.empty(shape, dtype=np.float64) if variance else None
        _check(lib().gdpt_progressive_group_reconstruct_error(self.handle, C.byref(p), 0, C.c_void_p(img.ctypes.data), C.c_void_p(emap.ctypes.data),
                                                              C.c_void_p(var.ctypes.data) if variance else None, C.byref(sp), C.byref(rs)))
        return (img, emap, var, sp, rs) if variance else (img, emap, sp, rs)

    def halves(self):
        """(A, B): Progressive views of two independent halves of the group's samples (gdpt_progressive_group_halves): the members
        that hold samples, in member order, merged alternately into A and B; rebuilt if a round has run since the last call. They
        read and denoise as `total` does and, like it, take no passes or merges of their own."""
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().gdpt_progressive_group_halves(self.handle, C.byref(a), C.byref(b)))
        return tuple(Progressive._view(self, h.value, self.total.shape, self.total.path) for h in (a, b))

    _SELECT_FILTERS = {"mean": defs.SELECT_MEAN, "nlm": defs.SELECT_NLM, "guided": defs.SELECT_NLM_GUIDED, "demod": defs.SELECT_NLM_DEMOD,
                       "regress": defs.SELECT_NLM_REGRESS, "atrous": defs.SELECT_ATROUS, "collab": defs.SELECT_NLM_COLLAB}

    def denoise_select(self, candidates, radius=None, feature_spp=4, maps=False, features=False, out_ptrs=None):
        """The filters in `candidates` run on the two halves and on the total, and per pixel the one whose error the halves estimate
        smallest (gdpt_progressive_group_denoise_select). A candidate is a dict: `filter` one of "mean", "nlm", "guided", "demod",
        "regress", "atrous", "collab" (or a GDPT_SELECT_* value); `var_smooth`: a radius, for "nlm", "guided" and "demod" only; `nlm`: a
        GdptNlmParams or a dict of nlm_params keywords; `atrous`: a GdptAtrousParams or a dict of atrous_params keywords; `guide`,
        `demod`, `regress`: the blocks, None as in the matching Progressive.denoise_* call. Returns (out HxWx3, GdptSelectStats, list
        of the candidates' GdptNlmStats on the total); with `maps=True` (out, sel HxW int32, mse HxW, stats, list); with
        `features=True` the two (8, H, W) feature arrays follow `out` (or `mse`). `out_ptrs` = (out, sel or None, mse or None) device
        addresses on devices[0]: everything stays there and (stats, list) are returned."""
        n = len(candidates)
        arr, keep = (defs.GdptSelectCandidate * max(1, n))(), []
        for j, c in enumerate(candidates):
            c = dict(c)
            f = c.pop("filter")
            if isinstance(f, str):
                if f not in self._SELECT_FILTERS:
                    raise GdptError(f"ProgressiveGroup.denoise_select: candidates[{j}]: filter must be one of {', '.join(self._SELECT_FILTERS)}")
                f = self._SELECT_FILTERS[f]
            vs = c.pop("var_smooth", None)
            arr[j].filter, arr[j].var_smooth_radius = int(f), -1 if vs is None else int(vs)
            nlm, atrous = c.pop("nlm", None), c.pop("atrous", None)
            blocks = dict(nlm=nlm_params(**nlm) if isinstance(nlm, dict) else nlm, atrous=atrous_params(**atrous) if isinstance(atrous, dict) else atrous,
                          guide=c.pop("guide", None), demod=c.pop("demod", None), regress=c.pop("regress", None))
            if c:
                raise GdptError(f"ProgressiveGroup.denoise_select: candidates[{j}]: unknown key {sorted(c)[0]}")
            for name, b in blocks.items():
                if b is not None:
                    keep.append(b)
                    setattr(arr[j], name, C.pointer(b))
        p = select_params(radius)
        st, cst = defs.GdptSelectStats(), (defs.GdptNlmStats * max(1, n))()
        if out_ptrs is not None:
            ptrs = [C.c_void_p(int(x)) if x else None for x in (list(out_ptrs) + [None, None])[:3]]
            _check(lib().gdpt_progressive_group_denoise_select(self.handle, arr, n, C.byref(p), int(feature_spp), 1, *ptrs, None, None, C.byref(st), cst))
            return st, list(cst[:n])
        shape = self.total.shape
        out = np.empty(shape, dtype=np.float64)
        sel = np.empty(shape[:2], dtype=np.int32) if maps else None
        mse = np.empty(shape[:2], dtype=np.float64) if maps else None
        fm = np.empty((defs.FEATURE_CHANNELS,) + shape[:2], dtype=np.float64) if features else None
        fv = np.empty((defs.FEATURE_CHANNELS,) + shape[:2], dtype=np.float64) if features else None
        host = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None      # noqa: E731
        _check(lib().gdpt_progressive_group_denoise_select(self.handle, arr, n, C.byref(p), int(feature_spp), 0, host(out), host(sel), host(mse), host(fm),
                                                           host(fv), C.byref(st), cst))
        res = (out,) + ((sel, mse) if maps else ()) + ((fm, fv) if features else ())
        return res + (st, list(cst[:n]))

    def member_status(self, i):
        st = defs.GdptProgressiveStatus()
        _check(lib().gdpt_progressive_group_member_status(self.handle, int(i), C.byref(st)))
        return Progressive._status_dict(st)

    def close(self):
        if getattr(self, "handle", None):
            self.total.close()
            lib().gdpt_progressive_group_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fourierSolve(width, height, imgData, imgGradX, imgGradY, dataCost=0.04, solver=defs.SOLVER_DEFAULT, tol=0.0,
                 max_iters=0, return_stats=False):
    """Screened-Poisson reconstruction on the GPU; arguments as the reference's fourierSolve
    (src/render.cpp:172-175). Inputs HxWx3 (or flat W*H*3) float64; returns HxWx3."""
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(height, width, 3) for x in (imgData, imgGradX, imgGradY)]
    out = np.empty((height, width, 3), dtype=np.float64)
    st = defs.GdptPoissonStats()
    _check(lib().gdpt_poisson_solve_ex(int(width), int(height), _dp(a[0]), _dp(a[1]), _dp(a[2]), float(dataCost), _dp(out),
                                       int(solver), float(tol), int(max_iters), C.byref(st)))
    return (out, st) if return_stats else out


def recon_params(norm=defs.RECON_L1, irls_iters=None, eps_init=0.0, eps_decay=0.0, eps_floor=0.0, cg_tol=0.0, cg_max_iters=0):
    """GdptReconParams (include/gdpt.h). None / 0 select the library's defaults (20 rounds, eps 0.05 halved per round down to 1e-3,
    CG to 1e-6 within 1000 iterations); irls_iters=0 means no reweighted round (the C struct spells that as a negative count)."""
    p = defs.GdptReconParams()
    p.norm = int(norm)
    p.irls_iters = 0 if irls_iters is None else (int(irls_iters) if int(irls_iters) > 0 else -1)
    p.cg_max_iters = int(cg_max_iters)
    p.eps_init, p.eps_decay, p.eps_floor, p.cg_tol = float(eps_init), float(eps_decay), float(eps_floor), float(cg_tol)
    return p


def reconstruct(width, height, c, gx, gy, dataCost=0.04, norm=defs.RECON_L1, **params):
    """Reconstruction of the final image from primal and gradients on the GPU (gdpt_reconstruct): RECON_L1 = IRLS over a weighted
    screened-Poisson solve, robust to outliers in the gradients; RECON_L2 = fourierSolve with the default solver, bit for bit.
    `params`: the keywords of recon_params. Inputs HxWx3 (or flat W*H*3) float64; returns (HxWx3 image, GdptReconStats)."""
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(height, width, 3) for x in (c, gx, gy)]
    out = np.empty((height, width, 3), dtype=np.float64)
    p, st = recon_params(norm, **params), defs.GdptReconStats()
    _check(lib().gdpt_reconstruct(int(width), int(height), _dp(a[0]), _dp(a[1]), _dp(a[2]), float(dataCost), C.byref(p), _dp(out), C.byref(st)))
    return out, st


def reconstruct_device(width, height, c_ptr, gx_ptr, gy_ptr, out_ptr, dataCost=0.04, norm=defs.RECON_L1, stream=None, **params):
    """reconstruct() on device addresses (gdpt_reconstruct_device); returns GdptReconStats. The L1 path waits for `stream`."""
    p, st = recon_params(norm, **params), defs.GdptReconStats()
    _check(lib().gdpt_reconstruct_device(int(width), int(height), C.c_void_p(int(c_ptr)), C.c_void_p(int(gx_ptr)), C.c_void_p(int(gy_ptr)),
                                         float(dataCost), C.byref(p), C.c_void_p(int(out_ptr)), C.c_void_p(int(stream) if stream else 0),
                                         C.byref(st)))
    return st


def weighted_recon_params(norm=defs.RECON_L2, conf_floor=0.0, **params):
    """GdptWeightedReconParams (include/gdpt.h): RECON_L2 = weighted least squares (one solve), RECON_L1 = weighted IRLS; conf_floor 0
    selects the default 0.05; `params`: the keywords of recon_params."""
    p = defs.GdptWeightedReconParams()
    p.recon = recon_params(norm, **params)
    p.conf_floor = float(conf_floor)
    return p


def group_recon_params(alpha=0.04, norm=defs.RECON_L2, weighted=False, radius=0, conf_floor=0.0, **params):
    """GdptGroupReconParams (include/gdpt.h): the reconstruction a group's members and total go through, and the error map's radius."""
    p = defs.GdptGroupReconParams()
    p.dataCost, p.weighted, p.map_radius = float(alpha), int(bool(weighted)), int(radius)
    p.recon = recon_params(norm, **params)
    p.wrecon = weighted_recon_params(norm, conf_floor, **params)
    return p


def _spread_args(images, weights, shape):
    n = len(images)
    tab = (C.c_void_p * max(1, n))()
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != n:
        raise GdptError("recon_spread: one weight per image")
    return n, tab, w


def recon_spread(images, weights, total=None, radius=0):
    """The weighted spread of N images of one film on the GPU (gdpt_recon_spread): per component var = M2 / ((N-1) W) around the
    weighted mean, the variance of that mean if image i has variance sigma^2 / weights[i]. Inputs HxWx3 float64; `total` (None: the
    weighted mean) is the image whose squares normalise the estimate. Returns (HxWx3 var, HxW map, GdptReconSpreadStats): the map is
    var summed over the channels, averaged over the finite entries of the (2 radius + 1)^2 window for radius >= 1."""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in images]
    shape = a[0].shape if a else (1, 1, 3)
    h, wd = shape[0], shape[1]
    n, tab, w = _spread_args(a, weights, shape)
    for i, x in enumerate(a):
        if x.shape != shape:
            raise GdptError("recon_spread: the images' shapes differ")
        tab[i] = x.ctypes.data
    t = None if total is None else np.ascontiguousarray(total, dtype=np.float64).reshape(shape)
    var, emap = np.empty((h, wd, 3), dtype=np.float64), np.empty((h, wd), dtype=np.float64)
    st = defs.GdptReconSpreadStats()
    _check(lib().gdpt_recon_spread(int(wd), int(h), n, tab, _dp(w), None if t is None else C.c_void_p(t.ctypes.data), int(radius),
                                   C.c_void_p(var.ctypes.data), C.c_void_p(emap.ctypes.data), C.byref(st)))
    return var, emap, st


def recon_spread_device(width, height, image_ptrs, weights, total_ptr=None, radius=0, var_ptr=None, map_ptr=None, stream=None):
    """recon_spread() on device addresses (gdpt_recon_spread_device); `var_ptr` (W*H*3) and `map_ptr` (W*H) may be None. Returns
    GdptReconSpreadStats. Waits for `stream`."""
    n, tab, w = _spread_args(image_ptrs, weights, None)
    for i, x in enumerate(image_ptrs):
        tab[i] = int(x) if x else None
    st = defs.GdptReconSpreadStats()
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_recon_spread_device(int(width), int(height), n, tab, _dp(w), opt(total_ptr), int(radius), opt(var_ptr), opt(map_ptr),
                                          opt(stream), C.byref(st)))
    return st


def nlm_params(window_radius=None, patch_radius=None, k=None, alpha=None, epsilon=None):
    """GdptNlmParams (include/gdpt.h): the library's defaults (gdpt_nlm_default_params: window radius 10, patch radius 3, k 0.45,
    alpha 1, epsilon 1e-10) with the keywords given in their places, taken literally."""
    p = defs.GdptNlmParams()
    lib().gdpt_nlm_default_params(C.byref(p))
    if window_radius is not None:
        p.window_radius = int(window_radius)
    if patch_radius is not None:
        p.patch_radius = int(patch_radius)
    if k is not None:
        p.k = float(k)
    if alpha is not None:
        p.alpha = float(alpha)
    if epsilon is not None:
        p.epsilon = float(epsilon)
    return p


def denoise_nlm(img, var, **params):
    """Non-local means with variance-cancelling patch distances on the GPU (gdpt_denoise_nlm): `img` a mean and `var` the variance of
    that mean, HxWx3 float64 (what Progressive.read() returns); `params`: the keywords of nlm_params. Returns (HxWx3 filtered image,
    HxWx3 variance of it with the weights taken as fixed, GdptNlmStats). Pixels with a non-finite value or a negative variance are
    returned unchanged and counted in stats.pixels_left_out."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm: img and var must be HxWx3 arrays of one shape")
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = nlm_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_nlm(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data), C.byref(p),
                                  C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data), C.byref(st)))
    return out, var_out, st


def denoise_nlm_device(width, height, img_ptr, var_ptr, out_ptr, var_out_ptr=None, stream=None, stats=True, params=None, **kw):
    """denoise_nlm() on device addresses (gdpt_denoise_nlm_device); `var_out_ptr` may be None. `params`: a GdptNlmParams taken as it
    is (else the keywords of nlm_params). Returns GdptNlmStats after waiting for `stream`; with `stats=False` the call only enqueues
    and returns None."""
    p = params if params is not None else nlm_params(**kw)
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_device(int(width), int(height), opt(img_ptr), opt(var_ptr), C.byref(p), opt(out_ptr), opt(var_out_ptr),
                                         opt(stream), C.byref(st) if stats else None))
    return st


def nlm_guide(num_channels=None, groups=None, k_f=None, alpha_f=None):
    """GdptNlmGuide (include/gdpt.h): the library's defaults (gdpt_nlm_default_guide: the 8 planes of a feature render, an albedo
    group (0, 3, 1e-3) and a normal group (3, 3, 1e-3), k_f 0.6, alpha_f 1) with the keywords given in their places, taken literally.
    `groups`: a list of (first_channel, num_channels, tau), at most 4."""
    g = defs.GdptNlmGuide()
    lib().gdpt_nlm_default_guide(C.byref(g))
    if num_channels is not None:
        g.num_channels = int(num_channels)
    if groups is not None:
        groups = list(groups)
        if len(groups) > defs.NLM_MAX_GROUPS:
            raise GdptError(f"nlm_guide: at most {defs.NLM_MAX_GROUPS} groups")
        g.num_groups = len(groups)
        for j in range(defs.NLM_MAX_GROUPS):
            first, count, tau = groups[j] if j < len(groups) else (0, 0, 0.0)
            g.groups[j] = defs.GdptNlmFeatureGroup(int(first), int(count), float(tau))
    if k_f is not None:
        g.k_f = float(k_f)
    if alpha_f is not None:
        g.alpha_f = float(alpha_f)
    return g


def _feature_planes(feat, feat_var, shape, guide):
    """The two planar feature arrays as C-contiguous (num_channels, H, W) float64, or (None, None)."""
    if feat is None or feat_var is None:
        return None, None
    f = np.ascontiguousarray(feat, dtype=np.float64)
    fv = np.ascontiguousarray(feat_var, dtype=np.float64)
    if f.ndim != 3 or f.shape != fv.shape or f.shape[1:] != tuple(shape[:2]) or f.shape[0] != guide.num_channels:
        raise GdptError("denoise_nlm_guided: feat and feat_var must be (num_channels, H, W) arrays of one shape")
    return f, fv


def denoise_nlm_guided(img, var, feat, feat_var, guide=None, **params):
    """denoise_nlm() with a feature distance capping the colour weights (gdpt_denoise_nlm_guided): `feat`, `feat_var` are planar
    (num_channels, H, W) float64 arrays, a feature and the variance of it per plane (what Scene.features() returns, or any other);
    `guide`: a GdptNlmGuide (nlm_guide(...)), None = the library's default. Returns (HxWx3 filtered image, HxWx3 variance of it,
    GdptNlmStats). Pixels at which a used feature channel is not finite or has a negative variance are left out as well."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm_guided: img and var must be HxWx3 arrays of one shape")
    g = guide if guide is not None else nlm_guide()
    f, fv = _feature_planes(feat, feat_var, a.shape, g)
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = nlm_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_nlm_guided(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                         C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                         C.byref(p), C.byref(g), C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data), C.byref(st)))
    return out, var_out, st


def denoise_nlm_guided_device(width, height, img_ptr, var_ptr, feat_ptr, feat_var_ptr, out_ptr, var_out_ptr=None, guide=None, stream=None,
                              stats=True, params=None, **kw):
    """denoise_nlm_guided() on device addresses (gdpt_denoise_nlm_guided_device); arguments as denoise_nlm_device, with the two planar
    feature arrays and `guide` (None = the library's default)."""
    p = params if params is not None else nlm_params(**kw)
    g = guide if guide is not None else nlm_guide()
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_guided_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), C.byref(p),
                                                C.byref(g), opt(out_ptr), opt(var_out_ptr), opt(stream), C.byref(st) if stats else None))
    return st


def _joint_table(ptrs, n):
    """n addresses as the `double *const *` of the C ABI (None entries stay NULL); None: a NULL table."""
    if ptrs is None:
        return None
    arr = (C.c_void_p * max(1, n))()
    for i in range(n):
        arr[i] = int(ptrs[i]) if i < len(ptrs) and ptrs[i] else None
    return arr


def denoise_nlm_joint(img, var, companions, companion_vars, feat=None, feat_var=None, guide=None, **params):
    """denoise_nlm_guided() whose weights also filter companion films (gdpt_denoise_nlm_joint): `img`, `var` the guide film,
    `companions`, `companion_vars` lists of at most 4 HxWx3 films and their variances, filtered with the guide film's weights.
    `guide`: a GdptNlmGuide (nlm_guide(...)), None = the library's default when `feat` is given and NO feature term when it is not.
    Returns (HxWx3 filtered guide film, its variance, list of filtered companions, list of their variances, GdptNlmJointStats). A
    pixel that is not finite, or has a negative variance, in any of the films is left out of all of them."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm_joint: img and var must be HxWx3 arrays of one shape")
    cs = [np.ascontiguousarray(x, dtype=np.float64) for x in companions]
    cv = [np.ascontiguousarray(x, dtype=np.float64) for x in companion_vars]
    if len(cs) != len(cv) or any(x.shape != a.shape for x in cs + cv):
        raise GdptError("denoise_nlm_joint: companions and companion_vars must be lists of one length of arrays shaped like img")
    g = guide if guide is not None else (nlm_guide() if feat is not None else nlm_guide(groups=[]))
    f, fv = _feature_planes(feat, feat_var, a.shape, g)
    n = len(cs)
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    co, cvo = [np.empty(a.shape, dtype=np.float64) for _ in range(n)], [np.empty(a.shape, dtype=np.float64) for _ in range(n)]
    p, st = nlm_params(**params), defs.GdptNlmJointStats()
    tab = lambda arrs: _joint_table([x.ctypes.data for x in arrs], n)      # noqa: E731
    _check(lib().gdpt_denoise_nlm_joint(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                        C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                        n, tab(cs), tab(cv), C.byref(p), C.byref(g), C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data),
                                        tab(co), tab(cvo), C.byref(st)))
    return out, var_out, co, cvo, st


def denoise_nlm_joint_device(width, height, img_ptr, var_ptr, comp_ptrs, comp_var_ptrs, out_ptr, comp_out_ptrs, var_out_ptr=None,
                             comp_var_out_ptrs=None, feat_ptr=None, feat_var_ptr=None, guide=None, stream=None, stats=True, params=None, **kw):
    """denoise_nlm_joint() on device addresses (gdpt_denoise_nlm_joint_device): `comp_ptrs`, `comp_var_ptrs`, `comp_out_ptrs` and
    `comp_var_out_ptrs` (None, or None entries: not wanted) are lists of one length, at most 4. `guide`: None = the library's default
    when `feat_ptr` is given and NO feature term when it is not. Returns GdptNlmJointStats after waiting for `stream`; with
    `stats=False` the call only enqueues and returns None."""
    p = params if params is not None else nlm_params(**kw)
    g = guide if guide is not None else (nlm_guide() if feat_ptr else nlm_guide(groups=[]))
    st = defs.GdptNlmJointStats() if stats else None
    n = len(comp_ptrs)
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_joint_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), n,
                                               _joint_table(comp_ptrs, n), _joint_table(comp_var_ptrs, n), C.byref(p), C.byref(g), opt(out_ptr),
                                               opt(var_out_ptr), _joint_table(comp_out_ptrs, n), _joint_table(comp_var_out_ptrs, n), opt(stream),
                                               C.byref(st) if stats else None))
    return st


def nlm_regress(channels=None, scales=None, ridge=None):
    """GdptNlmRegress (include/gdpt.h): the library's defaults (gdpt_nlm_default_regress: the planes 0 - 5 of a feature render, albedo
    and shading normal, every scale 1, ridge 1e-2) with the keywords given in their places, taken literally. `channels`: the regressor
    planes, at most 7; `scales`: one divisor per channel (None with `channels` given: 1.0 each)."""
    r = defs.GdptNlmRegress()
    lib().gdpt_nlm_default_regress(C.byref(r))
    if channels is not None:
        channels = [int(c) for c in channels]
        if len(channels) > defs.NLM_MAX_REGRESSORS:
            raise GdptError(f"nlm_regress: at most {defs.NLM_MAX_REGRESSORS} channels")
        r.num_regressors = len(channels)
        for j in range(defs.NLM_MAX_REGRESSORS):
            r.channel[j] = channels[j] if j < len(channels) else 0
            r.scale[j] = 1.0 if j < len(channels) else 0.0
    if scales is not None:
        scales = [float(x) for x in scales]
        if len(scales) != r.num_regressors:
            raise GdptError("nlm_regress: scales must have one entry per channel")
        for j, x in enumerate(scales):
            r.scale[j] = x
    if ridge is not None:
        r.ridge = float(ridge)
    return r


def denoise_nlm_regress(img, var, feat, feat_var, guide=None, regress=None, **params):
    """denoise_nlm_guided() with a weighted linear fit of the colour on feature planes in the place of the weighted mean
    (gdpt_denoise_nlm_regress): arguments as denoise_nlm_guided, with `regress` a GdptNlmRegress (nlm_regress(...)), None = the
    library's default. Returns (HxWx3 fitted image, HxWx3 variance of it with the weights taken as fixed, GdptNlmStats). Pixels at
    which a group's or a regressor's channel is not finite or has a negative variance are left out."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm_regress: img and var must be HxWx3 arrays of one shape")
    g = guide if guide is not None else nlm_guide()
    rg = regress if regress is not None else nlm_regress()
    f, fv = _feature_planes(feat, feat_var, a.shape, g)
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = nlm_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_nlm_regress(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                          C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                          C.byref(p), C.byref(g), C.byref(rg), C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data),
                                          C.byref(st)))
    return out, var_out, st


def denoise_nlm_regress_device(width, height, img_ptr, var_ptr, feat_ptr, feat_var_ptr, out_ptr, var_out_ptr=None, guide=None, regress=None,
                               stream=None, stats=True, params=None, **kw):
    """denoise_nlm_regress() on device addresses (gdpt_denoise_nlm_regress_device); arguments as denoise_nlm_guided_device, with
    `regress` (None = the library's default)."""
    p = params if params is not None else nlm_params(**kw)
    g = guide if guide is not None else nlm_guide()
    rg = regress if regress is not None else nlm_regress()
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_regress_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), C.byref(p),
                                                 C.byref(g), C.byref(rg), opt(out_ptr), opt(var_out_ptr), opt(stream),
                                                 C.byref(st) if stats else None))
    return st


def denoise_nlm_collab(img, var, feat, feat_var, guide=None, regress=None, coef=False, **params):
    """The collaborative form of denoise_nlm_regress() (gdpt_denoise_nlm_collab): every pixel takes the weighted average of all fits
    whose windows cover it. Arguments as denoise_nlm_regress. Returns (HxWx3 image, GdptNlmStats), with `coef=True` (image, the
    (3 (1 + m), H, W) coefficient film, stats): plane c (1 + m) + j holds beta_c,j. There is no variance of the result: the stats'
    sum_var_out and error_out are NaN."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm_collab: img and var must be HxWx3 arrays of one shape")
    g = guide if guide is not None else nlm_guide()
    rg = regress if regress is not None else nlm_regress()
    f, fv = _feature_planes(feat, feat_var, a.shape, g)
    out = np.empty(a.shape, dtype=np.float64)
    planes = np.empty((3 * (1 + max(0, int(rg.num_regressors))),) + a.shape[:2], dtype=np.float64) if coef else None
    p, st = nlm_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_nlm_collab(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                         C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                         C.byref(p), C.byref(g), C.byref(rg), C.c_void_p(out.ctypes.data),
                                         C.c_void_p(planes.ctypes.data) if coef else None, C.byref(st)))
    return (out, planes, st) if coef else (out, st)


def denoise_nlm_collab_device(width, height, img_ptr, var_ptr, feat_ptr, feat_var_ptr, out_ptr, coef_ptr=None, guide=None, regress=None,
                              stream=None, stats=True, params=None, **kw):
    """denoise_nlm_collab() on device addresses (gdpt_denoise_nlm_collab_device); arguments as denoise_nlm_regress_device, with
    `coef_ptr` (3 (1 + m) planes of width * height doubles; None = the library keeps the coefficient film) in the place of
    `var_out_ptr`."""
    p = params if params is not None else nlm_params(**kw)
    g = guide if guide is not None else nlm_guide()
    rg = regress if regress is not None else nlm_regress()
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_collab_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), C.byref(p),
                                                C.byref(g), C.byref(rg), opt(out_ptr), opt(coef_ptr), opt(stream),
                                                C.byref(st) if stats else None))
    return st


def nlm_demod(albedo_channel=None, coverage_channel=None, floor=None):
    """GdptNlmDemod (include/gdpt.h): the library's defaults (gdpt_nlm_default_demod: albedo planes 0-2, coverage plane 7, floor 1e-3,
    the layout of a feature render) with the keywords given in their places, taken literally. coverage_channel = -1: none."""
    d = defs.GdptNlmDemod()
    lib().gdpt_nlm_default_demod(C.byref(d))
    if albedo_channel is not None:
        d.albedo_channel = int(albedo_channel)
    if coverage_channel is not None:
        d.coverage_channel = int(coverage_channel)
    if floor is not None:
        d.floor = float(floor)
    return d


def denoise_nlm_demod(img, var, feat, feat_var, guide=None, demod=None, **params):
    """denoise_nlm() on the albedo-demodulated mean (gdpt_denoise_nlm_demod): img / a~ is filtered and a~ multiplied back, a~ the
    effective albedo max(floor, albedo + (1 - coverage)) taken from the planar (num_channels, H, W) arrays `feat`, `feat_var` (what
    Scene.features() returns, or any other). `demod`: a GdptNlmDemod (nlm_demod(...)), None = the library's default; `guide`: a
    GdptNlmGuide over the same planes, None = NO feature term (not the default guide: the albedo is already divided out). Returns
    (HxWx3 filtered image, HxWx3 variance of it, GdptNlmStats). Pixels whose albedo or coverage is not finite are left out as well."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_nlm_demod: img and var must be HxWx3 arrays of one shape")
    f = np.ascontiguousarray(feat, dtype=np.float64)
    fv = np.ascontiguousarray(feat_var, dtype=np.float64)
    if f.ndim != 3 or f.shape != fv.shape or f.shape[1:] != a.shape[:2]:
        raise GdptError("denoise_nlm_demod: feat and feat_var must be (num_channels, H, W) arrays of one shape")
    d = demod if demod is not None else nlm_demod()
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = nlm_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_nlm_demod(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                        C.c_void_p(f.ctypes.data), C.c_void_p(fv.ctypes.data), int(f.shape[0]), C.byref(p),
                                        C.byref(guide) if guide is not None else None, C.byref(d), C.c_void_p(out.ctypes.data),
                                        C.c_void_p(var_out.ctypes.data), C.byref(st)))
    return out, var_out, st


def denoise_nlm_demod_device(width, height, img_ptr, var_ptr, feat_ptr, feat_var_ptr, num_channels, out_ptr, var_out_ptr=None, guide=None,
                             demod=None, stream=None, stats=True, params=None, **kw):
    """denoise_nlm_demod() on device addresses (gdpt_denoise_nlm_demod_device); arguments as denoise_nlm_guided_device, with the number
    of planes, `demod` (None = the library's default) and `guide` (None = no feature term)."""
    p = params if params is not None else nlm_params(**kw)
    d = demod if demod is not None else nlm_demod()
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_demod_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), int(num_channels),
                                               C.byref(p), C.byref(guide) if guide is not None else None, C.byref(d), opt(out_ptr), opt(var_out_ptr),
                                               opt(stream), C.byref(st) if stats else None))
    return st


def atrous_params(levels=None, first_level=None, k=None, alpha=None, epsilon=None):
    """GdptAtrousParams (include/gdpt.h): the library's defaults (gdpt_atrous_default_params: 5 levels from level 0, k 2.0, alpha 1,
    epsilon 1e-10) with the keywords given in their places, taken literally."""
    p = defs.GdptAtrousParams()
    lib().gdpt_atrous_default_params(C.byref(p))
    if levels is not None:
        p.levels = int(levels)
    if first_level is not None:
        p.first_level = int(first_level)
    if k is not None:
        p.k = float(k)
    if alpha is not None:
        p.alpha = float(alpha)
    if epsilon is not None:
        p.epsilon = float(epsilon)
    return p


def denoise_atrous(img, var, feat=None, feat_var=None, guide=None, demod=None, **params):
    """The edge-avoiding a-trous wavelet filter on the GPU (gdpt_denoise_atrous), the cheap filter: `levels` passes of a 5x5 B3-spline
    kernel whose taps are spread by 1, 2, 4, ... pixels, every tap weighted by the variance-cancelling pixel distance of denoise_nlm,
    capped by the feature distance of `guide` (a GdptNlmGuide, nlm_guide(...); None = NO feature term), on img / a~ when `demod` (a
    GdptNlmDemod, nlm_demod(...); None = NO demodulation) is given. `img`, `var`: HxWx3 float64; `feat`, `feat_var`: planar
    (num_channels, H, W) float64 arrays, needed with a group or a demod block; `params`: the keywords of atrous_params. Returns
    (HxWx3 filtered image, HxWx3 variance of it with the weights taken as fixed, GdptNlmStats); stats.window_radius is the reach of
    the last level."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("denoise_atrous: img and var must be HxWx3 arrays of one shape")
    f = fv = None
    channels = guide.num_channels if guide is not None else 0
    if feat is not None and feat_var is not None:
        f = np.ascontiguousarray(feat, dtype=np.float64)
        fv = np.ascontiguousarray(feat_var, dtype=np.float64)
        if f.ndim != 3 or f.shape != fv.shape or f.shape[1:] != a.shape[:2]:
            raise GdptError("denoise_atrous: feat and feat_var must be (num_channels, H, W) arrays of one shape")
        channels = int(f.shape[0])
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = atrous_params(**params), defs.GdptNlmStats()
    _check(lib().gdpt_denoise_atrous(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                     C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                     channels, C.byref(p), C.byref(guide) if guide is not None else None,
                                     C.byref(demod) if demod is not None else None, C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data),
                                     C.byref(st)))
    return out, var_out, st


def denoise_atrous_device(width, height, img_ptr, var_ptr, feat_ptr, feat_var_ptr, num_channels, out_ptr, var_out_ptr=None, guide=None,
                          demod=None, stream=None, stats=True, params=None, **kw):
    """denoise_atrous() on device addresses (gdpt_denoise_atrous_device); arguments as denoise_nlm_demod_device, with `guide` and
    `demod` None = none of either, and `params` a GdptAtrousParams taken as it is (else the keywords of atrous_params)."""
    p = params if params is not None else atrous_params(**kw)
    st = defs.GdptNlmStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_atrous_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), int(num_channels),
                                            C.byref(p), C.byref(guide) if guide is not None else None,
                                            C.byref(demod) if demod is not None else None, opt(out_ptr), opt(var_out_ptr), opt(stream),
                                            C.byref(st) if stats else None))
    return st


def temporal_params(tau_z=None, tau_n=None, s_min=None, max_history=None):
    """GdptTemporalParams (include/gdpt.h): the library's defaults (gdpt_temporal_default_params: tau_z 0.05, tau_n 0.9, s_min 1e-3,
    max_history 32) with the keywords given in their places, taken literally."""
    p = defs.GdptTemporalParams()
    lib().gdpt_temporal_default_params(C.byref(p))
    if tau_z is not None:
        p.tau_z = float(tau_z)
    if tau_n is not None:
        p.tau_n = float(tau_n)
    if s_min is not None:
        p.s_min = float(s_min)
    if max_history is not None:
        p.max_history = int(max_history)
    return p


def temporal_grad_params(j_max=None, cos_min=None):
    """GdptTemporalGradParams (include/gdpt.h): the library's defaults (gdpt_temporal_default_grad_params: j_max 4, cos_min 0.02) with
    the keywords given in their places, taken literally."""
    p = defs.GdptTemporalGradParams()
    lib().gdpt_temporal_default_grad_params(C.byref(p))
    if j_max is not None:
        p.j_max = float(j_max)
    if cos_min is not None:
        p.cos_min = float(cos_min)
    return p


def temporal_world_to_sample(camera):
    """M(camera) of the temporal definition (gdpt_temporal_world_to_sample): the 4x4 float64 inverse(sample_to_cam)
    inverse(cam_to_world) as the library computes it."""
    M = np.empty((4, 4), dtype=np.float64)
    _check(lib().gdpt_temporal_world_to_sample(C.byref(camera) if camera is not None else None, _dp(M)))
    return M


def orbit_camera(camera, centre, degrees):
    """A copy of the GdptCamera `camera` whose cam_to_world is turned by `degrees` about the world's vertical (y) axis through the point
    `centre`: T(centre) R_y(degrees) T(-centre) cam_to_world, the camera of frame f of `lajolla --frames N --orbit DEG` at f DEG."""
    a = np.radians(float(degrees))
    cs, sn = np.cos(a), np.sin(a)
    c = [float(x) for x in centre]
    R = np.array([[cs, 0, sn, c[0] - cs * c[0] - sn * c[2]], [0, 1, 0, 0], [-sn, 0, cs, c[2] + sn * c[0] - cs * c[2]], [0, 0, 0, 1]])
    out = defs.GdptCamera.from_buffer_copy(camera)
    m = R @ np.array(list(camera.cam_to_world), dtype=np.float64).reshape(4, 4)
    for i in range(16):
        out.cam_to_world[i] = float(m.flat[i])
    return out


class Temporal:
    """Temporal reprojection of an accumulated mean and its variance across a camera move (include/gdpt.h, gdpt_temporal_*): a handle
    bound to (width, height, device, stream) that owns the history. `stream`: a hipStream_t address carrying the handle's work."""

    def __init__(self, width, height, device=0, stream=None):
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _check(lib().gdpt_temporal_create(self.width, self.height, int(device), C.c_void_p(int(stream) if stream else 0), C.byref(h)))
        self.handle = h

    def push(self, camera, img, var, feat, length=True, params=None, **kw):
        """One frame into the history (gdpt_temporal_push). `img`, `var`: HxWx3 float64, the frame's mean and variance of the mean;
        `feat`: the (8, H, W) float64 planes of a feature render of the frame; `params`: a GdptTemporalParams taken as it is (else the
        keywords of temporal_params). Returns (out, var_out, HxW history length N' or None, GdptTemporalStats)."""
        shape = (self.height, self.width, 3)
        a = np.ascontiguousarray(img, dtype=np.float64)
        v = np.ascontiguousarray(var, dtype=np.float64)
        f = np.ascontiguousarray(feat, dtype=np.float64)
        if a.shape != shape or v.shape != shape or f.shape != (defs.FEATURE_CHANNELS, self.height, self.width):
            raise GdptError("Temporal.push: img and var must be HxWx3 and feat (8, H, W) arrays of the handle's film")
        out, var_out = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.float64)
        n = np.empty(shape[:2], dtype=np.float64) if length else None
        p, st = params if params is not None else temporal_params(**kw), defs.GdptTemporalStats()
        _check(lib().gdpt_temporal_push(self.handle, C.byref(camera), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                        C.c_void_p(f.ctypes.data), C.byref(p), C.c_void_p(out.ctypes.data), C.c_void_p(var_out.ctypes.data),
                                        C.c_void_p(n.ctypes.data) if n is not None else None, C.byref(st)))
        return out, var_out, n, st

    def push_device(self, camera, img_ptr, var_ptr, feat_ptr, out_ptr, var_out_ptr, len_ptr=None, stats=True, params=None, **kw):
        """push() on device addresses (gdpt_temporal_push_device), enqueued on the handle's stream; enqueue-only with `stats` False.
        Returns the GdptTemporalStats or None."""
        p = params if params is not None else temporal_params(**kw)
        st = defs.GdptTemporalStats() if stats else None
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        _check(lib().gdpt_temporal_push_device(self.handle, C.byref(camera) if camera is not None else None, opt(img_ptr), opt(var_ptr),
                                               opt(feat_ptr), C.byref(p), opt(out_ptr), opt(var_out_ptr), opt(len_ptr),
                                               C.byref(st) if stats else None))
        return st

    GRAD_OUTPUTS = ("gx_out", "gx_var_out", "gy_out", "gy_var_out")

    @staticmethod
    def _split_grad_keywords(kw):
        """(keywords of temporal_params, keywords of temporal_grad_params)"""
        g = {k: kw[k] for k in ("j_max", "cos_min") if k in kw}
        return {k: v for k, v in kw.items() if k not in g}, g

    def push_gradients(self, camera, img, var, feat, gx, gx_var, gy, gy_var, length=True, params=None, grad_params=None, **kw):
        """One frame with its assembled gradients into the history (gdpt_temporal_push_gradients). `img`, `var`, `feat` as push();
        `gx`, `gy`: HxWx3 float64, the assembled cx, cy; `gx_var`, `gy_var`: their variances of the mean; `grad_params`: a
        GdptTemporalGradParams taken as it is (else the keywords j_max, cos_min of temporal_grad_params). Returns a dict: out, var_out,
        length (N' or None), gx_out, gx_var_out, gy_out, gy_var_out, glength (N_g' or None), stats (GdptTemporalGradStats)."""
        shape = (self.height, self.width, 3)
        ins = [np.ascontiguousarray(x, dtype=np.float64) for x in (img, var, gx, gx_var, gy, gy_var)]
        f = np.ascontiguousarray(feat, dtype=np.float64)
        if any(x.shape != shape for x in ins) or f.shape != (defs.FEATURE_CHANNELS, self.height, self.width):
            raise GdptError("Temporal.push_gradients: img, var and the gradients must be HxWx3 and feat (8, H, W) arrays of the handle's film")
        kw, gkw = self._split_grad_keywords(kw)
        p = params if params is not None else temporal_params(**kw)
        gp = grad_params if grad_params is not None else temporal_grad_params(**gkw)
        r = {k: np.empty(shape, dtype=np.float64) for k in ("out", "var_out") + self.GRAD_OUTPUTS}
        r["length"] = np.empty(shape[:2], dtype=np.float64) if length else None
        r["glength"] = np.empty(shape[:2], dtype=np.float64) if length else None
        st = defs.GdptTemporalGradStats()
        ptr = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None      # noqa: E731
        _check(lib().gdpt_temporal_push_gradients(self.handle, C.byref(camera), ptr(ins[0]), ptr(ins[1]), ptr(f), *[ptr(x) for x in ins[2:]],
                                                  C.byref(p), C.byref(gp), ptr(r["out"]), ptr(r["var_out"]), ptr(r["length"]),
                                                  *[ptr(r[k]) for k in self.GRAD_OUTPUTS], ptr(r["glength"]), C.byref(st)))
        r["stats"] = st
        return r

    def push_gradients_device(self, camera, img_ptr, var_ptr, feat_ptr, grad_ptrs, out_ptr, var_out_ptr, grad_out_ptrs, len_ptr=None,
                              glen_ptr=None, stats=True, params=None, grad_params=None, **kw):
        """push_gradients() on device addresses (gdpt_temporal_push_gradients_device), enqueued on the handle's stream. `grad_ptrs`: the
        four addresses of gx, gx_var, gy, gy_var; `grad_out_ptrs`: those of gx_out, gx_var_out, gy_out, gy_var_out. Enqueue-only with
        `stats` False. Returns the GdptTemporalGradStats or None."""
        kw, gkw = self._split_grad_keywords(kw)
        p = params if params is not None else temporal_params(**kw)
        gp = grad_params if grad_params is not None else temporal_grad_params(**gkw)
        st = defs.GdptTemporalGradStats() if stats else None
        opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
        gi, go = list(grad_ptrs), list(grad_out_ptrs)
        if len(gi) != 4 or len(go) != 4:
            raise GdptError("Temporal.push_gradients_device: grad_ptrs and grad_out_ptrs hold four addresses each")
        _check(lib().gdpt_temporal_push_gradients_device(self.handle, C.byref(camera) if camera is not None else None, opt(img_ptr), opt(var_ptr),
                                                         opt(feat_ptr), *[opt(x) for x in gi], C.byref(p), C.byref(gp), opt(out_ptr),
                                                         opt(var_out_ptr), opt(len_ptr), *[opt(x) for x in go], opt(glen_ptr),
                                                         C.byref(st) if stats else None))
        return st

    @staticmethod
    def assemble(means):
        """(c, cx, cy) of a GradPath session's five means, one addition a value: the bits of gdpt_assemble_device."""
        cx, cy = means["cx0"].copy(), means["cy0"].copy()
        cx[:, 1:] = means["cx0"][:, 1:] + means["cx1"][:, :-1]
        cy[1:, :] = means["cy0"][1:, :] + means["cy1"][:-1, :]
        return means["img"], cx, cy

    def _frame_gradients(self, scene, camera, frame_index, frames, spp, pass_spp, atrous, feature_spp, params, reconstruct_, alpha, kw):
        """frame() with gradients=True"""
        if reconstruct_ not in (None, "l2", "wl2", "wl1"):
            raise GdptError("Temporal.frame: reconstruct is None, 'l2', 'wl2' or 'wl1'")
        if scene.desc.desc.integrator == defs.INTEGRATOR_PATH:
            raise GdptError("Temporal.frame: gradients=True needs a GradPath scene; this one is Integrator::Path, which renders no gradients")
        scene.set_camera(camera)
        first, block = int(frame_index) * spp, int(frames) * spp
        session = Progressive(scene, block, path=False, slice=(first, spp))
        try:
            done = 0
            while done < spp:
                n = min(pass_spp, spp - done)
                session.add_pass(n)
                done += n
            means, vars_, asm = session.read()
        finally:
            session.close()
        feat, feat_var = scene.features(int(feature_spp) if feature_spp else spp, window=(block, first))
        c, cx, cy = self.assemble(means)
        r = self.push_gradients(camera, c, asm["c"], feat, cx, asm["cx"], cy, asm["cy"], params=params, **kw)
        r.update(mean=means["img"], var=vars_["img"], feat=feat, feat_var=feat_var, c=c, cx=cx, cy=cy, assembled_vars=asm)
        if atrous is not None:
            r["denoised"], r["denoised_var"], r["atrous_stats"] = denoise_atrous(r["out"], r["var_out"], feat, feat_var, guide=nlm_guide(), **atrous)
        if reconstruct_ == "l2":
            r["reconstructed"], r["recon_stats"] = reconstruct(self.width, self.height, r["out"], r["gx_out"], r["gy_out"], dataCost=alpha,
                                                               norm=defs.RECON_L2)
        elif reconstruct_ is not None:
            r["reconstructed"], r["recon_stats"] = reconstruct_weighted(self.width, self.height, r["out"], r["gx_out"], r["gy_out"], r["var_out"],
                                                                        r["gx_var_out"], r["gy_var_out"], dataCost=alpha,
                                                                        norm=defs.RECON_L2 if reconstruct_ == "wl2" else defs.RECON_L1)
        return r

    def frame(self, scene, camera, frame_index, frames, spp, pass_spp, path=True, atrous=None, feature_spp=None, params=None, gradients=False,
              reconstruct=None, alpha=0.04, **kw):
        """One frame of a moving camera, from pieces that exist: scene.set_camera(camera); a slice session over the sample window
        [frame_index spp, (frame_index + 1) spp) of frames spp streams, so that frames never repeat samples, in passes of `pass_spp`
        (at least two, so that a variance exists); its mean and variance (the primal's, for GradPath: `path` False); the features on
        the same window at `feature_spp` (None: spp) samples; push(). `atrous`: None, or a dict of atrous_params keywords: then
        denoise_atrous on (out, var_out) under the frame's features with the default guide. The history keeps the unfiltered
        accumulation. Returns a dict: out, var_out, length, stats, mean, var, feat, feat_var, and with `atrous` denoised,
        denoised_var, atrous_stats.
        With `gradients` (needs `path` False and a GradPath scene): the session's five means are assembled into c, cx, cy (assemble()),
        and push_gradients() takes them with the session's assembled variances (the keywords j_max, cos_min go to it). The dict gains
        gx_out, gx_var_out, gy_out, gy_var_out, glength, c, cx, cy, assembled_vars, stats becomes a GdptTemporalGradStats, and with
        `reconstruct` 'l2' | 'wl2' | 'wl1' it gains reconstructed (and recon_stats): reconstruct(norm=RECON_L2), or reconstruct_weighted
        on the accumulated variances, of the accumulated triple at dataCost `alpha`. Without `gradients` nothing changes."""
        spp, pass_spp = int(spp), int(pass_spp)
        if pass_spp < 1 or spp < 2 * pass_spp:
            raise GdptError("Temporal.frame: spp must hold at least two passes of pass_spp")
        if gradients:
            if path:
                raise GdptError("Temporal.frame: gradients=True needs path=False (a Path session renders no gradients)")
            return self._frame_gradients(scene, camera, frame_index, frames, spp, pass_spp, atrous, feature_spp, params, reconstruct, alpha, kw)
        if reconstruct is not None:
            raise GdptError("Temporal.frame: reconstruct needs gradients=True")
        scene.set_camera(camera)
        first, block = int(frame_index) * spp, int(frames) * spp
        session = Progressive(scene, block, path=path, slice=(first, spp))
        try:
            done = 0
            while done < spp:
                n = min(pass_spp, spp - done)
                session.add_pass(n)
                done += n
            means, vars_, _ = session.read()
        finally:
            session.close()
        feat, feat_var = scene.features(int(feature_spp) if feature_spp else spp, window=(block, first))
        out, var_out, length, st = self.push(camera, means["img"], vars_["img"], feat, params=params, **kw)
        r = dict(out=out, var_out=var_out, length=length, stats=st, mean=means["img"], var=vars_["img"], feat=feat, feat_var=feat_var)
        if atrous is not None:
            r["denoised"], r["denoised_var"], r["atrous_stats"] = denoise_atrous(out, var_out, feat, feat_var, guide=nlm_guide(), **atrous)
        return r

    def reset(self):
        """The next push is a first push (gdpt_temporal_reset)."""
        _check(lib().gdpt_temporal_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            lib().gdpt_temporal_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def var_smooth_params(radius=None):
    """GdptVarSmoothParams (include/gdpt.h): the library's default (gdpt_var_smooth_default_params: radius 2) with the keyword given
    in its place, taken literally."""
    p = defs.GdptVarSmoothParams()
    lib().gdpt_var_smooth_default_params(C.byref(p))
    if radius is not None:
        p.radius = int(radius)
    return p


def variance_smooth(img, var, feat=None, feat_var=None, demod=None, params=None, radius=None):
    """The box mean of the variance of a mean over the valid pixels of a (2 radius + 1)^2 window on the GPU (gdpt_variance_smooth):
    what the non-local-means filters are then run on in the place of `var`. `img`, `var`: HxWx3 float64. With the planar
    (num_channels, H, W) arrays `feat`, `feat_var` the mean is taken of var / a~^2 and a~^2 multiplied back, a~ the effective albedo of
    `demod` (a GdptNlmDemod, nlm_demod(...); None = the library's default block); without them `demod` must be None. `params`: a
    GdptVarSmoothParams taken as it is (else var_smooth_params(radius)). Returns (HxWx3 smoothed variance, GdptVarSmoothStats)."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError("variance_smooth: img and var must be HxWx3 arrays of one shape")
    f = fv = None
    if feat is not None or feat_var is not None:
        if feat is None or feat_var is None:
            raise GdptError("variance_smooth: feat and feat_var go together")
        f = np.ascontiguousarray(feat, dtype=np.float64)
        fv = np.ascontiguousarray(feat_var, dtype=np.float64)
        if f.ndim != 3 or f.shape != fv.shape or f.shape[1:] != a.shape[:2]:
            raise GdptError("variance_smooth: feat and feat_var must be (num_channels, H, W) arrays of one shape")
        if demod is None:
            demod = nlm_demod()
    p = params if params is not None else var_smooth_params(radius)
    out, st = np.empty(a.shape, dtype=np.float64), defs.GdptVarSmoothStats()
    _check(lib().gdpt_variance_smooth(int(a.shape[1]), int(a.shape[0]), C.c_void_p(a.ctypes.data), C.c_void_p(v.ctypes.data),
                                      C.c_void_p(f.ctypes.data) if f is not None else None, C.c_void_p(fv.ctypes.data) if fv is not None else None,
                                      int(f.shape[0]) if f is not None else 0, C.byref(p), C.byref(demod) if demod is not None else None,
                                      C.c_void_p(out.ctypes.data), C.byref(st)))
    return out, st


def variance_smooth_device(width, height, img_ptr, var_ptr, var_out_ptr, feat_ptr=None, feat_var_ptr=None, num_channels=0, demod=None, stream=None,
                           stats=True, params=None, radius=None):
    """variance_smooth() on device addresses (gdpt_variance_smooth_device). `feat_ptr`, `feat_var_ptr` and `demod` go together and are
    passed as they are: `demod` None is no block here. Returns GdptVarSmoothStats after waiting for `stream`; with `stats=False` the
    call only enqueues and returns None."""
    p = params if params is not None else var_smooth_params(radius)
    st = defs.GdptVarSmoothStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_variance_smooth_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), int(num_channels),
                                             C.byref(p), C.byref(demod) if demod is not None else None, opt(var_out_ptr), opt(stream),
                                             C.byref(st) if stats else None))
    return st


def select_params(radius=None):
    """GdptSelectParams (include/gdpt.h): the library's default (gdpt_select_default_params: radius 4) with the keyword given in its
    place, taken literally."""
    p = defs.GdptSelectParams()
    lib().gdpt_select_default_params(C.byref(p))
    if radius is not None:
        p.radius = int(radius)
    return p


def _pointer_array(ptrs):
    """A C array of void pointers from addresses; 0 or None gives NULL."""
    return (C.c_void_p * max(1, len(ptrs)))(*[C.c_void_p(int(x)) if x else None for x in ptrs])


def filter_select(FA, FB, T, uA, vA, uB, vB, params=None, radius=None, maps=True, E=False):
    """The per-pixel choice among candidate filters by the two-half error estimate on the GPU (gdpt_filter_select). `FA`, `FB`, `T`:
    sequences of n HxWx3 float64 arrays, candidate j run on half A, on half B and on all samples; `uA`, `vA`, `uB`, `vB`: the halves'
    means and the variances of those means. `params`: a GdptSelectParams taken as it is (else select_params(radius)). Returns
    (out HxWx3, sel HxW int32, mse HxW, GdptSelectStats), with `E=True` also the (n, H, W) window means E_j before the stats; with
    `maps=False` only (out, stats)."""
    arr = lambda a: np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
    FA, FB, T = [arr(a) for a in FA], [arr(a) for a in FB], [arr(a) for a in T]
    halves = [arr(a) for a in (uA, vA, uB, vB)]
    if len(FA) != len(T) or len(FB) != len(T):
        raise GdptError("filter_select: FA, FB and T must hold one image per candidate each")
    shape = halves[0].shape
    if len(shape) != 3 or shape[2] != 3 or any(a.shape != shape for a in FA + FB + T + halves):
        raise GdptError("filter_select: every image must be an HxWx3 array of one shape")
    n, (h, w) = len(T), shape[:2]
    p = params if params is not None else select_params(radius)
    out, st = np.empty(shape, dtype=np.float64), defs.GdptSelectStats()
    sel = np.empty((h, w), dtype=np.int32) if maps else None
    mse = np.empty((h, w), dtype=np.float64) if maps else None
    Ej = np.empty((n, h, w), dtype=np.float64) if E else None
    host = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None      # noqa: E731
    _check(lib().gdpt_filter_select(int(w), int(h), n, _pointer_array([a.ctypes.data for a in FA]), _pointer_array([a.ctypes.data for a in FB]),
                                    _pointer_array([a.ctypes.data for a in T]), *[host(a) for a in halves], C.byref(p), host(out), host(sel),
                                    host(mse), host(Ej), C.byref(st)))
    if not maps:
        return out, st
    return (out, sel, mse, Ej, st) if E else (out, sel, mse, st)


def filter_select_device(width, height, FA_ptrs, FB_ptrs, T_ptrs, uA_ptr, vA_ptr, uB_ptr, vB_ptr, out_ptr, sel_ptr=None, mse_ptr=None, E_ptr=None,
                         stream=None, stats=True, params=None, radius=None):
    """filter_select() on device addresses (gdpt_filter_select_device); `FA_ptrs`, `FB_ptrs`, `T_ptrs` are sequences of n addresses.
    `sel_ptr` (int32, W*H), `mse_ptr` (W*H) and `E_ptr` (n*W*H) may be None. Returns GdptSelectStats after waiting for `stream`; with
    `stats=False` the call only enqueues and returns None."""
    if len(FA_ptrs) != len(T_ptrs) or len(FB_ptrs) != len(T_ptrs):
        raise GdptError("filter_select_device: FA_ptrs, FB_ptrs and T_ptrs must hold one address per candidate each")
    p = params if params is not None else select_params(radius)
    st = defs.GdptSelectStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_filter_select_device(int(width), int(height), len(T_ptrs), _pointer_array(FA_ptrs), _pointer_array(FB_ptrs),
                                           _pointer_array(T_ptrs), opt(uA_ptr), opt(vA_ptr), opt(uB_ptr), opt(vB_ptr), C.byref(p), opt(out_ptr),
                                           opt(sel_ptr), opt(mse_ptr), opt(E_ptr), opt(stream), C.byref(st) if stats else None))
    return st


_KINDS = {"plain": defs.DENOISE_PLAIN, "guided": defs.DENOISE_GUIDED, "demod": defs.DENOISE_DEMOD}


def _kind(who, kind):
    """The GDPT_DENOISE_* value of "plain", "guided" or "demod"; an int is passed on as it is (the library refuses an unknown one)."""
    if isinstance(kind, str):
        if kind not in _KINDS:
            raise GdptError(f'{who}: kind must be "plain", "guided" or "demod"')
        return _KINDS[kind]
    return int(kind)


def _level_arrays(who, img, var, feat, feat_var):
    """A level's host arrays as C-contiguous float64: HxWx3 twice, and (num_channels, H, W) twice or (None, None)."""
    a = np.ascontiguousarray(img, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or v.shape != a.shape:
        raise GdptError(f"{who}: img and var must be HxWx3 arrays of one shape")
    if feat is None and feat_var is None:
        return a, v, None, None
    if feat is None or feat_var is None:
        raise GdptError(f"{who}: feat and feat_var go together")
    f = np.ascontiguousarray(feat, dtype=np.float64)
    fv = np.ascontiguousarray(feat_var, dtype=np.float64)
    if f.ndim != 3 or f.shape != fv.shape or f.shape[1:] != a.shape[:2]:
        raise GdptError(f"{who}: feat and feat_var must be (num_channels, H, W) arrays of one shape")
    return a, v, f, fv


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _ref(block):
    return C.byref(block) if block is not None else None


def nlm_pyramid_down(img, var, feat=None, feat_var=None, kind="plain", guide=None, demod=None):
    """The next coarser level of a multi-scale non-local-means call on the GPU (gdpt_nlm_pyramid_down): every 2 x 2 cell's mean of
    `img` and of the planes `feat`, and mean / n of `var` and `feat_var`, over the n pixels of the cell that are valid for the `kind`
    ("plain", "guided", "demod") with its blocks `guide`, `demod` (None: as the library reads a NULL block for the kind); NaN where
    n = 0. Returns (img', var', feat', feat_var', GdptNlmPyramidOpStats) of ((H + 1) // 2, (W + 1) // 2); the planes are None
    without `feat`."""
    a, v, f, fv = _level_arrays("nlm_pyramid_down", img, var, feat, feat_var)
    h, w = a.shape[:2]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    oi, ov = np.empty((hc, wc, 3), dtype=np.float64), np.empty((hc, wc, 3), dtype=np.float64)
    of, ofv = (np.empty((f.shape[0], hc, wc), dtype=np.float64), np.empty((f.shape[0], hc, wc), dtype=np.float64)) if f is not None else (None, None)
    st = defs.GdptNlmPyramidOpStats()
    _check(lib().gdpt_nlm_pyramid_down(w, h, _vp(a), _vp(v), _vp(f), _vp(fv), int(f.shape[0]) if f is not None else 0, _kind("nlm_pyramid_down", kind),
                                       _ref(guide), _ref(demod), _vp(oi), _vp(ov), _vp(of), _vp(ofv), C.byref(st)))
    return oi, ov, of, ofv, st


def nlm_pyramid_down_device(width, height, img_ptr, var_ptr, img_out_ptr, var_out_ptr, feat_ptr=None, feat_var_ptr=None, feat_out_ptr=None,
                            feat_var_out_ptr=None, num_channels=0, kind="plain", guide=None, demod=None, stream=None, stats=True):
    """nlm_pyramid_down() on device addresses (gdpt_nlm_pyramid_down_device). Returns GdptNlmPyramidOpStats after waiting for `stream`;
    with `stats=False` the call only enqueues and returns None."""
    st = defs.GdptNlmPyramidOpStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_nlm_pyramid_down_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), int(num_channels),
                                              _kind("nlm_pyramid_down_device", kind), _ref(guide), _ref(demod), opt(img_out_ptr), opt(var_out_ptr),
                                              opt(feat_out_ptr), opt(feat_var_out_ptr), opt(stream), C.byref(st) if stats else None))
    return st


def nlm_pyramid_up(img, var, filtered, coarse_out, feat=None, feat_var=None, kind="plain", guide=None, demod=None):
    """A filtered coarser level put back into a filtered finer one on the GPU (gdpt_nlm_pyramid_up): `filtered` (HxWx3, the kind's
    filter on this level) plus the bilinear interpolation of `coarse_out` - (the down mean of `filtered`), `coarse_out` the combined
    output of the next coarser level. `img`, `var`, `feat`, `feat_var`: this level's inputs, read for validity; an invalid pixel
    keeps the bits of `img`. Returns (HxWx3 combined output, GdptNlmPyramidOpStats)."""
    a, v, f, fv = _level_arrays("nlm_pyramid_up", img, var, feat, feat_var)
    h, w = a.shape[:2]
    fl = np.ascontiguousarray(filtered, dtype=np.float64)
    co = np.ascontiguousarray(coarse_out, dtype=np.float64)
    if fl.shape != a.shape or co.shape != ((h + 1) // 2, (w + 1) // 2, 3):
        raise GdptError("nlm_pyramid_up: filtered must have the shape of img, coarse_out that of the next coarser level")
    out, st = np.empty(a.shape, dtype=np.float64), defs.GdptNlmPyramidOpStats()
    _check(lib().gdpt_nlm_pyramid_up(w, h, _vp(a), _vp(v), _vp(f), _vp(fv), int(f.shape[0]) if f is not None else 0, _kind("nlm_pyramid_up", kind),
                                     _ref(guide), _ref(demod), _vp(fl), _vp(co), _vp(out), C.byref(st)))
    return out, st


def nlm_pyramid_up_device(width, height, img_ptr, var_ptr, filtered_ptr, coarse_out_ptr, out_ptr, feat_ptr=None, feat_var_ptr=None, num_channels=0,
                          kind="plain", guide=None, demod=None, stream=None, stats=True):
    """nlm_pyramid_up() on device addresses (gdpt_nlm_pyramid_up_device); `stats` as nlm_pyramid_down_device."""
    st = defs.GdptNlmPyramidOpStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_nlm_pyramid_up_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr), int(num_channels),
                                            _kind("nlm_pyramid_up_device", kind), _ref(guide), _ref(demod), opt(filtered_ptr), opt(coarse_out_ptr),
                                            opt(out_ptr), opt(stream), C.byref(st) if stats else None))
    return st


def denoise_nlm_multiscale(img, var, feat=None, feat_var=None, kind="plain", levels=2, guide=None, demod=None, **params):
    """A multi-scale (pyramid) form of denoise_nlm ("plain"), denoise_nlm_guided ("guided") or denoise_nlm_demod ("demod") on the GPU
    (gdpt_denoise_nlm_multiscale): the kind's filter runs on `levels` (1 - 4) levels of a 2 x 2 mean pyramid and each level's low
    frequencies are replaced by the filtered coarser level, which removes the noise a single window cannot reach. `guide`, `demod`:
    None = as the library reads a NULL block for the kind (guided: the default guide; demod: the default block, no feature term);
    `params`: the keywords of nlm_params. Returns (HxWx3 filtered image, HxWx3 variance of the finest level's filter, in which the
    correction is ignored, GdptNlmPyramidStats). levels=1 is the kind's single-scale filter, bit for bit."""
    a, v, f, fv = _level_arrays("denoise_nlm_multiscale", img, var, feat, feat_var)
    out, var_out = np.empty(a.shape, dtype=np.float64), np.empty(a.shape, dtype=np.float64)
    p, st = nlm_params(**params), defs.GdptNlmPyramidStats()
    _check(lib().gdpt_denoise_nlm_multiscale(int(a.shape[1]), int(a.shape[0]), _vp(a), _vp(v), _vp(f), _vp(fv), int(f.shape[0]) if f is not None else 0,
                                             _kind("denoise_nlm_multiscale", kind), int(levels), C.byref(p), _ref(guide), _ref(demod), _vp(out),
                                             _vp(var_out), C.byref(st)))
    return out, var_out, st


def denoise_nlm_multiscale_device(width, height, img_ptr, var_ptr, out_ptr, var_out_ptr=None, feat_ptr=None, feat_var_ptr=None, num_channels=0,
                                  kind="plain", levels=2, guide=None, demod=None, stream=None, stats=True, params=None, **kw):
    """denoise_nlm_multiscale() on device addresses (gdpt_denoise_nlm_multiscale_device); `var_out_ptr` may be None. `params`: a
    GdptNlmParams taken as it is (else the keywords of nlm_params). Returns GdptNlmPyramidStats after waiting for `stream`; with
    `stats=False` the call only enqueues and returns None."""
    p = params if params is not None else nlm_params(**kw)
    st = defs.GdptNlmPyramidStats() if stats else None
    opt = lambda x: C.c_void_p(int(x)) if x else None      # noqa: E731
    _check(lib().gdpt_denoise_nlm_multiscale_device(int(width), int(height), opt(img_ptr), opt(var_ptr), opt(feat_ptr), opt(feat_var_ptr),
                                                    int(num_channels), _kind("denoise_nlm_multiscale_device", kind), int(levels), C.byref(p), _ref(guide),
                                                    _ref(demod), opt(out_ptr), opt(var_out_ptr), opt(stream), C.byref(st) if stats else None))
    return st


def _ptr_table(ptrs):
    """3 addresses (None or 0 entries: not wanted) as the `double *const [3]` of the C ABI; None: a NULL table."""
    if ptrs is None:
        return None
    arr = (C.c_void_p * 3)()
    for i in range(3):
        arr[i] = int(ptrs[i]) if i < len(ptrs) and ptrs[i] else None
    return arr


def reconstruct_weighted(width, height, c, gx, gy, var_c, var_gx, var_gy, dataCost=0.04, norm=defs.RECON_L2, conf_floor=0.0,
                         confidence=False, **params):
    """Variance-weighted reconstruction on the GPU (gdpt_reconstruct_weighted): every residual row weighted by a confidence
    s / (v + conf_floor s) from the variance v of its input; RECON_L2 = one weighted solve, RECON_L1 = weighted IRLS (`params`: the
    keywords of recon_params). Inputs HxWx3 float64. Returns (image, GdptWeightedReconStats), or with `confidence=True`
    (image, HxWx3 confidences of the data, x-edge and y-edge rows, stats)."""
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(height, width, 3) for x in (c, gx, gy, var_c, var_gx, var_gy)]
    out = np.empty((height, width, 3), dtype=np.float64)
    planes = [np.empty((height, width), dtype=np.float64) for _ in range(3)] if confidence else None
    p, st = weighted_recon_params(norm, conf_floor, **params), defs.GdptWeightedReconStats()
    _check(lib().gdpt_reconstruct_weighted(int(width), int(height), *[_dp(x) for x in a], float(dataCost), C.byref(p), _dp(out),
                                           _ptr_table([x.ctypes.data for x in planes] if confidence else None), C.byref(st)))
    return (out, np.stack(planes, axis=2), st) if confidence else (out, st)


def reconstruct_weighted_device(width, height, c_ptr, gx_ptr, gy_ptr, var_c_ptr, var_gx_ptr, var_gy_ptr, out_ptr, dataCost=0.04,
                                norm=defs.RECON_L2, conf_floor=0.0, confidence_ptrs=None, stream=None, **params):
    """reconstruct_weighted() on device addresses (gdpt_reconstruct_weighted_device); `confidence_ptrs`: 3 device addresses of W*H
    doubles (or None). Returns GdptWeightedReconStats. Waits for `stream`."""
    p, st = weighted_recon_params(norm, conf_floor, **params), defs.GdptWeightedReconStats()
    ins = [C.c_void_p(int(x)) for x in (c_ptr, gx_ptr, gy_ptr, var_c_ptr, var_gx_ptr, var_gy_ptr)]
    _check(lib().gdpt_reconstruct_weighted_device(int(width), int(height), *ins, float(dataCost), C.byref(p), C.c_void_p(int(out_ptr)),
                                                  _ptr_table(confidence_ptrs), C.c_void_p(int(stream) if stream else 0), C.byref(st)))
    return st


def assemble_device(width, height, src_ptrs, dst_ptrs, stream=None, rows=(0, 0)):
    """c, cx, cy from the five accumulation buffers (src/render.cpp:340-350); `rows` = the band this rank owns."""
    _check(lib().gdpt_assemble_rows_device(int(width), int(height), int(rows[0]), int(rows[1]),
                                           *[C.c_void_p(int(x)) for x in src_ptrs],
                                           *[C.c_void_p(int(x)) for x in dst_ptrs], C.c_void_p(int(stream) if stream else 0)))


def band_rows(height, num_bands, band):
    """Rows [r0, r1) of one band of the sharded tile loop, as the C host computes them (gdpt_band_rows)."""
    r0, r1 = C.c_int32(), C.c_int32()
    _check(lib().gdpt_band_rows(int(height), int(num_bands), int(band), C.byref(r0), C.byref(r1)))
    return r0.value, r1.value


def band_rows_weighted(height, num_bands, band, costs):
    """Rows [r0, r1) of one band of a cost-balanced sharding, as the C host computes them (gdpt_band_rows_weighted)."""
    r0, r1 = C.c_int32(), C.c_int32()
    arr = (C.c_double * len(costs))(*[float(c) for c in costs])
    _check(lib().gdpt_band_rows_weighted(int(height), int(num_bands), int(band), arr, len(costs), C.byref(r0), C.byref(r1)))
    return r0.value, r1.value


def band_rows_from_row_costs(height, num_bands, band, row_costs, granularity=1):
    """Rows [r0, r1) of one band of a sharding balanced on per-row costs, as the C host computes them (gdpt_band_rows_from_row_costs;
    mirror: sharding.bands_from_row_costs)."""
    r0, r1 = C.c_int32(), C.c_int32()
    arr = (C.c_double * len(row_costs))(*[float(c) for c in row_costs])
    if len(row_costs) != int(height):
        raise ValueError("one cost per pixel row expected")
    _check(lib().gdpt_band_rows_from_row_costs(int(height), int(num_bands), int(band), arr, int(granularity), C.byref(r0), C.byref(r1)))
    return r0.value, r1.value


class MultiScene:
    """The scene uploaded to several devices of one node, tile loop sharded into row bands (include/gdpt.h,
    gdpt_multi_*): replaces the reference's thread pool over tiles (src/parallel.cpp:183-256)."""

    def __init__(self, scene_desc, devices, exchange=defs.EXCHANGE_RCCL, balance=False):
        self.desc = scene_desc
        self.width, self.height = scene_desc.width, scene_desc.height
        cfg = defs.GdptMultiConfig()
        cfg.num_devices, cfg.exchange, cfg.balance = len(devices), int(exchange), int(bool(balance))
        for i, d in enumerate(devices):
            cfg.devices[i] = int(d)
        h = C.c_void_p()
        _check(lib().gdpt_multi_create(scene_desc.ptr, C.byref(cfg), C.byref(h)))
        self.handle = h

    def gradient_path_render(self, spp=0, rng_scheme=defs.RNG_SAMPLE, alpha=0.04, return_buffers=False, shift=defs.SHIFT_REFERENCE):
        shape = (self.height, self.width, 3)
        out = np.zeros(shape, dtype=np.float64)
        bufs = {k: np.zeros(shape, dtype=np.float64) for k in ("img", "cx0", "cy0", "cx1", "cy1")}
        rs, ms = defs.GdptRenderStats(), defs.GdptMultiStats()
        p = _params(spp, rng_scheme, (0, 0), shift=shift)
        _check(lib().gdpt_multi_gradient_path_render(self.handle, C.byref(p), float(alpha), _dp(out),
                                                     _dp(bufs["img"]), _dp(bufs["cx0"]), _dp(bufs["cy0"]), _dp(bufs["cx1"]), _dp(bufs["cy1"]),
                                                     C.byref(rs), C.byref(ms)))
        return (out, bufs, rs, ms) if return_buffers else out

    def rebalance(self, band_ms, granularity=1):
        """Feedback between frames (gdpt_multi_rebalance): `band_ms` = GdptMultiStats.render_ms of the last call; the bands are cut
        again on the corrected cost model, at multiples of `granularity` rows."""
        arr = (C.c_double * len(band_ms))(*[float(t) for t in band_ms])
        _check(lib().gdpt_multi_rebalance(self.handle, arr, int(granularity)))

    def close(self):
        if getattr(self, "handle", None):
            lib().gdpt_multi_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def poisson_forget_stream(stream):
    """Drops the solver scratch kept for `stream` on the current device (gdpt_poisson_forget_stream): call before destroying a
    stream the solver has run on."""
    _check(lib().gdpt_poisson_forget_stream(C.c_void_p(int(stream) if stream else 0)))


def poisson_solve_device(width, height, c_ptr, gx_ptr, gy_ptr, out_ptr, alpha=0.04, solver=defs.SOLVER_DEFAULT, tol=0.0,
                         max_iters=0, stream=None, want_stats=False):
    st = defs.GdptPoissonStats() if want_stats else None
    _check(lib().gdpt_poisson_solve_device(int(width), int(height), C.c_void_p(int(c_ptr)), C.c_void_p(int(gx_ptr)),
                                           C.c_void_p(int(gy_ptr)), float(alpha), C.c_void_p(int(out_ptr)), int(solver),
                                           float(tol), int(max_iters), C.c_void_p(int(stream) if stream else 0),
                                           C.byref(st) if st is not None else None))
    return st


def assemble_solve_device(width, height, src_ptrs, dst_ptrs, out_ptr, alpha=0.04, solver=defs.SOLVER_DEFAULT, tol=0.0, max_iters=0,
                          stream=None, want_stats=False):
    """assemble_device over the whole film + poisson_solve_device on its outputs as one call (gdpt_assemble_solve_device): the
    assembly and the solver's right-hand side are one pass over the film. `src_ptrs` = img, cx0, cy0, cx1, cy1; `dst_ptrs` = c, cx, cy."""
    st = defs.GdptPoissonStats() if want_stats else None
    _check(lib().gdpt_assemble_solve_device(int(width), int(height), *[C.c_void_p(int(x)) for x in src_ptrs], *[C.c_void_p(int(x)) for x in dst_ptrs],
                                            float(alpha), C.c_void_p(int(out_ptr)), int(solver), float(tol), int(max_iters),
                                            C.c_void_p(int(stream) if stream else 0), C.byref(st) if st is not None else None))
    return st


def imwrite(filename, image):
    """.pfm (fp32) / .exr (fp16) by suffix, like src/image.cpp:135-173."""
    img = np.ascontiguousarray(image, dtype=np.float64)
    h, w, _ = img.shape
    _check(lib().gdpt_imwrite(os.fsencode(filename), w, h, _dp(img)))


def imread(filename, channels=3):
    """imread3 / imread1 of the reference (src/image.cpp:26-133): HxWxC float64 texels."""
    w, h = C.c_int(), C.c_int()
    p = C.POINTER(C.c_double)()
    _check(lib().gdpt_imread(os.fsencode(filename), int(channels), C.byref(w), C.byref(h), C.byref(p)))
    try:
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, int(channels))).copy()
    finally:
        lib().gdpt_image_free(p)
    return a


def bvh_check(bounds):
    """Builds + verifies the traversal trees over n fp32 boxes (n x 6: min xyz, max xyz); host only.
    Returns the stats dict of gdpt_bvh_check (include/gdpt.h)."""
    b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1, 6)
    st = (C.c_int32 * 8)()
    _check(lib().gdpt_bvh_check(b.ctypes.data_as(C.POINTER(C.c_float)), b.shape[0], st))
    return dict(zip(("bvh2_nodes", "bvh2_depth", "wide_nodes", "wide_arity", "wide_stack_need", "leaves", "max_leaf_prims", "bvh8_nodes"), list(st)[:8]))


def sbvh_check(tri_verts, budget=0.3, samples_per_tri=16):
    """Builds the BVH with spatial splits over n fp32 triangles (n x 3 x 3) and verifies it incl. coverage by point sampling;
    host only. Returns the stats dict of gdpt_sbvh_check (include/gdpt.h)."""
    t = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
    st = (C.c_int32 * 8)()
    _check(lib().gdpt_sbvh_check(t.ctypes.data_as(C.POINTER(C.c_float)), t.shape[0], C.c_double(budget), int(samples_per_tri), st))
    d = dict(zip(("bvh2_nodes", "bvh2_depth", "references", "wide_nodes", "wide_stack_need", "leaves"), list(st)[:6]))
    d["sah_nodes"] = st[6] / 1000.0; d["sah_prims"] = st[7] / 1000.0
    return d


def shape_triangles(scene_desc):
    """fp32 vertices of every triangle of a SceneDesc (T x 3 x 3), in shape order."""
    d = scene_desc.desc
    out = []
    for i in range(d.num_shapes):
        sh = d.shapes[i]
        if sh.num_triangles <= 0:
            continue
        pos = np.ctypeslib.as_array(sh.positions, shape=(sh.num_vertices, 3)).astype(np.float32)
        idx = np.ctypeslib.as_array(sh.indices, shape=(sh.num_triangles, 3))
        out.append(pos[idx])
    return np.concatenate(out, axis=0) if out else np.zeros((0, 3, 3), np.float32)


def shape_triangle_bounds(scene_desc):
    """fp32 boxes of every triangle of a SceneDesc, in shape order (what gdpt_scene_upload hands its BVH builder)."""
    d = scene_desc.desc
    out = []
    for i in range(d.num_shapes):
        sh = d.shapes[i]
        if sh.num_triangles <= 0:
            continue
        pos = np.ctypeslib.as_array(sh.positions, shape=(sh.num_vertices, 3)).astype(np.float32)
        idx = np.ctypeslib.as_array(sh.indices, shape=(sh.num_triangles, 3))
        tri = pos[idx]                                   # T x 3 x 3
        out.append(np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1))
    return np.concatenate(out, axis=0) if out else np.zeros((0, 6), np.float32)


class debug_knobs:
    """Test instrument (include/gdpt_debug.h): `with debug_knobs(force_eager=1, log2k=0): ...` forces an alternative
    schedule for the calls inside the block and restores the product path afterwards. The library reads no environment
    variable; manual sweep scripts under tests/ that take their settings from GDPT_* variables translate them through
    debug_knobs.from_env() explicitly."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            _check(lib().gdpt_debug_knob_set(k.encode(), float(v)))
        return self

    def __exit__(self, *exc):
        lib().gdpt_debug_knobs_reset()
        return False

    @staticmethod
    def set(**knobs):
        for k, v in knobs.items():
            _check(lib().gdpt_debug_knob_set(k.encode(), float(v)))

    @staticmethod
    def reset():
        lib().gdpt_debug_knobs_reset()

    @staticmethod
    def chunk_plan(spp, film_pixels, resident_lanes=256 * 2 * 256, force_log2k=-1):
        """Sample ranges of a pixel's work items: [begin[c], begin[c+1]) (include/gdpt_debug.h)."""
        buf = (C.c_int32 * 80)()
        n = lib().gdpt_debug_chunk_plan(int(spp), int(force_log2k), int(film_pixels), int(resident_lanes), buf, 80)
        if n < 0:
            raise GdptError("gdpt_debug_chunk_plan: capacity")
        return list(buf)[:n + 1]

    @staticmethod
    def stamps():
        """Per-segment wave cycles of the last render made under debug_knobs(stamps=1) (include/gdpt_debug.h)."""
        v = (C.c_double * 16)()
        lib().gdpt_debug_get_stamps(v)
        d = dict(zip(("loop_head", "trace", "vertex", "consume", "bsdf", "finish", "camera", "wave_steps", "publish", "take", "item"), list(v)))
        d["busy_us"] = (v[13] - v[12]) / 100.0      # first wave started -> first wave found the queue empty
        d["drain_us"] = (v[14] - v[13]) / 100.0     # ... -> last wave ended
        return d

    @staticmethod
    def setup_passes():
        """Full-width passes of the sample set-up in the last render made under debug_knobs(stamps=1), over all waves (slot 11 of
        gdpt_debug_get_stamps; stamps()["wave_steps"] is the count to set it against)."""
        v = (C.c_double * 16)()
        lib().gdpt_debug_get_stamps(v)
        return v[11]

    @staticmethod
    def last_route():
        """Kernel route of this thread's last render (include/gdpt_debug.h: gdpt_debug_last_route)."""
        return lib().gdpt_debug_last_route().decode()

    @staticmethod
    def last_dct_shape():
        """Shape of the folded GEMMs of this thread's last GDPT_SOLVER_DCT_MFMA solve (include/gdpt_debug.h: gdpt_debug_last_dct_shape)."""
        return lib().gdpt_debug_last_dct_shape().decode()

    @staticmethod
    def route_names():
        """Every route name the library can report (include/gdpt_debug.h: gdpt_debug_route_names)."""
        n = lib().gdpt_debug_route_names(None, 0)
        buf = (C.c_char_p * n)()
        if lib().gdpt_debug_route_names(buf, n) != n:
            raise GdptError("gdpt_debug_route_names: capacity")
        return [x.decode() for x in buf]

    @staticmethod
    def image_grid(kernel, width, height):
        """(blocks launched, units of work they stride over) of an image-space launch on a width x height film, as the launch
        computes them (include/gdpt_debug.h: gdpt_debug_image_grid). No GPU call."""
        out = (C.c_int32 * 2)()
        _check(lib().gdpt_debug_image_grid(kernel.encode(), int(width), int(height), out))
        return int(out[0]), int(out[1])

    @staticmethod
    def prepare_scene(scene_desc):
        """The host half of an upload of `scene_desc`, on the CPU (include/gdpt_debug.h: gdpt_debug_prepare_scene): a dict of the
        traits and scalars, `count` and `digest` by table name, and the emitter selection table `light_pmf`, `light_cdf`."""
        n = scene_desc.desc.num_lights
        info = defs.GdptPreparedInfo()
        pmf, cdf = np.zeros(n + 1), np.zeros(n + 1)
        _check(lib().gdpt_debug_prepare_scene(scene_desc.ptr, C.byref(info), _dp(pmf), _dp(cdf), n + 1))
        d = {k: getattr(info, k) for k, _ in defs.GdptPreparedInfo._fields_ if k not in ("count", "digest", "bounds", "leaf_hist")}
        d["bounds"], d["leaf_hist"] = list(info.bounds), list(info.leaf_hist)
        d["count"] = dict(zip(defs.PREPARED_TABLES, info.count))
        d["digest"] = dict(zip(defs.PREPARED_TABLES, info.digest))
        have = d["count"]["light_pmf"]                   # (a scene without emitters has no table)
        d["light_pmf"], d["light_cdf"] = pmf[:have], cdf[:have + 1 if have else 0]
        return d

    @staticmethod
    def kat_variants(family):
        """The family's table of variants (include/gdpt_debug.h: gdpt_debug_kat_variants): a list of dicts, in the order the
        `variant` argument of kat() indexes. No GPU call."""
        n = lib().gdpt_debug_kat_variants(family.encode(), None, 0)
        if n < 0:
            raise GdptError(lib().gdpt_last_error().decode("utf-8", "replace"))
        rows = (defs.GdptKatVariant * n)()
        if lib().gdpt_debug_kat_variants(family.encode(), rows, n) != n:
            raise GdptError(lib().gdpt_last_error().decode("utf-8", "replace"))
        return [{"name": r.name.decode(), "mask": int(r.mask), "rough": bool(r.rough), "twosided": bool(r.twosided),
                 "inline_lambert": bool(r.inline_lambert), "plain": int(r.plain)} for r in rows]

    @staticmethod
    def kat(scene, family, variant, queries):
        """Runs one device function family on an array of cases (include/gdpt_debug.h: gdpt_debug_kat_<family>). `queries`: a ctypes
        array of the family's query struct (defs.KAT_STRUCTS); returns the ctypes array of results."""
        result = defs.KAT_STRUCTS[family][1]
        out = (result * max(1, len(queries)))()
        _check(getattr(lib(), "gdpt_debug_kat_" + family)(scene.handle, int(variant), len(queries), queries, out))
        return out

    @staticmethod
    def kat_trace_variants():
        """The rows of the "trace" family (include/gdpt_debug.h: gdpt_debug_kat_trace_variants): a list of dicts, in the order the
        `variant` argument of kat_trace() indexes. No GPU call."""
        n = lib().gdpt_debug_kat_trace_variants(None, 0)
        rows = (defs.GdptKatTraceVariant * max(1, n))()
        if n < 0 or lib().gdpt_debug_kat_trace_variants(rows, n) != n:
            raise GdptError(lib().gdpt_last_error().decode("utf-8", "replace"))
        return [{"name": r.name.decode(), **{k: int(getattr(r, k)) for k, _ in defs.GdptKatTraceVariant._fields_[1:]}} for r in rows[:n]]

    @staticmethod
    def kat_trace(scene, variant, queries):
        """Walks one row of the "trace" family over a ctypes array of GdptKatTraceQuery (include/gdpt_debug.h: gdpt_debug_kat_trace);
        returns the ctypes array of GdptKatTraceResult."""
        out = (defs.GdptKatTraceResult * max(1, len(queries)))()
        _check(lib().gdpt_debug_kat_trace(scene.handle, int(variant), len(queries), queries, out))
        return out

    @staticmethod
    def from_env(environ=None):
        """GDPT_FORCE_EAGER=1 -> force_eager=1 ... for the manual sweep scripts (tests/sweep_*.py, tune_render.py)."""
        environ = os.environ if environ is None else environ
        names = ("force_eager", "log2k", "keep_frac", "search_frac", "blocks_per_cu", "no_lds_scene", "lds_wide",
                 "no_twosided_machine", "presplit", "presplit_floor", "bvh_leaf_max", "bvh_leaf_factor", "sbvh", "sbvh_alpha", "plan_rounds", "plan_shrink", "plan_digits", "bvh_collapse_dp", "stamps", "wavefront", "wf_slots", "wf_sort", "multi_fail_band", "multi_fail_stage", "dct_bk", "dct_bm", "full_material_switch", "no_plain_kernel", "replay_per_step", "no_render_overlap", "whole_leaf_trips", "no_setup_batch", "nlm_direct", "lds_fixed_layout", "nlm_collab_pass")
        lib().gdpt_debug_knobs_reset()
        for n in names:
            v = environ.get("GDPT_" + n.upper())
            if v is not None:
                _check(lib().gdpt_debug_knob_set(n.encode(), float(v)))


def build_arch():
    return lib().gdpt_build_arch().decode()
