// denoise_nlm.h — non-local means on a mean and the variance of that mean (denoise_nlm.hip; include/gdpt.h: gdpt_denoise_nlm*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a parameter block; the message names the field. `who` names the caller. Host only.
void nlm_check_params(const std::string &who, const GdptNlmParams &p);

// The same for the guide of the guided entry points (gdpt_denoise_nlm_guided*).
void nlm_check_guide(const std::string &who, const GdptNlmGuide &g);
// The guided filter on device pointers of the current device, every argument checked (the session's entry point). Enqueued on
// `stream`; waits for it if `stats` is asked for.
void denoise_nlm_guided_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               const GdptNlmParams &p, const GdptNlmGuide &g, double *d_out, double *d_var_out, hipStream_t stream,
                               GdptNlmStats *stats);

// The same for the block of the demodulated entry points (gdpt_denoise_nlm_demod*), whose planes number `num_channels`.
void nlm_check_demod(const std::string &who, const GdptNlmDemod &d, int num_channels);
// The demodulated filter on device pointers of the current device, every argument checked (the session's entry point); `g` nullable: no
// feature term. Enqueued on `stream`; waits for it if `stats` is asked for.
void denoise_nlm_demod_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                              const GdptNlmParams &p, const GdptNlmGuide *g, const GdptNlmDemod &d, double *d_out, double *d_var_out,
                              hipStream_t stream, GdptNlmStats *stats);

// The joint filter (nlm_joint.hip; gdpt_denoise_nlm_joint*). What its entry points refuse, with the field named; fills the parameters
// and the guide in force. Host only.
void nlm_joint_check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                               const double *feat_var, int n, const double *const *comp, const double *const *comp_var,
                               const GdptNlmParams *params, const GdptNlmGuide *guide, const double *out, const double *var_out,
                               double *const *comp_out, double *const *comp_var_out, GdptNlmParams &p, GdptNlmGuide &g);
// ... on device pointers of the current device, every argument checked (the session's entry point); d_comp .. d_comp_var_out are host
// arrays of n device pointers, d_comp_var_out and its entries nullable. Enqueued on `stream`; waits for it if `stats` is asked for.
void denoise_nlm_joint_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var, int n,
                              const double *const *d_comp, const double *const *d_comp_var, const GdptNlmParams &p, const GdptNlmGuide &g,
                              double *d_out, double *d_var_out, double *const *d_comp_out, double *const *d_comp_var_out, hipStream_t stream,
                              GdptNlmJointStats *stats);

// Launch geometry of both kernel forms: film::tile_grid (image_kernels.h) over tiles of kNlmTile x kNlmTile pixels. The filter's
// scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
constexpr int kNlmTile = 16;

} // namespace gdpt
