// nlm_regress.h — a first-order feature regression on the non-local-means weights (nlm_regress.hip; include/gdpt.h:
// gdpt_denoise_nlm_regress*).
#pragma once
#include "../../../include/gdpt.h"
#include "device_mem.h"

#include <string>

namespace gdpt {

// What every entry point refuses in a regression block beside a guide of `num_channels` planes; the message names the field. `who`
// names the caller. Host only.
void nlm_check_regress(const std::string &who, const GdptNlmRegress &r, int num_channels);

// The blocks in force of a regression call (the collaborative form's too), and what the entry points refuse: the films, the blocks, an
// output aliasing an input; `who` names the caller. var_out nullable. Host only.
struct NlmRegressBlocks {
    GdptNlmParams p; GdptNlmGuide g; GdptNlmRegress rg;
    bool planes() const { return g.num_groups > 0 || rg.num_regressors > 0; }      // whether a group or a regressor reads a feature plane
    size_t feature_elems(int width, int height) const { return planes() ? (size_t)width * height * g.num_channels : 0; }      // doubles of feat, of feat_var
};
NlmRegressBlocks nlm_regress_check_arguments(const std::string &who, int width, int height, const double *img, const double *var, const double *feat,
                                             const double *feat_var, const GdptNlmParams *params, const GdptNlmGuide *guide,
                                             const GdptNlmRegress *regress, const double *out, const double *var_out);

// The regression on device pointers of the current device, every argument checked (the session's entry point). Enqueued on `stream`;
// waits for it if `stats` is asked for. Launch geometry: film::tile_grid over tiles of kNlmTile x kNlmTile pixels (denoise_nlm.h);
// the scratch is kept per (device, stream), and dropped by forget_stream (device_mem.h).
void denoise_nlm_regress_launch(int w, int h, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                const GdptNlmParams &p, const GdptNlmGuide &g, const GdptNlmRegress &rg, double *d_out, double *d_var_out,
                                hipStream_t stream, GdptNlmStats *stats);

} // namespace gdpt
