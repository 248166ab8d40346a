/* gdpt_debug.h — test instrument, NOT part of the drop-in boundary of include/gdpt.h.
 *
 * The product entry points take every scheduling decision (which evaluator, how a pixel's samples are cut into work
 * items, whether a small scene is copied to LDS, BVH leaf policy ...) from the scene and the render parameters alone;
 * no environment variable is read anywhere in libgdpt.so. The parity tests, however, must be able to force the
 * alternatives (straight-loop evaluator vs lane machine, 1 / 2 / 8 work items per pixel, HBM walk of an LDS-sized
 * scene, a second BVH over the same triangles) to show that they agree. These two calls are that switchboard: a
 * process-global table of overrides, empty unless a test fills it. Nothing in lajolla, bench.py's timed region or the
 * library itself calls them.
 *
 * Knob names (value semantics in parentheses; an unknown name is an error):
 *   force_eager          (0/1)  straight per-sample loop instead of the lane machine
 *   log2k                (int)  work items (or lanes) per pixel = 2^value
 *   keep_frac            (0..255) trace phase is left when this fraction /256 of its rays is unfinished
 *   search_frac          (0..255) node loop is left when this fraction /256 of the live lanes still searches a leaf
 *   blocks_per_cu        (int)  persistent blocks per compute unit
 *   no_lds_scene         (0/1)  walk an LDS-sized scene from HBM
 *   lds_wide             (0/1)  LDS-resident scenes in BVH4 form (default 1)
 *   no_twosided_machine  (0/1)  two-sided lobes on the straight loop instead of the replay machine
 *   presplit             (real) triangle pre-split budget, extra references per primitive (scene upload)
 *   presplit_floor       (real) pre-split priority floor (scene upload)
 *   bvh_leaf_max         (1..4) SAH builder: primitives per leaf (scene upload)
 *   bvh_leaf_factor      (real) SAH builder: leaf cost factor (scene upload)
 *   sbvh                 (real) SAH builder with spatial splits: extra references allowed per primitive, 0 = object splits only (scene upload)
 *   plan_rounds          (1..8) work-item plan: rounds of items (one per resident lane) every size of the plan's shrinking tail lasts (default 4)
 *   plan_shrink          (10..90) work-item plan: percentage of the samples still unassigned that the next chunk takes (default 55)
 *   plan_digits          (int) work-item plan spelled out: decimal digits = chunk sizes (552211 = 5,5,2,2,1,1), used when they add up to the spp
 *   sbvh_alpha           (real) ... spatial splits are tried where the object split's children overlap by more than this fraction of the root's area
 *   wavefront            (0/1)  scenes walked from HBM, one-sided lobes: 1 = wavefront pipeline (step + trace kernels, path
 *                               state in HBM), 0 = lane machine; the two give bit-identical images
 *   wf_slots             (int)  wavefront pipeline: at most this many path slots (forces slots to run several items)
 *   wf_sort              (0/1/2) wavefront pipeline: ray queue in slot order / sorted by (octant, origin cell) / by (origin cell, octant)
 *   multi_fail_band / multi_fail_stage (int)  gdpt_multi_*: band `multi_fail_band` throws in stage 1 (render), 2 (halo +
 *                               assembly), 3 (all-gather) or 4 (solve): the other bands must stand down, not hang
 *   dct_bk (16 / 32), dct_bm (32 / 64)   GDPT_SOLVER_DCT_MFMA: force a shape of the folded GEMM (default: by grid size, and the
 *                               small-footprint shape beside a resident render kernel). dct_bm = 32 alone is the deep-prefetch 32-row shape;
 *                               dct_bm = 32 with dct_bk = 16 is the small-footprint shape (32 x 32 tile, 256 threads)
 *   lds_fixed_layout (0/1)      one-sided lane machine on an LDS-resident scene: the block takes the caps (12 stack levels, 20 KB of scene
 *                               copy) instead of the LDS its scene needs; same kernel, same route name
 *   replay_per_step (n >= 1)    two-sided lane machine: replay iterations of an offset per wave step (default 4; 1 = one per step)
 *   no_plain_kernel (0/1)       one-sided lane machine: the kernel with sphere and texture code even for a triangles-only, constant-texture scene
 *   no_render_overlap (0/1)     one-sided lane machine: every launch wholly on the caller's stream, none on the handle's render streams
 *   full_material_switch (0/1)  lane machines: the kernel with the full material switch even when the scene fits a small set
 *   whole_leaf_trips (0/1)      one-sided lane machine on an LDS-resident scene: the kernel whose leaf trips test the whole leaf (four
 *                               tests in a row) instead of two records per trip with the cursor in the leaf reference; same route name
 *   no_setup_batch (0/1)        route lambert_plain/lds_const (and its stamped build, lambert_stamped/lds_plain): the kernel whose camera block
 *                               makes each sample's set-up (stream seeding, two draws, pixel filter) in the step that needs it, instead
 *                               of ahead and at full wave width; same route name
 *   nlm_direct (0/1)            gdpt_denoise_nlm*: the direct form of the filter (one thread per pixel, every patch distance summed
 *                               from global memory: the literal definition) instead of the tiled form (a block's tile and halo
 *                               staged in LDS, separable patch sums). gdpt_denoise_atrous* picks a form per level: 0 the staged
 *                               form up to step 4 and the direct form beyond (the measured routes), 1 the direct form at every
 *                               step, 2 the staged form at every step that has one (1 - 8), for measurements; the other filters
 *                               read 2 as 1
 *   nlm_collab_pass (0/1/2)     gdpt_denoise_nlm_collab*, for measurements: 1 launches the fit alone (the coefficient film is written,
 *                               out is not), 2 the gather alone (on the coefficient film an earlier call left in the caller's d_coef);
 *                               0, the default, both
 *   stamps               (0/1)  Lambertian lane machine: the diagnostic build with in-kernel cycle stamps; a render with
 *                               stats then leaves its per-segment wave cycles for gdpt_debug_get_stamps
 *
 * Route names (gdpt_debug_last_route): the kernel a render launched, as `family/variant`. "lds" = the scene copied to
 * LDS (lds_wide: in its BVH4 form, lds_bvh2: BVH2), "hbm" = walked from HBM; "plain" / "const" = the build without sphere
 * and texture code, "tex" = without sphere code only; "env" = with the environment-map lookups.
 *   GradPath, GDPT_RNG_SAMPLE, GDPT_SHIFT_REFERENCE, one-sided lobes (lane machine with lazy offsets):
 *     lambert_plain/{lds_const, lds_tex, hbm_const, hbm_tex}   Lambertian, triangles only
 *     lambert/{lds_wide, lds_bvh2, hbm}                         Lambertian, with spheres (or an LDS scene in BVH2 form)
 *     lambert_stamped/{lds_plain, lds, hbm}                     the diagnostic build (knob stamps)
 *     general_set_a/{disney_diffuse, disney_metal}, general_set_b/{disney_clearcoat, disney_sheen}
 *                                                               HBM triangle scenes of Lambertian + that one lobe
 *     general/{lds_wide, lds_bvh2, hbm}                         the full material switch
 *     wavefront/{lambert, general}                              HBM scenes under the knob wavefront
 *   GradPath, two-sided lobes (DisneyGlass, DisneyBSDF), replay machine:
 *     twosided/{lds, hbm, hbm_glass}                            hbm_glass: Lambertian + DisneyGlass only
 *   GradPath, straight per-sample loops: eager (rough lobes; two-sided lobes whose depth bound outruns the replay's
 *     bounce log; knob force_eager), tile_eager (GDPT_RNG_TILE with rough or two-sided lobes)
 *   GradPath, GDPT_RNG_TILE, one-sided lobes: tile_phases_lambert, tile_phases_general
 *   GradPath, GDPT_SHIFT_RECONNECT: reconnect/{lds_lambert, hbm_lambert, general} (one general kernel, walked from HBM)
 *   Path: path/tile (GDPT_RNG_TILE), path/eager (knob force_eager), path_persistent/{lds_lambert_plain, lds_lambert,
 *     lds_lambert_env, hbm_lambert, hbm_lambert_env, lds_general, lds_general_env, hbm_general, hbm_general_env}
 */
#ifndef GDPT_DEBUG_H
#define GDPT_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Sets one override; returns 0, or non-zero (message in gdpt_last_error) for an unknown name. */
int gdpt_debug_knob_set(const char *name, double value);
/* Wave cycles per segment of the last stamped render (summed over waves): [0] loop head remainder, [1] traversal,
 * [2] hit-vertex rebuild, [3] state arms, [4] BSDF block, [5] offset / finish arm, [6] camera-ray block, [7] wave steps
 * (a count), [8] publishing finished items, [9] work-queue take, [10] item -> pixel mapping, [11] full-width passes of the sample
 * set-up (a count like [7]: per-wave table fills and on-demand passes; 0 under no_setup_batch and on other films than powers of two); wall clock
 * (s_memrealtime, 100 MHz ticks): [12] first wave started, [13] first wave found the queue empty, [14] last wave ended. */
void gdpt_debug_get_stamps(double out[16]);
/* The work-item plan of the persistent render kernels (make_chunk_plan, csrc/hip/render_kernels.hip): chunk c of a pixel
 * covers samples [begin[c], begin[c+1]). Returns the number of chunks (begin[] gets n + 1 entries), -1 if `capacity` is too
 * small. force_log2k < 0: the product plan. Host only. */
int gdpt_debug_chunk_plan(int spp, int force_log2k, long long film_pixels, long long resident_lanes, int32_t *begin, int capacity);
/* Route of the last gdpt_render / gdpt_path_render (and their _device forms) made by the CALLING thread: one of the
 * names above, "" before the first one (or after a render that failed before its launch). The string is static. */
const char *gdpt_debug_last_route(void);
/* Shape of the folded GEMMs of the last GDPT_SOLVER_DCT_MFMA solve enqueued by the CALLING thread: "64x64x32", "32x64x32", "64x64x16"
 * (block tile rows x columns x K step) or "32x32x16", the small-footprint shape a solve takes while a render kernel may be resident
 * beside it; "" before the first such solve. The string is static. */
const char *gdpt_debug_last_dct_shape(void);
/* Renders of this handle so far whose kernel went on one of the handle's own render streams (include/gdpt.h: gdpt_render_device);
 * -1 for a null handle. Lets a test see that the overlapped path was taken. */
struct GdptScene;
long long gdpt_debug_overlapped_launches(const struct GdptScene *scene);
/* Leaves of the binary BVH the upload built, by size: hist[k] = leaves of k + 1 primitive records. The wide forms the kernels walk
 * (BVH4, quantised BVH4, BVH8) are collapsed from that tree and keep its leaves as they are, so these are the leaves every kernel
 * meets. The root is an inner node whenever the scene has a primitive (a scene of one leaf hangs it under the root); a scene without
 * primitives gives zeros. Returns 0, or non-zero for a null argument. */
int gdpt_debug_leaf_histogram(const struct GdptScene *scene, int32_t hist[4]);
/* Every name gdpt_debug_last_route can return: fills out[0..n) and returns n, or -1 if `capacity` < n; out == NULL
 * returns n alone. */
int gdpt_debug_route_names(const char **out, int capacity);
/* The grid of an image-space launch on a film of width x height, as the launch itself computes it: out[0] = blocks launched (256
 * threads each), out[1] = units of work those blocks stride over (tiles, or groups of 256 consecutive pixels / elements). A block takes
 * a second trip of its work loop where out[1] > out[0]; the reduction of the per-block partials takes one where out[0] > 256. Names,
 * one per grid rule: "fold" (fold_kernel, merge_kernel: pixels), "variance" (variance_kernel: the 3 W H elements), "spread"
 * (spread_kernel: pixels), "box" (box_kernel: 32 x 8 tiles), "nlm" (both forms of the filter: 16 x 16 tiles), "recon_tiles" (the tile
 * kernels of the L1 and the variance-weighted reconstruction: 32 x 8 tiles), "recon_pixels" (pcg_step_b: pixels, on the grid of the
 * tile kernels), "cg" (the Poisson CG: the 3 W H elements). Makes no GPU call. Returns 0, or non-zero (message in gdpt_last_error)
 * for an unknown name, a null argument or an empty film. */
int gdpt_debug_image_grid(const char *kernel, int width, int height, int32_t out[2]);
/* The host half of a scene upload (csrc/host/scene_prepare.h: prepare_scene) on `desc`, with the default options of a product upload
 * and no knob applied; makes no GPU call, so it runs where there is none. `info` receives the table sizes, the traits that choose a
 * render's route, the intersection epsilon and a 64-bit FNV-1a digest of the bytes of every table (GDPT_PREPARED_* index it; an empty
 * table digests to the FNV offset basis). light_pmf / light_cdf (either may be NULL) receive the emitter selection table, num_lights
 * and num_lights + 1 entries; `capacity` = entries each of the two arrays can hold. Returns 0, or non-zero (message in
 * gdpt_last_error: the one gdpt_scene_upload gives for the same description) on error or when `capacity` is too small. */
enum { GDPT_PREPARED_NODES, GDPT_PREPARED_NODES4, GDPT_PREPARED_NODES8, GDPT_PREPARED_NODES4Q, GDPT_PREPARED_PRIMS, GDPT_PREPARED_TRIS,
       GDPT_PREPARED_SPHERES, GDPT_PREPARED_MATERIALS, GDPT_PREPARED_LIGHT_INTENSITY, GDPT_PREPARED_IMAGES, GDPT_PREPARED_TEXELS,
       GDPT_PREPARED_LIGHTS, GDPT_PREPARED_LIGHT_PMF, GDPT_PREPARED_LIGHT_CDF, GDPT_PREPARED_LIGHT_TRI_CDF, GDPT_PREPARED_LIGHT_TRI_POS,
       GDPT_PREPARED_LIGHT_TRI_NRM, GDPT_PREPARED_ENV_CDF_ROWS, GDPT_PREPARED_ENV_PDF_ROWS, GDPT_PREPARED_ENV_CDF_MARGINALS,
       GDPT_PREPARED_ENV_PDF_MARGINALS, GDPT_PREPARED_TABLES };
typedef struct GdptPreparedInfo {
    int64_t count[GDPT_PREPARED_TABLES];     /* elements of each table (records, or doubles for the fp64 pools) */
    uint64_t digest[GDPT_PREPARED_TABLES];
    double isect_eps;
    float bounds[6];                         /* fp32 scene bounds: min xyz, max xyz */
    int32_t bvh_depth, leaf_hist[4], wide_stack_need, wide8_stack_need;
    int32_t one_sided, lambert_only, has_rough, plan_take_pct;
    uint32_t material_mask;
    int32_t has_envmap, env_w, env_h, all_textures_constant;
} GdptPreparedInfo;
struct GdptSceneDesc;
int gdpt_debug_prepare_scene(const struct GdptSceneDesc *desc, GdptPreparedInfo *info, double *light_pmf, double *light_cdf, int capacity);
/* ---- The per-vertex device functions on arrays of cases (csrc/hip/debug_kat.hip) ------------------------------------------------
 * What the render kernels call at a vertex (the BSDF trio of device_bsdf.h and its fused eval_pdf, the inline Lambertian of
 * render_device.h, texture lookups, the pixel filter and the camera, the shading info of a hit, emitter sampling) is otherwise
 * observable only summed into an image. Each family below is one kernel that calls the product's functions as they are, one thread
 * per case (256-thread blocks, no LDS scene, no traversal), and one entry point
 *     gdpt_debug_kat_<family>(scene, variant, n, in, out)
 * with host arrays of n queries and n results. The entry runs on the scene's first render stream and has waited for it when it
 * returns. Before the launch the host checks `variant` against the family's table and every index a query carries against the table
 * sizes of the uploaded scene; a bad argument is refused (non-zero, message in gdpt_last_error) and never reaches the kernel.
 *
 * gdpt_debug_kat_variants(family, out, capacity): the family's table of variants, one row each, in the order `variant` indexes; returns
 * their number (out == NULL: the number alone), -1 for an unknown family or a capacity too small. Families: "bsdf", "texture",
 * "filter", "primary", "shading", "light", "envmap", "trace" (its rows carry the name alone: gdpt_debug_kat_trace_variants). The bsdf rows:
 *   - one per <ROUGH, TWOSIDED, MASK> triple of bsdf_sample / bsdf_eval / bsdf_pdf / bsdf_eval_pdf that a product kernel instantiates,
 *     the triple taken from the product's own constants (kAllMaterials, kSetGlass, the sets of render_phases_general_sets.h); `mask` bit
 *     t = material type t is in the kernel's set, `rough` / `twosided` = the RoughPlastic / RoughDielectric and the DisneyGlass /
 *     DisneyBSDF arms are compiled in;
 *   - two with inline_lambert = 1: mat_sample / mat_eval_pdf / mat_pdf with LAMBERT = true (Lambertian materials only), plain = the
 *     PLAIN flag of mat_eval_pdf (0, or kPlainConstTex = 2: constant reflectances only). That path has no separate eval: f[] is NaN.
 * "primary": variant 0 takes s = the screen position in [0, 1)^2, variant 1 the pixel-space numbers (x + u, y + v) (PIXEL_SPACE).
 * The other families have one variant.
 *
 * bsdf results: [0] = at the direction bsdf_sample returned (zeros when sample_valid == 0), [1] = at dir_out2; f/pdf from the
 * separate bsdf_eval and bsdf_pdf, fused_f/fused_pdf from bsdf_eval_pdf. texture: tex3 / tex1 of texture `slot` of a material.
 * shading: shading_info_tri of global triangle `index` (need_uv as given) or shading_info_sphere of sphere `index`. light:
 * sample_point_on_light and pdf_point_on_light of that point, for area emitter `light_id` (the environment map's placeholder is refused).
 * envmap: the environment-map code of render_path.h on the scene's own map, per case a pair of random numbers and a world direction
 * `dir` towards the light. sample_uv = table2d_sample(rnd); sample_dir = envmap_sample_dir(rnd); sample_pdf = envmap_pdf(-sample_dir) and
 * sample_emission = envmap_emission(-sample_dir), as next-event estimation forms them; dir_uv = envmap_uv of the local direction of `dir`;
 * dir_pdf = envmap_pdf(-dir) and dir_emission = envmap_emission(-dir), as the miss branches call them. Refused on the host, before any
 * launch: a scene without an environment map; a number that is not finite; a random number outside [0, 1]; a zero `dir`; n above 2^20. */
typedef struct GdptKatVariant { const char *name; uint32_t mask; int32_t rough, twosided, inline_lambert, plain; } GdptKatVariant;
typedef struct GdptKatVertex { double gn[3], fx[3], fy[3], fn[3], uv[2], uv_screen_size; } GdptKatVertex;   /* what the lobes read of gd::Vertex */
typedef struct GdptKatBsdfQuery { int32_t material_id, pad; GdptKatVertex vertex; double dir_in[3], dir_out2[3], ruv[2], rw; } GdptKatBsdfQuery;
typedef struct GdptKatBsdfResult {
    int32_t sample_valid, pad;
    double s_dir[3], s_eta, s_rough;
    double f[2][3], pdf[2];
    double fused_f[2][3], fused_pdf[2];
} GdptKatBsdfResult;
typedef struct GdptKatTextureQuery { int32_t material_id, slot; double uv[2], uv_screen_size; } GdptKatTextureQuery;
typedef struct GdptKatTextureResult { double tex3[3], tex1; } GdptKatTextureResult;
typedef struct GdptKatFilterQuery { int32_t type, pad; double param, u[2]; } GdptKatFilterQuery;
typedef struct GdptKatFilterResult { double out[2]; } GdptKatFilterResult;
typedef struct GdptKatPrimaryQuery { double s[2]; } GdptKatPrimaryQuery;
typedef struct GdptKatPrimaryResult { double org[3], dir[3]; } GdptKatPrimaryResult;
typedef struct GdptKatShadingQuery { int32_t is_sphere, index, need_uv, pad; double st[2], gn[3]; } GdptKatShadingQuery;
typedef struct GdptKatShadingResult { double uv[2], fx[3], fy[3], fn[3], inv_uv_size; } GdptKatShadingResult;
typedef struct GdptKatLightQuery { int32_t light_id, pad; double ref[3], uv[2], w; } GdptKatLightQuery;
typedef struct GdptKatLightResult { double position[3], normal[3], pdf; } GdptKatLightResult;
typedef struct GdptKatEnvmapQuery { double rnd[2], dir[3]; } GdptKatEnvmapQuery;
typedef struct GdptKatEnvmapResult {
    double sample_uv[2], sample_dir[3], sample_pdf, sample_emission[3];
    double dir_uv[2], dir_pdf, dir_emission[3];
} GdptKatEnvmapResult;
int gdpt_debug_kat_variants(const char *family, GdptKatVariant *out, int capacity);
int gdpt_debug_kat_bsdf(const struct GdptScene *scene, int variant, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out);
int gdpt_debug_kat_texture(const struct GdptScene *scene, int variant, int n, const GdptKatTextureQuery *in, GdptKatTextureResult *out);
int gdpt_debug_kat_filter(const struct GdptScene *scene, int variant, int n, const GdptKatFilterQuery *in, GdptKatFilterResult *out);
int gdpt_debug_kat_primary(const struct GdptScene *scene, int variant, int n, const GdptKatPrimaryQuery *in, GdptKatPrimaryResult *out);
int gdpt_debug_kat_shading(const struct GdptScene *scene, int variant, int n, const GdptKatShadingQuery *in, GdptKatShadingResult *out);
int gdpt_debug_kat_light(const struct GdptScene *scene, int variant, int n, const GdptKatLightQuery *in, GdptKatLightResult *out);
int gdpt_debug_kat_envmap(const struct GdptScene *scene, int variant, int n, const GdptKatEnvmapQuery *in, GdptKatEnvmapResult *out);
/* ---- The BVH walks on arrays of rays (csrc/hip/debug_kat_trace.hip) -----------------------------------------------------------------
 * Family "trace": closest hit (device_trace.h: smallest fp32 t in [tnear, tfar), lowest primitive id on ties) or, with any_hit, whether
 * any primitive accepts the ray, by one of the walks the render kernels make. One thread per ray in 256-thread blocks, the lanes past n
 * finished from the start. The kernels call setup_trace, trav_init and trav_run as the product does, re-entering the walk as
 * trace_pending does (stop_below = pending * keep_frac >> 8; knobs keep_frac and search_frac, the product's defaults when unset).
 * gdpt_debug_kat_trace_variants: the table, one row per distinct (TraceCfg, residency) that a product kernel instantiates, then two
 * rows that run the wavefront pipeline's own trace kernel (launch_wf_trace) on a ray queue written as its step kernel writes it.
 * ww / wide / flat / spheres / spec / leaf_k: the TraceCfg (render_device.h); lds_scene: the walk reads the block's LDS copy of the scene;
 * lds_stack_levels: stack slots per lane in LDS, 0 = the tree's own bound (dynamic LDS; scenes walked from HBM), the wavefront rows
 * keep deeper levels in HBM. gdpt_debug_kat_variants("trace") gives the same rows by name alone.
 * Result: gid = -1 for a miss (t, u, v are then without meaning); ng is set for a sphere hit only. With any_hit only gid >= 0 counts.
 * Refused on the host, before any launch: an unknown variant; an lds_scene row for a scene that does not fit the LDS copy of that form;
 * a spheres = 0 row on a scene with spheres; a wavefront row with a finite tfar or any_hit; a number that is not finite (tfar may be
 * +infinity) or does not stay finite in fp32; a direction that is zero in fp32; tnear < 0; tfar < tnear; n above 2^20. */
typedef struct GdptKatTraceVariant { const char *name; int32_t ww, wide, flat, spheres, spec, leaf_k, lds_scene, wavefront, lds_stack_levels; } GdptKatTraceVariant;
typedef struct GdptKatTraceQuery { double org[3], dir[3], tnear, tfar; int32_t any_hit, pad; } GdptKatTraceQuery;
typedef struct GdptKatTraceResult { int32_t gid; float t, u, v, ng[3]; } GdptKatTraceResult;
int gdpt_debug_kat_trace_variants(GdptKatTraceVariant *out, int capacity);
int gdpt_debug_kat_trace(const struct GdptScene *scene, int variant, int n, const GdptKatTraceQuery *in, GdptKatTraceResult *out);
/* Removes every override: the library is back on its product path. */
void gdpt_debug_knobs_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GDPT_DEBUG_H */
