/* gdpt.h — C ABI of the MI355X-native gradient-domain path tracing hot path.
 *
 * This is the drop-in boundary for LaJolla's `Integrator::GradPath` path
 * (reference: vedrocks15/Gradient-Based-Path-Tracing). The reference has no FFI
 * layer; its seams are C++ functions linked statically. Each entry point below
 * names the reference interface it replaces (file:line under /root/reference).
 *
 *   gdpt_parse_scene        <- parse_scene()            src/parsers/parse_scene.h:9, parse_scene.cpp:1615-1630
 *   gdpt_scene_upload       <- Scene::Scene()           src/scene.cpp:4-53   (Embree BVH build -> own BVH2 + HBM upload)
 *   gdpt_render             <- gradient_path_render()   src/render.cpp:257-333 (tile loop + grad_path_tracing, src/path_tracing.h:354-1050)
 *   gdpt_assemble           <- gradient assembly        src/render.cpp:336-350
 *   gdpt_poisson_solve      <- fourierSolve()           src/render.cpp:172-254 (argument-for-argument)
 *   gdpt_gradient_path_render <- gradient_path_render() src/render.cpp:257-370 (whole: render + assemble + solve)
 *   gdpt_imwrite            <- imwrite()                src/image.cpp:135-173
 *   gdpt_multi_*            <- parallel_for tile pool   src/parallel.cpp:183-256, src/render.cpp:271-277 (bands over several GPUs)
 *
 * Plain pointers and sizes only; no C++/torch types. All images are row-major
 * `data[(y*W+x)*3+c]` fp64, exactly `Image3::data` (src/image.h:13-39).
 * Every function returns 0 on success, non-zero on failure; the message is
 * available from gdpt_last_error() (thread-local).
 */
#ifndef GDPT_H
#define GDPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scene description (host memory, flattened `Scene`, src/scene.h:40-80) ---- */

enum { GDPT_TEX_CONSTANT = 0, GDPT_TEX_IMAGE = 1, GDPT_TEX_CHECKERBOARD = 2 }; /* src/texture.h:83-102 */

/* Texture<Real> uses v0[0]/v1[0]; Texture<Spectrum> uses all three channels. */
typedef struct GdptTexture {
    int32_t type;
    int32_t image_id;         /* IMAGE: index into GdptSceneDesc::images (1- or 3-channel) */
    double v0[3];             /* CONSTANT: value; CHECKERBOARD: color0 */
    double v1[3];             /* CHECKERBOARD: color1 */
    double uscale, vscale, uoffset, voffset;
} GdptTexture;

/* Order follows the std::variant in src/material.h:82-90. */
enum {
    GDPT_MAT_LAMBERTIAN = 0, GDPT_MAT_ROUGHPLASTIC = 1, GDPT_MAT_ROUGHDIELECTRIC = 2,
    GDPT_MAT_DISNEY_DIFFUSE = 3, GDPT_MAT_DISNEY_METAL = 4, GDPT_MAT_DISNEY_GLASS = 5,
    GDPT_MAT_DISNEY_CLEARCOAT = 6, GDPT_MAT_DISNEY_SHEEN = 7, GDPT_MAT_DISNEY_BSDF = 8
};

/* Texture slots per material type (member order of the structs in src/material.h:12-80):
 *   LAMBERTIAN       0 reflectance
 *   DISNEY_DIFFUSE   0 base_color 1 roughness 2 subsurface
 *   DISNEY_METAL     0 base_color 1 roughness 2 anisotropic
 *   DISNEY_GLASS     0 base_color 1 roughness 2 anisotropic            (+eta)
 *   DISNEY_CLEARCOAT 0 clearcoat_gloss
 *   DISNEY_SHEEN     0 base_color 1 sheen_tint
 *   DISNEY_BSDF      0 base_color 1 specular_transmission 2 metallic 3 subsurface 4 specular
 *                    5 roughness 6 specular_tint 7 anisotropic 8 sheen 9 sheen_tint
 *                    10 clearcoat 11 clearcoat_gloss                    (+eta)
 */
#define GDPT_MAT_MAX_TEX 12
typedef struct GdptMaterial {
    int32_t type;
    int32_t _pad;
    double eta;
    GdptTexture tex[GDPT_MAT_MAX_TEX];
} GdptMaterial;

typedef struct GdptImage {     /* level 0 of a Mipmap1/Mipmap3 (src/mipmap.h:9-12); mips are built by the library */
    int32_t width, height, channels; /* channels 1 or 3 */
    int32_t _pad;
    const double *texels;      /* width*height*channels, row-major */
} GdptImage;

enum { GDPT_SHAPE_SPHERE = 0, GDPT_SHAPE_TRIMESH = 1 }; /* src/shape.h:44 */

typedef struct GdptShape {
    int32_t type;
    int32_t material_id;
    int32_t area_light_id;     /* -1 if not an emitter */
    int32_t num_vertices, num_triangles;
    int32_t _pad;
    double center[3];          /* sphere */
    double radius;             /* sphere */
    const double *positions;   /* 3*num_vertices (world space) */
    const int32_t *indices;    /* 3*num_triangles */
    const double *normals;     /* 3*num_vertices or NULL */
    const double *uvs;         /* 2*num_vertices or NULL */
} GdptShape;

typedef struct GdptLight {     /* DiffuseAreaLight (src/light.h), or the placeholder of the environment map (shape_id = -1,
                                  its data is GdptSceneDesc::envmap) so that light ids keep the reference's parse order */
    int32_t shape_id;
    int32_t _pad;
    double intensity[3];
} GdptLight;

enum { GDPT_FILTER_BOX = 0, GDPT_FILTER_TENT = 1, GDPT_FILTER_GAUSSIAN = 2 }; /* src/filter.h:31-46 */

typedef struct GdptCamera {    /* src/camera.h:10-26 */
    double sample_to_cam[16];  /* row-major 4x4 */
    double cam_to_world[16];
    int32_t width, height;
    int32_t filter_type;
    int32_t _pad;
    double filter_param;       /* Box/Tent: width; Gaussian: stddev */
} GdptCamera;

enum { GDPT_INTEGRATOR_PATH = 5, GDPT_INTEGRATOR_GRADPATH = 7, GDPT_INTEGRATOR_OTHER = -1 }; /* src/scene.h:14-23 */

typedef struct GdptEnvmap {    /* Envmap, src/light.h + src/lights/envmap.inl: lat-long image, uv = (azimuth/2pi, elevation/pi) */
    int32_t light_id;          /* index into lights[] */
    int32_t image_id;          /* 3-channel image */
    double scale;
    double to_world[16], to_local[16];   /* row-major; to_local = inverse(to_world) */
} GdptEnvmap;

typedef struct GdptSceneDesc {
    GdptCamera camera;
    int32_t integrator;
    int32_t samples_per_pixel; /* <sampler sampleCount>; the reference ignores it (src/render.cpp:293) */
    int32_t max_depth;         /* -1 = unbounded (RR only) */
    int32_t rr_depth;
    int32_t num_materials, num_shapes, num_lights, num_images;
    const GdptMaterial *materials;
    const GdptShape *shapes;
    const GdptLight *lights;
    const GdptImage *images;
    char output_filename[256]; /* film `filename`, default "image.exr" (src/parsers/parse_scene.cpp:15) */
    int32_t has_envmap;        /* the XML holds an <emitter type="envmap">: ignored by GradPath (src/path_tracing.h:982-985),
                                  sampled and looked up by the Path entry points */
    int32_t _pad;
    GdptEnvmap envmap;         /* valid when has_envmap */
} GdptSceneDesc;

/* ---- render parameters ---- */

/* How PCG32 streams (src/pcg.h:33-41) are assigned.
 *   TILE   : init_pcg32(tile_y*ntx+tile_x), pixels y-outer/x-inner, samples innermost — bit-for-bit the
 *            reference order (src/render.cpp:281-309). Serial per tile: one GPU lane per tile (slow; for checks).
 *   SAMPLE : init_pcg32((y*W+x)*spp + s) per sample — every sample independent (the throughput mode). */
enum { GDPT_RNG_TILE = 0, GDPT_RNG_SAMPLE = 2 };
/* How the four offset paths follow the base path.
 * GDPT_SHIFT_REFERENCE: what grad_path_tracing does (src/path_tracing.h:351-560): offsets replay the base path's random
 *   numbers and never rejoin it. The drop-in, parity-tested behaviour.
 * GDPT_SHIFT_RECONNECT: the offset path's first vertex is reconnected to the base path's second vertex, with the
 *   Jacobian and the balance-heuristic weights of the reference's own sketch (small_gdpt.py:163-219, :380-420); the
 *   gradient buffers then are unbiased estimates of I(x)-I(x-1), I(y)-I(y-1) and the Poisson solve denoises. Same
 *   base path (and primal image) as the reference mode. GDPT_RNG_SAMPLE only. Not part of the reference's output. */
enum { GDPT_SHIFT_REFERENCE = 0, GDPT_SHIFT_RECONNECT = 1 };

typedef struct GdptRenderParams {
    int32_t spp;               /* <=0: use scene samples_per_pixel; the reference hard-codes 1000 (src/render.cpp:293) */
    int32_t rng_scheme;        /* GDPT_RNG_* */
    int32_t row_begin, row_end;/* render rows [row_begin,row_end) only (multi-GPU bands); 0,0 = whole image.
                                  Rows outside the band are left untouched in the output buffers. */
    int32_t max_depth_override;/* 0 = use scene; else value */
    int32_t shift_mode;        /* GDPT_SHIFT_* (gdpt_render* only; 0 = the reference's behaviour) */
    int32_t plan_rows;         /* 0 = film height. A pixel's samples are cut into work items ("chunks") whose partial sums are
                                  merged in chunk order; the cut is made for a band of this many rows, so that a small band
                                  rendered alone (one device of N) still consists of many short items instead of a few long
                                  ones. Renders of the same pixel with the same plan_rows are bit-identical whatever band
                                  they are part of: the multi-device hosts pass the rows of their largest band, and a
                                  single-device render given the same value reproduces their images bit for bit. */
    int32_t reserved;          /* 0 */
} GdptRenderParams;

/* A render's spp samples as a window of a larger block of PCG streams (GDPT_RNG_SAMPLE only): sample s of pixel (x,y) draws from
 * stream (y*W + x)*stream_spp + first_sample + s, and first_sample + spp <= stream_spp. The buffers stay means over the window's spp
 * samples. Windows that tile [0, stream_spp) hold, together, exactly the samples of the one-shot render at spp = stream_spp;
 * stream_spp = spp, first_sample = 0 IS that render. W*H*stream_spp must fit 63 bits. */
typedef struct GdptSampleWindow { int32_t stream_spp, first_sample; } GdptSampleWindow;

typedef struct GdptRenderStats {
    uint64_t samples;          /* grad_path_tracing calls */
    uint64_t rays;             /* closest-hit queries (5 primaries + 1 per bounce; the reference's 4 tfar=0 rays are omitted) */
    uint64_t bounces;          /* bounce-loop iterations */
    uint64_t nodes_visited;    /* BVH nodes fetched (counting builds only, else 0) */
    uint64_t tris_tested;      /* triangles tested (counting builds only, else 0) */
    uint64_t nonfinite_samples;/* samples whose record held a NaN/Inf (propagated, as the reference does) */
    double render_ms;          /* device time of the render kernel(s), HIP events */
    uint64_t node_bytes;       /* size of one fetched BVH node in the form this render walked (64: BVH2, 128: BVH4) */
    /* SIMT utilisation of the persistent kernel (counting builds only, else 0): loop trips counted once per wave */
    uint64_t wave_node_trips;  /* node-visit trips;  nodes_visited / (64 * this) = lane utilisation of the box tests */
    uint64_t wave_leaf_trips;  /* leaf-test trips */
    uint64_t wave_steps;       /* lane-machine steps (one pending ray per live lane each) */
    uint64_t lane_steps;       /* live lanes summed over those steps */
} GdptRenderStats;

typedef struct GdptPoissonStats {
    int32_t iterations;        /* CG iterations (0 for the direct DCT solver) */
    int32_t solver;            /* GDPT_SOLVER_* actually used */
    double rel_residual;       /* ||W(h - A f)|| / ||W h|| at exit (CG) */
    double solve_ms;           /* device time, HIP events */
} GdptPoissonStats;

/* CG: conjugate gradients on W(alpha I - L) f = W h + DC shift (matches the DCT solve to the CG tolerance; differs
 *     from the reference by its fp32-lambda quirk, ~3e-9).
 * DCT_MFMA (the default): direct solve, exact reference operator. The two 1-D DCT-I passes are fp64 GEMMs against fixed
 *     cosine matrices, run by hand-written fp64 MFMA kernels on HALF the flops (even / odd fold of the DCT-I matrix); their
 *     epilogues carry the spectral division, the DC override and the final scaling (5 launches).
 * DCT: the same solve with the passes as rocBLAS dgemm_strided_batched on the unfolded matrices (8 launches): kept as the
 *     measured alternative (tests/time_poisson.py). */
enum { GDPT_SOLVER_CG = 0, GDPT_SOLVER_DCT = 1, GDPT_SOLVER_DCT_MFMA = 2 };
#define GDPT_SOLVER_DEFAULT GDPT_SOLVER_DCT_MFMA   /* what gdpt_poisson_solve, gdpt_gradient_path_render and gdpt_multi_* use */

typedef struct GdptScene GdptScene;   /* opaque: device-resident scene (BVH2 + BVH4, triangles, materials, textures) */

/* ---- host-side scene ingest (Mitsuba-0.x XML subset) ---- */
int gdpt_parse_scene(const char *xml_path, GdptSceneDesc **out_desc);
/* Same with the <film> extent replaced (0 = keep the scene's): the benchmark configurations quote their own film
 * sizes (sponza at 1280x720, cbox at 1024x1024); the camera is built for the new aspect ratio, as if the XML said so. */
int gdpt_parse_scene_film(const char *xml_path, int film_width, int film_height, GdptSceneDesc **out_desc);
void gdpt_free_scene_desc(GdptSceneDesc *desc);

/* ---- device scene ---- */
int gdpt_scene_upload(const GdptSceneDesc *desc, int device, GdptScene **out_scene);
void gdpt_scene_free(GdptScene *scene);
/* Copies the BVH the library built (for inspection/tests): node count, triangle count, depth. */
int gdpt_scene_info(const GdptScene *scene, int32_t *num_nodes, int32_t *num_tris, int32_t *num_spheres, int32_t *bvh_depth);

/* ---- hot path, host buffers (caller-owned W*H*3 doubles each, as Image3::data) ---- */
int gdpt_render(GdptScene *scene, const GdptRenderParams *params,
                double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                GdptRenderStats *stats /* nullable */);

/* ---- hot path, device buffers (hipMalloc'd / torch CUDA tensors; data stays in HBM) ----
 * `stream` is a hipStream_t passed as void* (NULL = default stream). Asynchronous w.r.t. the host
 * unless `stats` is non-NULL (then it synchronises to read the counters).
 * Calls on one scene handle come from one host thread at a time. The output buffers are written only by work on `stream`,
 * in call order, so consecutive renders on one stream behave as ordered by it. Internally an enqueue-only render
 * (stats == NULL) of a scene with one-sided lobes runs its render kernel on one of two streams the handle owns, with one
 * of two sets of launch scratch (work queue, per-item partial sums, counters; the second set, the size of the first, is
 * allocated by the second such call): the previous frame's reduction and whatever the caller enqueued behind it (its solve)
 * then run while this frame's kernel drains, where most of the chip would idle. The kernel reads only the scene, so it does
 * not wait for the caller's stream as it is at this call, only as it was at the previous one; what it needs beyond that
 * (scratch reuse two frames apart, another caller stream, growth) is ordered by events. Every other render (stats requested, two-sided or rough lobes, GDPT_RNG_TILE, GDPT_SHIFT_RECONNECT,
 * Integrator::Path, a stream that is being captured into a graph) runs wholly on `stream` after waiting for the handle's
 * own streams. A captured launch uses the first scratch set and leaves no event of the handle's in the graph: replays of such a
 * graph must not be mixed with direct enqueue-only renders of the same handle unless the caller orders them (a device or stream
 * synchronise between the two kinds). gdpt_scene_free waits for what the handle has in flight. To render on several devices upload one scene
 * handle per device. The reference's render() is called once, synchronously (src/main.cpp:40). */
int gdpt_render_device(GdptScene *scene, const GdptRenderParams *params,
                       double *d_img, double *d_cx0, double *d_cy0, double *d_cx1, double *d_cy1,
                       void *stream, GdptRenderStats *stats /* nullable */);

/* ---- Integrator::Path (path_render, src/render.cpp:74-117 over path_tracing, src/path_tracing.h:13-348) ----
 * Unidirectional path tracing with next-event estimation + MIS for scenes lit by area emitters (meshes, spheres)
 * and / or an environment map (src/lights/envmap.inl): img = mean over spp of path_tracing(x, y). Same parameters,
 * RNG schemes and stats as gdpt_render; scenes without any emitter are refused (error status). */
int gdpt_path_render(GdptScene *scene, const GdptRenderParams *params, double *img, GdptRenderStats *stats /* nullable */);
int gdpt_path_render_device(GdptScene *scene, const GdptRenderParams *params, double *d_img,
                            void *stream, GdptRenderStats *stats /* nullable */);

/* gdpt_render_device / gdpt_path_render_device on a sample window. window == NULL forwards to the plain call. Refused with an error:
 * GDPT_RNG_TILE (one stream per tile, no window), a window that leaves [0, stream_spp), a stream_spp too large for the film. */
int gdpt_render_window_device(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window /* nullable */,
                              double *d_img, double *d_cx0, double *d_cy0, double *d_cx1, double *d_cy1,
                              void *stream, GdptRenderStats *stats /* nullable */);
int gdpt_path_render_window_device(GdptScene *scene, const GdptRenderParams *params, const GdptSampleWindow *window /* nullable */,
                                   double *d_img, void *stream, GdptRenderStats *stats /* nullable */);

/* c=img; cx=cx0(x,y)+cx1(x-1,y); cy=cy0(x,y)+cy1(x,y-1)  (src/render.cpp:340-350). Device pointers. */
int gdpt_assemble_device(int width, int height,
                         const double *d_img, const double *d_cx0, const double *d_cy0,
                         const double *d_cx1, const double *d_cy1,
                         double *d_c, double *d_cx, double *d_cy, void *stream);

/* Screened Poisson reconstruction; same arguments as fourierSolve (src/render.cpp:172-175). Host pointers.
 * Uses GDPT_SOLVER_DEFAULT: the reference's algorithm itself (DCT-I, fp32-rounded eigenvalue, DC override), the
 * transform evaluated as fp64 MFMA GEMMs on the GPU. */
int gdpt_poisson_solve(int width, int height,
                       const double *imgData, const double *imgGradX, const double *imgGradY,
                       double dataCost, double *imgOut);
/* Same with solver choice, tolerance and stats. solver: GDPT_SOLVER_*. tol<=0 selects the default 1e-10. */
int gdpt_poisson_solve_ex(int width, int height,
                          const double *imgData, const double *imgGradX, const double *imgGradY,
                          double dataCost, double *imgOut,
                          int solver, double tol, int max_iters, GdptPoissonStats *stats /* nullable */);
/* Device-pointer variant (inputs/outputs in HBM). The library keeps its scratch per (device, stream). With
 * GDPT_SOLVER_DCT_MFMA / GDPT_SOLVER_DCT and stats == NULL the call only enqueues work on `stream` (no event, no host wait); with stats it
 * brackets the solve with HIP events and waits for it. GDPT_SOLVER_CG always waits (host-side convergence check). */
int gdpt_poisson_solve_device(int width, int height,
                              const double *d_c, const double *d_gx, const double *d_gy,
                              double dataCost, double *d_out,
                              int solver, double tol, int max_iters,
                              void *stream, GdptPoissonStats *stats /* nullable */);

/* gdpt_assemble_device followed by gdpt_poisson_solve_device on its outputs — what gradient_path_render does after the tile loop
 * (src/render.cpp:340-353) — as one call for a film that sits whole on one device: with the DCT solvers the assembly and the
 * right-hand side of the solve are one pass over the film. d_c / d_cx / d_cy are written as gdpt_assemble_device writes them; every
 * result has the bits of the two separate calls. Enqueue-only unless `stats` (as gdpt_poisson_solve_device). */
int gdpt_assemble_solve_device(int width, int height,
                               const double *d_img, const double *d_cx0, const double *d_cy0,
                               const double *d_cx1, const double *d_cy1,
                               double *d_c, double *d_cx, double *d_cy,
                               double dataCost, double *d_out,
                               int solver, double tol, int max_iters,
                               void *stream, GdptPoissonStats *stats /* nullable */);

/* Drops the solver scratch the library keeps for `stream` on the current device (buffers, handles, events). Owners of a
 * stream call it before destroying the stream, with no solve in flight on it; a stream the library never saw is fine. */
int gdpt_poisson_forget_stream(void *stream);

/* Whole Integrator::GradPath: render -> assemble -> solve -> final image (host, W*H*3 doubles).
 * Optionally returns the five raw buffers too (any of them may be NULL). */
int gdpt_gradient_path_render(GdptScene *scene, const GdptRenderParams *params, double dataCost,
                              double *out_image,
                              double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                              GdptRenderStats *rstats, GdptPoissonStats *pstats);

/* ---- robust (L1) reconstruction: IRLS over a weighted screened-Poisson solve (not part of the reference) ----
 * fourierSolve is a least-squares solve: one firefly in a gradient buffer is spread over the image as a dipole. The L1
 * reconstruction minimises  E(f) = sum over rows of |r|_2  instead, rows of three channels each:
 *     data row of pixel (x,y):  r_d = sqrt(dataCost) (f - c)
 *     x-edge row, x >= 1:       r_x = f(x,y) - f(x-1,y) - gx(x,y)
 *     y-edge row, y >= 1:       r_y = f(x,y) - f(x,y-1) - gy(x,y)
 * Edges exist inside the film only (natural boundary: gx(0,.) and gy(.,0) are not read; NOT fourierSolve's mirror operator).
 * Round 0 solves the unweighted system from f = c; round k = 1..irls_iters gives every row the weight
 * w = 1 / (eps_k + |r|_2) of the previous image (one weight for its three channels: no colour shift),
 * eps_k = max(eps_init eps_decay^(k-1), eps_floor), and solves, per channel,
 *     (a diag(w_d) + Dx^T diag(w_x) Dx + Dy^T diag(w_y) Dy) f = a w_d c + Dx^T (w_x gx) + Dy^T (w_y gy),   a = dataCost,
 * by Jacobi-preconditioned conjugate gradients warm-started from the previous image, until |residual| <= cg_tol |rhs| or
 * cg_max_iters. Deterministic: the same inputs give the same bits. */
enum { GDPT_RECON_L2 = 0, GDPT_RECON_L1 = 1 };
typedef struct GdptReconParams {
    int32_t norm;              /* GDPT_RECON_*; GDPT_RECON_L2 = the default fourierSolve path, every other field ignored */
    int32_t irls_iters;        /* reweighted rounds K after round 0. 0: default 20; < 0: none (round 0 alone) */
    int32_t cg_max_iters;      /* per round. <= 0: default 1000 */
    int32_t reserved;          /* 0 */
    double eps_init;           /* 0: default 0.05 */
    double eps_decay;          /* in (0, 1]. 0: default 0.5 */
    double eps_floor;          /* 0: default 1e-3 (without a floor the systems become too ill-conditioned for the CG) */
    double cg_tol;             /* 0: default 1e-6 */
} GdptReconParams;             /* negative or non-finite eps_* / cg_tol and eps_decay > 1 are refused */
typedef struct GdptReconStats {
    int32_t norm;              /* GDPT_RECON_* actually used */
    int32_t irls_rounds;       /* systems solved: K + 1 (L2: 0) */
    int32_t cg_iters_total;    /* CG iterations over all rounds */
    int32_t cg_iters_last;     /* ... of the last round */
    double energy_first;       /* E(f_0): after the unweighted round */
    double energy_last;        /* E(f_K): of the image returned */
    double rel_residual_last;  /* |b - A f| / |b| at the exit of the last round */
    double solve_ms;           /* device time, HIP events */
} GdptReconStats;
/* Host pointers (W*H*3 doubles each, as gdpt_poisson_solve). params == NULL or norm == GDPT_RECON_L2: gdpt_poisson_solve's result,
 * bit for bit. No CPU fallback. */
int gdpt_reconstruct(int width, int height, const double *c, const double *gx, const double *gy, double dataCost,
                     const GdptReconParams *params /* nullable */, double *out, GdptReconStats *stats /* nullable */);
/* Device pointers; `out` must not alias an input. The L1 path waits for `stream` (host-side convergence checks) and keeps its
 * scratch per (device, stream): gdpt_poisson_forget_stream drops it with the solver's. */
int gdpt_reconstruct_device(int width, int height, const double *d_c, const double *d_gx, const double *d_gy, double dataCost,
                            const GdptReconParams *params /* nullable */, double *d_out, void *stream,
                            GdptReconStats *stats /* nullable */);
/* gdpt_gradient_path_render with the final solve replaced by gdpt_reconstruct on the assembled c, cx, cy; the five raw buffers
 * are those of gdpt_gradient_path_render. */
int gdpt_gradient_path_render_recon(GdptScene *scene, const GdptRenderParams *params, double dataCost,
                                    const GdptReconParams *recon /* nullable */, double *out_image,
                                    double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                                    GdptRenderStats *rstats /* nullable */, GdptReconStats *cstats /* nullable */);

/* ---- progressive rendering: accumulated passes with per-pixel variance (not part of the reference) ----
 * A session renders a scene in passes. Pass k draws the window [done, done + n_k) of every pixel's block of budget_spp streams, so
 * a session that spends its budget has drawn exactly the samples of the one-shot render at spp = budget_spp. Each pass (a mean
 * m over its n samples, per buffer component) is folded into a running mean and a sum of weighted squared deviations
 * (West 1979):   W += n;  d = m - mean;  mean += (n/W) d;  M2 += n d (m - mean_new).
 * After K passes, E[M2] = (K-1) sigma^2 for per-sample variance sigma^2, so the variance of the running mean is estimated by
 *     var_mean = M2 / ((K-1) done)                                                          (defined from K >= 2)
 * and the session's error estimate is the estimated relative RMSE of the primal mean,
 *     sqrt( sum var_mean(img) / sum mean(img)^2 )   over pixels and channels.
 * A non-finite pass value propagates into the mean, as everywhere in this library; pixels whose img mean or M2 is not finite are
 * left out of both sums and counted. The sums are reduced in a fixed order: the same session gives the same bits.
 * The session holds all its planes in HBM and uses the scene handle's launch scratch: one render per scene handle at a time. */
enum { GDPT_PROGRESSIVE_GRADPATH = 0, GDPT_PROGRESSIVE_PATH = 1 };
enum { GDPT_STOP_NONE = 0, GDPT_STOP_TARGET = 1, GDPT_STOP_BUDGET = 2, GDPT_STOP_MAX_PASSES = 3 };
typedef struct GdptProgressiveConfig {
    int32_t mode;              /* GDPT_PROGRESSIVE_*: GradPath (five buffers) or Integrator::Path (img alone) */
    int32_t shift_mode;        /* GDPT_SHIFT_* (GradPath) */
    int32_t budget_spp;        /* samples per pixel the session may draw: the stream_spp of every pass. <= 0: the scene's */
    int32_t max_depth_override;/* 0 = use scene */
} GdptProgressiveConfig;
typedef struct GdptProgressiveStatus {
    int32_t passes;            /* K */
    int32_t spp_done;          /* samples per pixel so far */
    int32_t budget_spp;
    int32_t stop_reason;       /* GDPT_STOP_* of the last gdpt_progressive_run (GDPT_STOP_NONE before one) */
    double error_estimate;     /* NaN while K < 2 */
    uint64_t pixels_left_out;  /* of the error estimate (non-finite) */
    double fold_ms;            /* device time of the last pass's fold launches, HIP events */
    GdptRenderStats totals;    /* counters and render_ms summed over the passes; node_bytes of the last pass */
} GdptProgressiveStatus;
typedef struct GdptProgressive GdptProgressive;   /* opaque */

/* `stream` (hipStream_t as void*, NULL = default) carries all of the session's work. The scene must outlive the session. */
int gdpt_progressive_create(GdptScene *scene, const GdptProgressiveConfig *config, void *stream, GdptProgressive **out);
void gdpt_progressive_free(GdptProgressive *session);
/* Renders the window [done, done + spp) into the pass buffers, folds it in (one launch over the film), advances done. Blocking.
 * A pass beyond the budget, or spp <= 0, is refused. stats (nullable): this pass's. */
int gdpt_progressive_add_pass(GdptProgressive *session, int spp, GdptRenderStats *stats);
int gdpt_progressive_status(const GdptProgressive *session, GdptProgressiveStatus *status);
/* Copies out W*H*3 doubles per plane; any pointer may be NULL; on_device != 0: the pointers are device memory. Blocking.
 *   means[k], vars[k]: running mean and variance of the mean of buffer k = img, cx0, cy0, cx1, cy1 (Path: k = 0 only, the
 *                      others must be NULL). Variances need K >= 2.
 *   assembled_vars[3]: variances of the assembled c, cx, cy. cx0(x,y) and cx1(x-1,y) come from different pixels' streams and are
 *                      independent: var(cx)(x,y) = var(cx0)(x,y) + var(cx1)(x-1,y), var(cy)(x,y) = var(cy0)(x,y) + var(cy1)(x,y-1)
 *                      (the second term absent at x = 0 / y = 0); var(c) = var(img). GradPath only. */
int gdpt_progressive_read(GdptProgressive *session, int on_device, double *const means[5], double *const vars[5],
                          double *const assembled_vars[3]);
/* gdpt_assemble_device on the running means, then gdpt_reconstruct_device (recon NULL: L2) into `out` (W*H*3 doubles, host, or
 * device with on_device != 0). May be called after any pass: a preview. GradPath only. Blocking. */
int gdpt_progressive_reconstruct(GdptProgressive *session, double dataCost, const GdptReconParams *recon /* nullable */,
                                 int on_device, double *out, GdptReconStats *stats /* nullable */);
/* Adds passes of pass_spp samples (the last one shortened to the budget) until the budget is spent (GDPT_STOP_BUDGET),
 * max_passes passes were added by this call (GDPT_STOP_MAX_PASSES; max_passes <= 0: no limit), or K >= 2 and the error estimate is
 * <= target_error (GDPT_STOP_TARGET; target_error <= 0: no target). Blocking; status (nullable) as gdpt_progressive_status. */
int gdpt_progressive_run(GdptProgressive *session, double target_error, int pass_spp, int max_passes, GdptProgressiveStatus *status);

/* ---- sessions over a slice of the stream block, and their merge: a session's samples split over sessions and devices ----
 * A pass is identified by its window of the block of budget_spp streams alone, so two sessions that own disjoint slices of one
 * block render disjoint samples of the whole film, each at the same cost per sample (no bands, no halo, no balancing). What they
 * hold combines exactly (Chan, Golub, LeVeque 1979), per buffer component:
 *     W = Wa + Wb;  d = mean_b - mean_a;  mean = mean_a + (Wb/W) d;  M2 = (M2a + M2b) + d d (Wa Wb / W);  K = Ka + Kb
 * which is the state of one session that folded all the passes of both: var_mean = M2 / ((K-1) W) and the error estimate keep
 * their meaning.
 * gdpt_progressive_create_slice: config->budget_spp stays the size of the block (the stream_spp of every pass); the session owns
 * [first_sample, first_sample + num_samples) of it and its passes draw the windows {budget_spp, first_sample + own samples done}.
 * first_sample < 0, num_samples < 0 and a slice that leaves [0, budget_spp) are refused; num_samples == 0 is an accumulator that only
 * receives merges. gdpt_progressive_create is the slice [0, budget_spp). For every session GdptProgressiveStatus reads:
 *     spp_done = W, all samples held, merged ones included;  passes = K;  totals include the totals of merged sessions;
 *     budget_spp = the slice size + the samples merged in ("budget spent" stays spp_done == budget_spp);
 * add_pass and run check the budget against the session's own slice. */
int gdpt_progressive_create_slice(GdptScene *scene, const GdptProgressiveConfig *config, int first_sample, int num_samples, void *stream,
                                  GdptProgressive **out);
/* dst takes in src's statistics by the update above (one launch over the film, on dst's stream); src is unchanged. Blocking. Merging
 * into a session that holds nothing copies src's planes, bit for bit. Afterwards error_estimate, pixels_left_out and fold_ms refer to
 * the merge launch as they would to a fold, and dst may go on adding passes of its own. A src without passes is a no-op.
 * Every session keeps the intervals of the block it holds (its own [first, first + own samples done) and the merged ones). Refused:
 * a src holding samples that dst holds or that dst's own slice may still draw (so: the same src twice, overlapping slices); another
 * film size, mode, shift mode, max_depth_override or block size; dst == src; NULL. src may live on another device: its planes are
 * copied into staging planes on dst's device (hipMemcpyPeerAsync on dst's stream; allocated by the first such merge). Both sessions
 * must be idle (every session call is blocking: a concern for callers with threads only). */
int gdpt_progressive_merge(GdptProgressive *dst, const GdptProgressive *src);

/* A group: the budget_spp of one session split over `num_devices` slice sessions, one per entry of `devices` (HIP ordinals; a device
 * may appear more than once; 1..GDPT_MULTI_MAX_DEVICES entries), each with its own uploaded scene and stream. Member i owns
 * [floor(i B / N), floor((i+1) B / N)) of the budget B. The total is an accumulator on devices[0]: a GdptProgressive that
 * gdpt_progressive_read / _reconstruct / _reconstruct_weighted / _status accept; add_pass / run / merge on it are refused.
 * Members on devices other than devices[0] reach the total through gdpt_progressive_merge's cross-device copy; the test of that path
 * (test_group_on_two_gpus) needs two GPUs, every other test runs the group with one device listed several times. */
typedef struct GdptProgressiveGroup GdptProgressiveGroup;   /* opaque */
int gdpt_progressive_group_create(const GdptSceneDesc *desc, const int32_t *devices, int num_devices,
                                  const GdptProgressiveConfig *config, GdptProgressiveGroup **out);
void gdpt_progressive_group_free(GdptProgressiveGroup *group);
/* Rounds: every member with budget left adds one pass of min(pass_spp, left), one host thread per member; then the total is
 * rebuilt: emptied, all members merged into it in member order (the bits do not depend on thread timing). With target_error > 0
 * the total is rebuilt after every round, otherwise once before the call returns. Stops when all slices are spent
 * (GDPT_STOP_BUDGET), max_rounds rounds were done by this call (GDPT_STOP_MAX_PASSES; <= 0: no limit), or K >= 2 and the total's
 * error estimate is <= target_error (GDPT_STOP_TARGET). status (nullable): the total's; totals.render_ms is the sum of the members'
 * device times. Blocking. */
int gdpt_progressive_group_run(GdptProgressiveGroup *group, double target_error, int pass_spp, int max_rounds,
                               GdptProgressiveStatus *status);
GdptProgressive *gdpt_progressive_group_total(GdptProgressiveGroup *group);   /* borrowed; valid until gdpt_progressive_group_free */
/* Two independent halves of the group's samples, for estimates that need them (gdpt_filter_select): two more accumulators beside the
 * total, on devices[0] and the total's stream, built and emptied like it. The members that hold samples, in member order, are merged
 * alternately into A and B; a round marks the halves stale together with the total, and this call rebuilds them if they are. Both
 * are borrowed, valid until gdpt_progressive_group_free, and are what the total is to gdpt_progressive_read and
 * gdpt_progressive_denoise_*; add_pass, run and merge refuse them as they refuse the total. Refused: fewer than two members with
 * samples. Blocking. */
int gdpt_progressive_group_halves(GdptProgressiveGroup *group, GdptProgressive **half_a, GdptProgressive **half_b);
int gdpt_progressive_group_member_status(const GdptProgressiveGroup *group, int member, GdptProgressiveStatus *status);

/* ---- variance-weighted reconstruction: generalised least squares on per-row confidences (not part of the reference) ----
 * gdpt_reconstruct's rows (data row per pixel, x-edge for x >= 1, y-edge for y >= 1, natural boundary), each weighted by a
 * confidence taken from the variance of its input: minimises  sum kappa_row |r_row|^2  with kappa ~ 1 / variance. A firefly sits in
 * a pixel whose sample variance is huge, so the row that carries it is all but switched off before the solve.
 * Variance planes var_c, var_gx, var_gy: W*H*3 doubles each, the variances of c, gx, gy (a session's assembled_vars). Per row:
 *     v      = sum of its three channel variances. The row is valid if they are finite and >= 0, v is finite, and the row's
 *              c / gx / gy triple is finite.
 *     s_d    = exp(mean(log v)) over the valid data rows with v > 0 (geometric mean: a few fireflies do not move it);
 *     s_g    = the same over the valid x- and y-edge rows together (one scale: their relative precision survives; the data rows'
 *              own scale keeps the meaning of dataCost). A family without such a row has scale 1.
 *     kappa  = s / (v + conf_floor s)  for a valid row (v = 0: 1 / conf_floor),  0 for an invalid row.
 * Round 0 solves gdpt_reconstruct's system with row weights kappa; IRLS round k >= 1 with kappa / (eps_k + |r|_2). A row with
 * kappa = 0 is selected out of the system (its values may be NaN); a pixel all of whose rows have kappa = 0 gets diagonal 1 and
 * right-hand side 0 (its value is 0) and is counted in pixels_isolated. The energies in the stats are sums of kappa |r|_2.
 * Uniform variance planes give one kappa for all rows, i.e. gdpt_reconstruct(GDPT_RECON_L1)'s image for the same round count.
 * recon.norm: GDPT_RECON_L2 = round 0 alone (weighted least squares; irls_iters is ignored), GDPT_RECON_L1 = weighted IRLS; the
 * other fields as for gdpt_reconstruct. params == NULL: weighted least squares with the defaults.
 * Weights estimated from the same samples as the means are correlated with them: a dark-biased estimate. */
typedef struct GdptWeightedReconParams {
    GdptReconParams recon;
    double conf_floor;         /* delta. 0: default 0.05; must be finite and >= 0 */
    int32_t reserved[2];       /* 0 */
} GdptWeightedReconParams;
typedef struct GdptWeightedReconStats {
    GdptReconStats recon;      /* norm: the one used; irls_rounds: systems solved (weighted L2: 1) */
    double scale_data;         /* s_d */
    double scale_grad;         /* s_g */
    uint64_t rows_dropped;     /* invalid rows */
    uint64_t pixels_isolated;
} GdptWeightedReconStats;
/* Host pointers. confidence (nullable; any entry nullable): kappa of the data, x-edge and y-edge rows, W*H doubles each (0 where
 * the film has no such row: x = 0, y = 0). NULL variance pointers, `out` aliasing an input, width or height < 2, a non-positive or
 * non-finite dataCost or conf_floor are refused. No CPU fallback. */
int gdpt_reconstruct_weighted(int width, int height, const double *c, const double *gx, const double *gy,
                              const double *var_c, const double *var_gx, const double *var_gy, double dataCost,
                              const GdptWeightedReconParams *params /* nullable */, double *out,
                              double *const confidence[3] /* nullable */, GdptWeightedReconStats *stats /* nullable */);
/* Device pointers (the confidence planes too). Waits for `stream`; scratch per (device, stream), dropped by
 * gdpt_poisson_forget_stream. */
int gdpt_reconstruct_weighted_device(int width, int height, const double *d_c, const double *d_gx, const double *d_gy,
                                     const double *d_var_c, const double *d_var_gx, const double *d_var_gy, double dataCost,
                                     const GdptWeightedReconParams *params /* nullable */, double *d_out,
                                     double *const d_confidence[3] /* nullable */, void *stream,
                                     GdptWeightedReconStats *stats /* nullable */);
/* The weighted reconstruction of a session: its running means assembled into c, cx, cy and its assembled variances, all on the
 * device. Needs a GradPath session with at least 2 passes (no variance is defined before). `out` and the confidence planes are
 * host memory, or device memory with on_device != 0. Blocking. */
int gdpt_progressive_reconstruct_weighted(GdptProgressive *session, double dataCost, const GdptWeightedReconParams *params /* nullable */,
                                          int on_device, double *out, double *const confidence[3] /* nullable */,
                                          GdptWeightedReconStats *stats /* nullable */);

/* ---- several devices of one node: the tile loop sharded into row bands ----
 * Replaces the reference's only parallelism, parallel_for over 16x16 tiles on a std::thread pool
 * (src/render.cpp:271-277, src/parallel.cpp:183-256): contiguous bands of whole tile rows go to the devices, one host
 * thread per device; between render and solve each device sends the last cy1 row of its band to the next one
 * (src/render.cpp:345-349 needs it), assembles c, cx, cy for its own band, and the three images are all-gathered in
 * place; the global solve runs on devices[0]. Results equal the single-device entry points bit for bit (same per-sample
 * RNG streams, same per-pixel summation order). */
#define GDPT_MULTI_MAX_DEVICES 16
/* Transport of the halo row and the all-gather.
 *   GDPT_EXCHANGE_RCCL:      ncclSend/ncclRecv + grouped in-place ncclAllGather (ncclBroadcast per band when the bands are
 *                            ragged) on one communicator per device; devices must be distinct. NOT YET RUN BETWEEN TWO
 *                            DEVICES (every box this library was developed on had one GPU): correct by construction
 *                            and by the one-device tests only. A failure behind the first collective aborts the
 *                            communicators (ncclCommAbort) and spends the handle: create a new one.
 *   GDPT_EXCHANGE_PEER_COPY: direct device-to-device copies (hipMemcpyPeerAsync over xGMI, ordered by events): every device
 *                            pushes its band to every other one, N-1 links at once. Accepts a device twice. */
enum { GDPT_EXCHANGE_RCCL = 0, GDPT_EXCHANGE_PEER_COPY = 1 };
typedef struct GdptMultiConfig {
    int32_t num_devices;       /* 1..GDPT_MULTI_MAX_DEVICES */
    int32_t exchange;          /* GDPT_EXCHANGE_* */
    int32_t devices[GDPT_MULTI_MAX_DEVICES];   /* HIP device ordinals, band order */
    int32_t balance;           /* 0: bands of equal tile-row count (gdpt_band_rows). 1: bands of equal measured cost — a pilot
                                  render (1 spp, first device, at create time) counts the rays of every tile row and the
                                  bands are cut by gdpt_band_rows_weighted */
    int32_t reserved;          /* 0 */
} GdptMultiConfig;
typedef struct GdptMultiStats {
    int32_t num_devices, exchange;
    int32_t row_begin[GDPT_MULTI_MAX_DEVICES], row_end[GDPT_MULTI_MAX_DEVICES];
    double render_ms[GDPT_MULTI_MAX_DEVICES];  /* device time of each band's render (HIP events) */
    double render_ms_max;      /* slowest band */
    double exchange_ms;        /* halo + assembly + all-gather, slowest device (includes waiting for the slowest band) */
    double solve_ms;           /* Poisson solve on devices[0] */
    double wall_ms;            /* host wall time of the call, D2H of the results included */
} GdptMultiStats;
typedef struct GdptMulti GdptMulti;   /* opaque: one uploaded scene, stream and image set per device (+ communicators) */

/* Rows [row_begin,row_end) of band `band` of `num_bands`: whole 16-pixel tile rows (src/render.cpp:271), balanced by
 * tile-row count, in band order. Host only. */
int gdpt_band_rows(int height, int num_bands, int band, int32_t *row_begin, int32_t *row_end);
/* The same with bands of (nearly) equal COST: tile_row_cost[t] >= 0 is the cost of tile row t (num_tile_rows =
 * ceil(height / 16) of them); the split minimises the cost of the most expensive band among all contiguous splits into
 * whole tile rows, rank-ordered. Host only. */
int gdpt_band_rows_weighted(int height, int num_bands, int band, const double *tile_row_cost, int num_tile_rows,
                            int32_t *row_begin, int32_t *row_end);
/* Cost of every 16-pixel tile row of the film: rays traced by a pilot render of that tile row alone at `spp` samples per
 * pixel (GDPT_RNG_SAMPLE, reference shift). Exact counts, so every caller — every rank of a sharded run — gets the same
 * numbers. `capacity` >= ceil(height / 16). Blocking; what the multi-device hosts balance their bands by. */
int gdpt_tile_row_costs(GdptScene *scene, int spp, double *cost, int capacity);
/* The same partition on a cost per pixel ROW (`row_cost[height]`), cuts on multiples of `granularity_rows` (1, 2, 4, 8 or 16): the
 * persistent kernels anchor their 16x16 work items at a band's first row, so a band of the GDPT_RNG_SAMPLE streams need not consist
 * of whole tile rows (GDPT_RNG_TILE does: granularity 16). Host only. */
int gdpt_band_rows_from_row_costs(int height, int num_bands, int band, const double *row_cost, int granularity_rows,
                                  int32_t *row_begin, int32_t *row_end);
int gdpt_multi_create(const GdptSceneDesc *desc, const GdptMultiConfig *config, GdptMulti **out);
/* Feedback between frames: `band_ms[i]` = measured render time of band i in the last call (GdptMultiStats.render_ms). The handle
 * keeps a cost model of the film's rows (uniform, or the pilot's with config.balance); every band's rows are rescaled so that the
 * band's modelled share equals its measured share, and the bands are cut again, on multiples of `granularity_rows`. Call between
 * two renders, from the thread that renders. The images of later calls differ from earlier ones in the last bits of their sums
 * (the work items follow the largest band, GdptRenderParams.plan_rows); GDPT_RNG_TILE renders need granularity 16. */
int gdpt_multi_rebalance(GdptMulti *multi, const double *band_ms, int granularity_rows);
void gdpt_multi_free(GdptMulti *multi);
/* Whole Integrator::GradPath on the device set; arguments as gdpt_gradient_path_render (params->row_begin/row_end
 * must be 0: the library chooses the bands). Blocking. */
int gdpt_multi_gradient_path_render(GdptMulti *multi, const GdptRenderParams *params, double dataCost, double *out_image,
                                    double *img, double *cx0, double *cy0, double *cx1, double *cy1,
                                    GdptRenderStats *rstats /* nullable */, GdptMultiStats *mstats /* nullable */);
/* gdpt_assemble_device restricted to rows [row_begin,row_end) (0,0 = all): what one band owner runs. */
int gdpt_assemble_rows_device(int width, int height, int row_begin, int row_end,
                              const double *d_img, const double *d_cx0, const double *d_cy0,
                              const double *d_cx1, const double *d_cy1,
                              double *d_c, double *d_cx, double *d_cy, void *stream);

/* ---- the error of the reconstructed image, from the members of a group (not part of the reference) ----
 * A session's error estimate is that of the PRIMAL mean; the image delivered is a reconstruction, whose error is several times
 * smaller and lies elsewhere on the film. The N members of a GdptProgressiveGroup hold N independent estimates of the same film over
 * disjoint sample slices; each can be reconstructed on its own, and the spread of those reconstructions measures the error of their
 * mean. Members i = 1..N with W_i > 0 samples per pixel and reconstructions f_i (W*H*3 doubles), per component:
 *     W = sum W_i;   fbar = sum W_i f_i / W;   M2 = sum W_i (f_i - fbar)^2;   var = M2 / ((N - 1) W)
 * computed with West's weighted update in member order (the fold's arithmetic with f_i in the place of a pass). If every f_i has
 * variance sigma^2 / W_i, var is an unbiased estimate of the variance of fbar; for N = 2 it is (W_a W_b / W^2) (f_a - f_b)^2.
 * The L2 reconstruction is linear in c, cx, cy: fbar IS the reconstruction of the merged total, up to rounding, and var estimates its
 * variance. L1 and the variance-weighted kinds are NOT linear: var then measures the spread of the members' reconstructions, not
 * the bias they share (every member reconstructs fewer samples than the total and is biased alike), and the total's reconstruction
 * is not fbar. The error estimate of the reconstruction is
 *     sqrt( sum var / sum f_tot^2 )   over pixels and channels,
 * f_tot the reconstruction of the total (the image delivered). A pixel is left out of both sums, and counted, if any member's triple,
 * the f_tot triple or the resulting var triple is not finite (the session's convention). The error map is var summed over the three
 * channels, per pixel (W*H doubles); with radius r >= 1 its mean over the (2r+1)^2 window clipped to the film, taken over the finite
 * entries alone (NaN where the window holds none). At N = 2 the raw map has one degree of freedom per pixel: use a window.
 * The sums are reduced in a fixed order: the same call gives the same bits. */
typedef struct GdptReconSpreadStats {
    int32_t members;           /* N */
    int32_t radius;            /* of the map's window */
    double error_estimate;     /* sqrt(sum_var / sum_sq) */
    double sum_var;
    double sum_sq;             /* sum f_tot^2 */
    uint64_t pixels_left_out;
    double spread_ms;          /* device time of the spread launches (statistic, reduction, window), HIP events */
} GdptReconSpreadStats;
/* The statistic alone, on any images: device pointers on the current device. d_images[n], weights[n]; d_total nullable: fbar takes
 * its place; d_var (W*H*3) and d_map (W*H) nullable. Refused: n < 2 or n > GDPT_MULTI_MAX_DEVICES, a non-positive or non-finite
 * weight, radius outside [0, 8], width or height < 1, an output that aliases an input (or the other output), NULL images.
 * Waits for `stream`; scratch per (device, stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_recon_spread_device(int width, int height, int n, const double *const *d_images, const double *weights,
                             const double *d_total /* nullable */, int radius, double *d_var /* nullable */, double *d_map /* nullable */,
                             void *stream, GdptReconSpreadStats *stats /* nullable */);
/* Host pointers. */
int gdpt_recon_spread(int width, int height, int n, const double *const *images, const double *weights, const double *total /* nullable */,
                      int radius, double *var /* nullable */, double *map /* nullable */, GdptReconSpreadStats *stats /* nullable */);

typedef struct GdptGroupReconParams {
    double dataCost;
    int32_t weighted;          /* 0: gdpt_progressive_reconstruct with `recon`; 1: gdpt_progressive_reconstruct_weighted with `wrecon` */
    int32_t map_radius;        /* 0..8 */
    GdptReconParams recon;
    GdptWeightedReconParams wrecon;
} GdptGroupReconParams;
/* The group's image with its error: rebuilds the total if it is stale; reconstructs every member that holds samples, one host thread
 * per member, each on its own device and stream (errors are reported after all threads have been joined); copies the images of
 * members on another device into staging on devices[0] (hipMemcpyPeerAsync on the total's stream; allocated on first use; NOT YET RUN
 * BETWEEN TWO DEVICES); reconstructs the total; runs the statistic above on the total's stream.
 * out_image: the total's reconstruction, bit for bit what gdpt_progressive_reconstruct[_weighted] on the total returns. out_map
 * (W*H) and out_var (W*H*3) nullable; host memory, or device memory on devices[0] with on_device != 0. recon_stats: the total's
 * (GdptReconStats; for weighted != 0 the `recon` part of its GdptWeightedReconStats). Refused: fewer than two members that hold
 * samples; for the weighted kinds a member used with fewer than 2 passes (the message names it); a Path group. Blocking. */
int gdpt_progressive_group_reconstruct_error(GdptProgressiveGroup *group, const GdptGroupReconParams *params, int on_device,
                                             double *out_image, double *out_map /* nullable */, double *out_var /* nullable */,
                                             GdptReconSpreadStats *spread_stats /* nullable */, GdptReconStats *recon_stats /* nullable */);
/* gdpt_progressive_group_run with the estimate above as the target: evaluated after every check_every-th round of this call
 * (<= 0: 1) from the round after which two members hold samples, and once before returning (spread_stats, nullable: that last one's;
 * zeroed if it could not be evaluated). Stops with GDPT_STOP_TARGET when the estimate is <= target_recon_error (<= 0: no target),
 * else as gdpt_progressive_group_run. status: the total's (its error_estimate stays the primal's). */
int gdpt_progressive_group_run_recon(GdptProgressiveGroup *group, double target_recon_error, int pass_spp, int max_rounds, int check_every,
                                     const GdptGroupReconParams *params, GdptProgressiveStatus *status,
                                     GdptReconSpreadStats *spread_stats /* nullable */);

/* ---- a variance-driven non-local-means filter for a mean and the variance of that mean (not part of the reference) ----
 * What a progressive session yields per pixel, a running mean u and the variance v of that mean, is what non-local means with
 * variance-cancelling patch distances takes (Rousselle, Knaus, Zwicker, "Adaptive rendering with non-local means filtering",
 * SIGGRAPH Asia 2012, sections 4-5). img, var: W*H*3 doubles, interleaved like every film here. Window radius r, patch radius f,
 * k > 0, alpha >= 0, epsilon > 0. A pixel is VALID if its three img and its three var values are finite and the var values >= 0.
 *   e_o(x) = (1/3) sum_c [ (u_c(x) - u_c(x+o))^2 - alpha (v_c(x) + min(v_c(x+o), v_c(x))) ] / [ epsilon + k^2 (v_c(x) + v_c(x+o)) ]
 *            for x and x+o both in the film and valid (such an x counts 1); otherwise 0, counting 0
 *   S_o(p) = sum of e_o(p+n) over |n|_inf <= f, C_o(p) the same sum of the counts;   D_o(p) = max(0, S_o(p) / C_o(p))
 *   w_o(p) = exp(-D_o(p)) if C_o(p) > 0 and p, p+o are both in the film and valid, else 0   (w_0(p) = 1)
 *   out_c(p) = sum_o w_o(p) u_c(p+o) / sum_o w_o(p),   var_out_c(p) = sum_o w_o(p)^2 v_c(p+o) / (sum_o w_o(p))^2
 * with the sums over |o|_inf <= r in row-major order of o. An invalid p keeps its input triples in out and var_out, bit for bit,
 * and is counted in pixels_left_out. r = 0 returns the input; f = 0 gives pixel-wise distances. 0 <= r <= 10, 0 <= f <= 3 (the
 * paper's defaults are the caps). The film sums run over the valid pixels and are reduced in a fixed order: the same call gives the
 * same bits. error_in = sqrt(sum_var_in / sum_sq_in) is the session's own error estimate restricted to the valid pixels;
 * error_out = sqrt(sum_var_out / sum_sq_out) treats the weights as fixed and independent of the data and ignores the filter's
 * bias: it is the variance the weighted average would have if its weights were given, not the error of the filtered image. */
typedef struct GdptNlmParams { int32_t window_radius, patch_radius; double k, alpha, epsilon; int32_t reserved[2]; } GdptNlmParams;
typedef struct GdptNlmStats  { uint64_t pixels_left_out; double sum_var_in, sum_sq_in, sum_var_out, sum_sq_out, error_in, error_out, filter_ms;
                               int32_t window_radius, patch_radius; } GdptNlmStats;
#define GDPT_NLM_MAX_WINDOW_RADIUS 10
#define GDPT_NLM_MAX_PATCH_RADIUS 3
void gdpt_nlm_default_params(GdptNlmParams *p);            /* 10, 3, 0.45, 1.0, 1e-10; every field of a passed struct is taken literally */
/* Device pointers on the current device. Refused, with a message that names the field, before any device call: NULL d_img, d_var or
 * d_out; d_out or d_var_out aliasing an input or each other; width or height < 1; radii outside the caps; a non-finite k, alpha or
 * epsilon, k <= 0, alpha < 0, epsilon <= 0; non-zero reserved. Enqueued on `stream`; with stats it waits for the stream (the sums
 * and filter_ms, HIP events, come back), with stats == NULL it only enqueues. Scratch (the block partials of the sums) per
 * (device, stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_denoise_nlm_device(int width, int height, const double *d_img, const double *d_var, const GdptNlmParams *params /* NULL: defaults */,
                            double *d_out, double *d_var_out /* nullable */, void *stream, GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm(int width, int height, const double *img, const double *var, const GdptNlmParams *params /* NULL: defaults */,
                     double *out, double *var_out /* nullable */, GdptNlmStats *stats /* nullable */);
/* The filter on a session's buffer 0: its running mean with the variance of that mean, the image of an Integrator::Path session and
 * the primal of a GradPath session (a group's total included). Needs at least 2 passes (no variance is defined before). `out` and
 * `var_out` (nullable) are host memory, or device memory with on_device != 0. Blocking. */
int gdpt_progressive_denoise(GdptProgressive *session, const GdptNlmParams *params /* NULL: defaults */, int on_device, double *out,
                             double *var_out /* nullable */, GdptNlmStats *stats /* nullable */);

/* ---- first-hit feature buffers with per-pixel variances (not part of the reference) ----
 * Albedo, shading normal, depth and coverage of a render's own base primary rays (Rousselle, Manzi, Zwicker, "Robust denoising using
 * feature and colour information", Pacific Graphics 2013, section 3): outputs in their own right, and the guide of
 * gdpt_denoise_nlm_guided below. mean, var: GDPT_FEATURE_CHANNELS planes of W*H doubles each, channel-PLANAR (plane c starts at c W H
 * and is row-major; the guided filter reads them plane by plane), not interleaved like the films.
 * GDPT_RNG_SAMPLE is the only scheme. Sample s of pixel (x, y) draws from stream (y W + x) stream_spp + first_sample + s (window ==
 * NULL: stream_spp = spp, first_sample = 0), takes the stream's first two numbers (rx, ry) as the sub-pixel position and makes the
 * camera ray of the render's own sample s: sample_primary(camera, (x + rx) / W, (y + ry) / H), with the texture footprint of a
 * primary ray (ray-differential spread 0.25 / max(W, H)). On a hit its eight values are
 *     0-2  albedo:   texture slot 0 of the hit's material, evaluated as a spectrum texture at the vertex (reflectance, base_color,
 *                    the rough lobes' first reflectance); (1, 1, 1) for GDPT_MAT_DISNEY_CLEARCOAT, whose slot 0 is a scalar
 *     3-5  normal:   the vertex's shading-frame normal, as interpolated (not flipped towards the ray)
 *     6    depth:    |position - ray origin|
 *     7    coverage: 1
 * and on a miss all eight are 0. Emission and environment maps play no part. Per pixel and channel the n = spp values x_1 .. x_n are
 * folded in sample order, i = 1 .. n:   d = x_i - mean;  mean += d / i;  M2 += d (x_i - mean);   var = M2 / (n (n - 1)), the variance
 * of the mean (0 for n = 1). A pixel whose samples all return one value has variance exactly 0; a pixel of hits only, or of misses
 * only, has coverage exactly 1 or 0.
 * params (NULL: the scene's spp, the whole film): spp (<= 0: the scene's), row_begin / row_end (rows outside the band are left
 * untouched); max_depth_override and plan_rows are ignored. Refused, with a message that names the field, before any device call:
 * a NULL scene, mean or var (or the two aliasing); GDPT_RNG_TILE or an unknown rng_scheme; shift_mode != 0; reserved != 0; a bad row
 * band; a window with stream_spp <= 0, first_sample < 0 or one that leaves [0, stream_spp).
 * It is not a render route and takes none of the handle's launch scratch: the kernel reads the scene and writes mean and var only,
 * so it is enqueued on `stream` as it is, beside whatever render of the same handle is in flight. With stats it waits for the stream
 * (samples, rays and render_ms are filled, the rest is 0); with stats == NULL it only enqueues. No CPU fallback. */
#define GDPT_FEATURE_CHANNELS 8   /* planes: 0-2 albedo, 3-5 shading normal, 6 depth, 7 coverage */
int gdpt_features_render_device(GdptScene *scene, const GdptRenderParams *params /* nullable */, const GdptSampleWindow *window /* nullable */,
                                double *d_mean, double *d_var, void *stream, GdptRenderStats *stats /* nullable */);
/* Host pointers. Blocking. */
int gdpt_features_render(GdptScene *scene, const GdptRenderParams *params /* nullable */, const GdptSampleWindow *window /* nullable */,
                         double *mean, double *var, GdptRenderStats *stats /* nullable */);

/* ---- the non-local-means filter guided by features (not part of the reference) ----
 * gdpt_denoise_nlm's weights come from colour alone: detail that is small against the noise (a texture, an edge between surfaces of
 * similar radiance, a crease) is smoothed away. Here a feature distance caps the colour weight (Rousselle, Manzi, Zwicker 2013,
 * section 4). feat, feat_var: num_channels <= GDPT_NLM_MAX_CHANNELS planes of W*H doubles, channel-planar as above: any planar array
 * and the variance of it, not only a feature render's. A group j names the channels C_j = [first_channel, first_channel +
 * num_channels) that are compared together, with a floor tau_j > 0 on the variance in the denominator (a squared feature value:
 * what counts as "the same" where the feature is noise-free).
 * The definition extends gdpt_denoise_nlm's. A pixel is VALID if it is valid there and every channel that some group names is finite
 * at it, with variance >= 0. For valid p and p+o, g the features and s their variances:
 *   phi_j(p,o) = (1/|C_j|) sum_{c in C_j} [ (g_c(p) - g_c(p+o))^2 - alpha_f (s_c(p) + min(s_c(p+o), s_c(p))) ]
 *                                          / [ k_f^2 max(tau_j, s_c(p) + s_c(p+o)) ]       (channels summed in index order)
 *   D^f_o(p)   = max(0, max_j phi_j(p,o))                                                   (0 with no group)
 *   w_o(p)     = exp(-max(D_o(p), D^f_o(p)))
 * and e_o, S, C, D_o, out, var_out, the film sums and pixels_left_out are gdpt_denoise_nlm's. The feature term is a term of the pixel
 * pair (p, p+o), not of a patch. Features only ever lower a weight: num_groups = 0, or features constant over the film with variance
 * 0, give gdpt_denoise_nlm's result bit for bit; the gain shows once the colour term is loosened (k towards 1). */
#define GDPT_NLM_MAX_GROUPS 4
#define GDPT_NLM_MAX_CHANNELS 16
typedef struct GdptNlmFeatureGroup { int32_t first_channel, num_channels; double tau; } GdptNlmFeatureGroup;
typedef struct GdptNlmGuide { int32_t num_channels, num_groups; GdptNlmFeatureGroup groups[GDPT_NLM_MAX_GROUPS];
                              double k_f, alpha_f; int32_t reserved[2]; } GdptNlmGuide;
void gdpt_nlm_default_guide(GdptNlmGuide *g);   /* 8 channels; groups {0,3,1e-3} albedo, {3,3,1e-3} normal; k_f 0.6; alpha_f 1 */
/* Device pointers on the current device. What gdpt_denoise_nlm_device refuses is refused, and, naming the field: num_channels outside
 * [0, 16]; num_groups outside [0, 4]; a group that leaves [0, num_channels) or has fewer than 1 channel; tau <= 0 or non-finite;
 * k_f <= 0 or non-finite; alpha_f < 0 or non-finite; non-zero reserved; NULL d_feat or d_feat_var when num_groups > 0; an output
 * aliasing any input. guide == NULL: gdpt_nlm_default_guide. Enqueue-only with stats == NULL; scratch as gdpt_denoise_nlm_device. */
int gdpt_denoise_nlm_guided_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                                   double *d_out, double *d_var_out /* nullable */, void *stream, GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm_guided(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                            const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                            double *out, double *var_out /* nullable */, GdptNlmStats *stats /* nullable */);
/* The guided filter on a session's buffer 0 (as gdpt_progressive_denoise: at least 2 passes, a group's total included), guided by the
 * features of the session's film: gdpt_features_render_device on the session's stream with feature_spp samples of the window
 * {stream_spp = budget_spp, first_sample = 0}, the camera rays of the session's own first samples; 2 <= feature_spp <= budget_spp.
 * guide->num_channels must be GDPT_FEATURE_CHANNELS. features, features_var (nullable): receive the 8 planes. All output pointers
 * are host memory, or device memory with on_device != 0. Blocking. */
int gdpt_progressive_denoise_guided(GdptProgressive *session, const GdptNlmParams *params /* NULL: defaults */,
                                    const GdptNlmGuide *guide /* NULL: defaults */, int feature_spp, int on_device, double *out,
                                    double *var_out /* nullable */, double *features /* nullable */, double *features_var /* nullable */,
                                    GdptNlmStats *stats /* nullable */);

/* ---- a first-order feature regression on the non-local-means weights (not part of the reference) ----
 * Every filter above is a weighted mean, which is biased wherever the signal has a gradient inside the window; the guide's only
 * answer is to lower weights. Here the weights stay and the weighted mean becomes a weighted linear fit of the colour on feature
 * planes inside the window, read at the centre pixel (Bitterli, Rousselle, Moon, Iglesias-Guitian, Adler, Mitchell, Jarosz, Novak,
 * "Nonlinearly weighted first-order regression for denoising Monte Carlo renderings", EGSR 2016, section 4; the successor of
 * Rousselle, Manzi, Zwicker 2013): where the colour is locally affine in the regressors the bias vanishes.
 * The definition extends gdpt_denoise_nlm_guided's; img, var, feat, feat_var, GdptNlmParams and GdptNlmGuide are its. The regressors
 * are m = num_regressors planes c_j = channel[j-1], j = 1 .. m, each divided by scale[j-1] > 0; d = 1 + m unknowns per colour channel.
 * A pixel is VALID if it is valid for the guided filter and every regressor plane is finite at it with variance >= 0 (the channels
 * that count are those of the groups together with those of the regressors). On this validity, for valid p and p+o:
 *   w_o(p)   = the guided filter's weight exp(-max(D_o(p), D^f_o(p))), 0 as there   (w_0(p) = 1)
 *   z_0      = 1,   z_j(p,o) = (g_{c_j}(p+o) - g_{c_j}(p)) / scale[j-1]
 *   A_ij     = sum_o (w_o z_i) z_j  (i >= j; A is symmetric),   b_c,i = sum_o (w_o z_i) u_c(p+o),   W = A_00 = sum_o w_o
 *              every entry accumulated on its own over |o|_inf <= r in row-major order of o; then A_jj += ridge W for j >= 1
 * A is symmetric positive definite: the tap o = 0 gives e_0 e_0^T with weight 1, every other diagonal entry gets ridge W >= ridge > 0.
 * Four right-hand sides, A beta_c = b_c (c = 0, 1, 2) and A q = e_0, are solved by LDL^T without pivoting; no square root is taken.
 * The order, every sum running over k in index order, subtracted term by term from its first operand:
 *   for j = 0 .. d-1:   t_k = L_jk D_k (k < j);   D_j = A_jj - sum_{k<j} L_jk t_k;
 *                       for i = j+1 .. d-1:   L_ij = (A_ij - sum_{k<j} L_ik t_k) / D_j
 *   for i = 0 .. d-1:   y_i = rhs_i - sum_{k<i} L_ik y_k;       then y_i = y_i / D_i for every i;
 *   for i = d-1 .. 0:   x_i = y_i - sum_{k>i} L_ki x_k
 *   out_c(p)     = beta_c[0]
 *   var_out_c(p) = sum_o (w_o(p) l_o(p))^2 v_c(p+o),   l_o = q_0 + sum_{j=1..m} q_j z_j(p,o) (terms added in index order)
 * var_out is the variance of the linear estimator under fixed weights and carries the caveat of error_out above. An invalid p keeps
 * its input triples bit for bit and is counted; the film sums and GdptNlmStats are gdpt_denoise_nlm's. r = 0 returns the input bits
 * (W = 1, every z = 0). m = 0 is the guided filter, out = (sum w u) / W and var_out = sum (w / W)^2 v, equal to
 * gdpt_denoise_nlm_guided's up to the rounding of where the division stands, not bit for bit.
 * Defaults: the six planes 0 .. 5 (albedo and shading normal of a feature render), every scale 1, ridge 1e-2. Depth has no default
 * scale as it has no default tau: its unit is the scene's. These rest on a synthetic film alone. */
#define GDPT_NLM_MAX_REGRESSORS 7
typedef struct GdptNlmRegress { int32_t num_regressors; int32_t channel[GDPT_NLM_MAX_REGRESSORS];
                                double scale[GDPT_NLM_MAX_REGRESSORS]; double ridge; int32_t reserved[2]; } GdptNlmRegress;
void gdpt_nlm_default_regress(GdptNlmRegress *r);   /* 6 regressors: planes 0..5 (albedo, normal), every scale 1.0, ridge 1e-2 */
/* Device pointers on the current device. What gdpt_denoise_nlm_guided_device refuses is refused, and, naming the field:
 * num_regressors outside [0, 7]; a channel outside [0, guide->num_channels); a channel listed twice; a scale that is non-finite or
 * <= 0; a ridge that is non-finite or <= 0; non-zero reserved; NULL d_feat or d_feat_var when num_regressors > 0 or num_groups > 0.
 * params, guide == NULL: gdpt_nlm_default_params, gdpt_nlm_default_guide (the library picks no other k or groups for the regression;
 * the lajolla CLI does); regress == NULL: gdpt_nlm_default_regress. Enqueue-only with stats == NULL; scratch per (device, stream)
 * as gdpt_denoise_nlm_device. When neither d_var_out nor stats is asked for, the second sweep over the window is not run. */
int gdpt_denoise_nlm_regress_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                    const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                                    const GdptNlmRegress *regress /* NULL: defaults */, double *d_out, double *d_var_out /* nullable */,
                                    void *stream, GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm_regress(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                             const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                             const GdptNlmRegress *regress /* NULL: defaults */, double *out, double *var_out /* nullable */,
                             GdptNlmStats *stats /* nullable */);
/* The regression on a session's buffer 0, built as gdpt_progressive_denoise_guided in every respect: the session renders its features
 * on its stream, at least 2 passes, a group's total included, 2 <= feature_spp <= budget_spp; guide->num_channels must be
 * GDPT_FEATURE_CHANNELS. Blocking. */
int gdpt_progressive_denoise_regress(GdptProgressive *session, const GdptNlmParams *params /* NULL: defaults */,
                                     const GdptNlmGuide *guide /* NULL: defaults */, const GdptNlmRegress *regress /* NULL: defaults */,
                                     int feature_spp, int on_device, double *out, double *var_out /* nullable */,
                                     double *features /* nullable */, double *features_var /* nullable */, GdptNlmStats *stats /* nullable */);

/* ---- the collaborative form of the first-order regression (not part of the reference) ----
 * gdpt_denoise_nlm_regress keeps of every window's fit its value at the centre alone. The fit is a model for every pixel of its
 * window, so a pixel can take the weighted average of all fits whose windows cover it, about (2r+1)^2 estimates in the place of one
 * (Bitterli et al. 2016, "collaborative filtering"). Where the point estimate's error is variance, not bias, this lowers it.
 * The inputs, the validity rule, w_o(p), z(p,o), A, b_c, the ridge and the LDL^T order are exactly gdpt_denoise_nlm_regress's, d = 1 + m.
 *   1. Fit. For every valid p the whole solution beta_c(p) in R^d, c = 0, 1, 2, is kept in a coefficient film of 3 d channel-planar
 *      planes of width * height doubles: plane c d + j holds beta_c,j. An invalid p stores beta_c,0 = u_c(p) (its input bits) and 0.0
 *      elsewhere; nothing reads it.
 *   2. Gather. For every valid q, over the offsets t with |t|_inf <= r in row-major order of t, with p = q + t inside the film and valid:
 *        omega_t(q) = w_{-t}(p), the weight the fit centred at p gave its partner q. Neither the pair distance nor the feature
 *                     distance is symmetric in its variances: the patch distance is sum_n e(p+n; q+n) with the centre's triple
 *                     first, summed and counted over the same patch taps n in the same order as the fit's S_o, C_o, and the feature
 *                     distance takes p in the centre's place and q in the partner's.
 *        y_c        = beta_c,0(p) + sum_{j=1..m} beta_c,j(p) z_j,   z_j = (g_{c_j}(q) - g_{c_j}(p)) / scale[j-1]
 *                     (terms added in index order; the division is skipped at scale 1)
 *        N_c += omega y_c,   Omega += omega;   out_c(q) = N_c / Omega.   The tap t = 0 has omega = 1, so Omega >= 1.
 *   3. An invalid q keeps its input triple bit for bit and is counted once in pixels_left_out; an invalid p contributes to nobody.
 *   4. There is NO var_out. The variance of this estimator under fixed weights is a double sum over the window, O(r^4) per pixel, and a
 *      cheap surrogate would be a number with no meaning. GdptNlmStats.sum_var_out and .error_out are NaN: "not estimated". To learn
 *      where the collaborative image beats another filter's, use the two-half estimate of gdpt_progressive_group_denoise_select's
 *      kind (gdpt_filter_select), which needs no candidate variance. sum_var_in, sum_sq_in, sum_sq_out, error_in, pixels_left_out,
 *      the radii and filter_ms (both passes) are as everywhere.
 * Exact by construction: r = 0 returns the input bits; no pass writes a plane it reads; the same call gives the same bits (a gather,
 * no atomics); the coefficient plane c d + 0 equals gdpt_denoise_nlm_regress's out channel c bit for bit.
 * Refused: what gdpt_denoise_nlm_regress_device refuses, the field named, and a d_coef whose 3 d planes overlap an input or d_out.
 * d_coef == NULL: the film is kept in the library's scratch per (device, stream), 24 width height doubles at d = 8, grown on demand
 * and dropped by gdpt_poisson_forget_stream. Enqueue-only with stats == NULL. Quality rests on a synthetic film alone (DESIGN.md
 * section 4.16). */
int gdpt_denoise_nlm_collab_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                   const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                                   const GdptNlmRegress *regress /* NULL: defaults */, double *d_out,
                                   double *d_coef /* nullable: 3 (1 + m) planes */, void *stream, GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. coef (nullable) receives the coefficient film. */
int gdpt_denoise_nlm_collab(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                            const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                            const GdptNlmRegress *regress /* NULL: defaults */, double *out, double *coef /* nullable */,
                            GdptNlmStats *stats /* nullable */);
/* The collaborative regression on a session's buffer 0, built as gdpt_progressive_denoise_regress in every respect (Path sessions,
 * GradPath primals, a group's total; at least 2 passes; the coefficient film is the library's). Blocking. */
int gdpt_progressive_denoise_collab(GdptProgressive *session, const GdptNlmParams *params /* NULL: defaults */,
                                    const GdptNlmGuide *guide /* NULL: defaults */, const GdptNlmRegress *regress /* NULL: defaults */,
                                    int feature_spp, int on_device, double *out, double *features /* nullable */,
                                    double *features_var /* nullable */, GdptNlmStats *stats /* nullable */);

/* ---- an edge-avoiding a-trous wavelet filter with variance-guided weights: the cheap filter (not part of the reference) ----
 * Every filter above weighs a (2r+1)^2 window by patch distances, 441 offsets of 49 patch taps at the defaults. This one runs L
 * passes of a 5x5 B3-spline kernel whose taps are spread by 1, 2, 4, ... pixels, 25 L taps per pixel, and reaches +-62 pixels in five
 * passes (Dammertz, Sewtz, Hanika, Lensch, "Edge-avoiding A-Trous wavelet transform for fast global illumination filtering", HPG
 * 2010; Schied et al., "Spatiotemporal variance-guided filtering", HPG 2017). The edge-stopping weight is the distance the filters
 * above already use: e_o(p) of gdpt_denoise_nlm at patch radius 0, capped by the feature distance of gdpt_denoise_nlm_guided; the
 * filter can sit between the two steps of gdpt_denoise_nlm_demod (GdptNlmDemod, below).
 * Inputs: those of gdpt_denoise_nlm_guided (img, var W*H*3 doubles, interleaved; feat, feat_var num_channels channel-planar planes; a
 * GdptNlmGuide, NULL or no group: no feature term) and an optional GdptNlmDemod. Parameters: 1 <= levels, 0 <= first_level,
 * first_level + levels <= GDPT_ATROUS_MAX_LEVELS; level i = 0 .. levels-1 uses the step s_i = 2^(first_level + i); k, alpha, epsilon
 * as gdpt_denoise_nlm's.
 * A pixel is VALID if it is valid for the guided filter on (img, var, the groups' channels) and, with a demod block, its albedo and
 * coverage values are valid as gdpt_denoise_nlm_demod defines them. The valid set is fixed by the inputs: it is the same at every
 * level. An invalid pixel keeps its input bits in out and var_out, is counted once in pixels_left_out and is never a tap.
 *   1. u_0 = u, v_0 = v; with a demod block the quotients u / a~, v / a~^2 of step 1 of gdpt_denoise_nlm_demod, in those operations.
 *   2. for each level i and valid p, over the taps (a, b) in {-2..2}^2, a the row, b the column, in row-major order, o = (b s_i, a s_i),
 *      a tap counting only if p+o lies in the film and is valid:
 *        e   = e_o(p) of gdpt_denoise_nlm on u_i, v_i: the channel terms summed as (t0 + t1) + t2 and divided by 3;   D = max(0, e)
 *        D^f = the guided filter's feature distance of the pair (p, p+o) on feat, feat_var (the same at every level; no group: 0)
 *        w   = (h_a h_b) exp(-max(D, D^f)),   h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *        Wsum += w,   num_c += w u_i,c(p+o),   vnum_c += (w w) v_i,c(p+o)
 *      u_{i+1},c(p) = num_c / Wsum,   v_{i+1},c(p) = vnum_c / (Wsum Wsum).   The centre tap has D = 0 and weight 9/64, so Wsum > 0.
 *      Every level reads the previous level's planes only, never its own output.
 *   3. out = u_L, var_out = v_L; with a demod block multiplied back as in step 3 of gdpt_denoise_nlm_demod.
 * GdptNlmStats: sum_var_in, sum_sq_in over the original var and img of the valid pixels, sum_var_out, sum_sq_out over the final
 * outputs; window_radius reports the reach 2 s of the last level, patch_radius 0; filter_ms covers all levels. var_out takes the
 * weights as fixed AND ignores the correlation that earlier levels introduce between pixels: from the second level on the taps are
 * no longer independent, so var_out (and error_out with it) underestimates, more than error_out of the filters above already does.
 * Exact, bit for bit: one call with levels = n equals n successive calls with levels = 1 and first_level = f, f + 1, ..., each fed
 * the previous call's out and var_out, when there is no demod block; no group, or features that are constant over the film with
 * variance 0, give the unguided result; a demod block with albedo 1 and coverage 1 gives the undemodulated result. */
#define GDPT_ATROUS_MAX_LEVELS 6
typedef struct GdptAtrousParams { int32_t levels, first_level; double k, alpha, epsilon; int32_t reserved[2]; } GdptAtrousParams;
void gdpt_atrous_default_params(GdptAtrousParams *p);   /* 5, 0, 2.0, 1.0, 1e-10 */
struct GdptNlmDemod;   /* defined with gdpt_denoise_nlm_demod, below */
/* Device pointers on the current device; one kernel per level, enqueued on `stream`. Refused before any device call, naming the field:
 * NULL d_img, d_var or d_out; an output aliasing an input or the other output; width or height < 1; levels or first_level outside
 * their ranges; k, alpha, epsilon non-finite or outside gdpt_denoise_nlm's ranges; non-zero reserved; num_channels outside [0,
 * GDPT_NLM_MAX_CHANNELS]; what gdpt_denoise_nlm_demod_device refuses for the guide and the demod block; NULL d_feat or d_feat_var when
 * a group or a demod block needs them. Enqueue-only with stats == NULL; scratch (the sums and the planes between the levels) per
 * (device, stream) as gdpt_denoise_nlm_device, dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_denoise_atrous_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                               int num_channels, const GdptAtrousParams *params /* NULL: defaults */,
                               const GdptNlmGuide *guide /* NULL: no feature term, as in the demod entries */,
                               const struct GdptNlmDemod *demod /* NULL: no demodulation */, double *d_out, double *d_var_out /* nullable */,
                               void *stream, GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_atrous(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                        int num_channels, const GdptAtrousParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: none */,
                        const struct GdptNlmDemod *demod /* NULL: none */, double *out, double *var_out /* nullable */,
                        GdptNlmStats *stats /* nullable */);
/* The filter on a session's buffer 0, built as gdpt_progressive_denoise_demod: the session renders its features on its stream, at
 * least 2 passes, Path sessions, the primal of GradPath sessions and a group's total, 2 <= feature_spp <= budget_spp; a guide's
 * num_channels must be GDPT_FEATURE_CHANNELS. With neither a group nor a demod block no features are rendered, feature_spp is ignored
 * and features, features_var must be NULL. Blocking. */
int gdpt_progressive_denoise_atrous(GdptProgressive *session, const GdptAtrousParams *params /* NULL: defaults */,
                                    const GdptNlmGuide *guide /* NULL: none */, const struct GdptNlmDemod *demod /* NULL: none */,
                                    int feature_spp, int on_device, double *out, double *var_out /* nullable */,
                                    double *features /* nullable */, double *features_var /* nullable */, GdptNlmStats *stats /* nullable */);

/* ---- the non-local-means filter on the albedo-demodulated mean (not part of the reference) ----
 * The guided filter keeps a texture only by lowering weights across albedo differences: exactly where a surface is textured fewer
 * pixels are averaged and more noise stays. Here the illumination is filtered, not the colour: the mean is divided by the first-hit
 * albedo, the quotient is filtered, and the albedo is multiplied back. The texture is carried by a nearly noise-free buffer and is
 * restored exactly, and pixels on either side of a texel edge average each other freely. Inputs as gdpt_denoise_nlm_guided (img, var
 * interleaved; feat, feat_var channel-planar, num_channels planes) and a block GdptNlmDemod: the albedo is planes albedo_channel ..
 * albedo_channel + 2, the coverage plane coverage_channel (-1: none, cov = 1 everywhere). The EFFECTIVE ALBEDO of channel c = 0..2 is
 *   a~_c(p) = max(floor, a_c(p) + (1 - cov(p)))
 * (a feature render's albedo mean already averages zeros for misses: a background pixel gets a~ = 1, an edge pixel something in
 * between). The albedo's own variance is NOT used: the variance planes of the albedo and of the coverage are read for validity only.
 * A pixel is VALID if it is valid for the guided filter (for gdpt_denoise_nlm when there is no guide), its three albedo values are
 * finite with variances finite and >= 0, and, with a coverage channel, its coverage is finite with variance finite and >= 0.
 *   1. u'_c = u_c / a~_c,   v'_c = v_c / (a~_c a~_c)                          (in exactly these operations)
 *   2. O, VO = the definition of gdpt_denoise_nlm (no guide) or gdpt_denoise_nlm_guided on (u', v'); features and groups untouched
 *   3. out_c = O_c a~_c,    var_out_c = VO_c (a~_c a~_c)
 * An invalid pixel keeps its input bits and is counted, as there. The film sums stay in the colour domain: sum_var_in and sum_sq_in
 * are sums of the original v and u (gdpt_denoise_nlm's, bit for bit, when the valid sets agree), sum_var_out and sum_sq_out are sums
 * of the remodulated outputs; error_out keeps its meaning and its weakness. r = 0 returns (u / a~) a~, which is not always the input
 * bits. Exact: albedo 1 with coverage 1, or albedo 0 with coverage 0, give the undemodulated result bit for bit; multiplying img and
 * the albedo planes by a per-pixel power of two m and var by m^2 (nothing at the floor, coverage 1) multiplies out by m and var_out
 * by m^2, bit for bit. */
typedef struct GdptNlmDemod { int32_t albedo_channel, coverage_channel; double floor; int32_t reserved[2]; } GdptNlmDemod;
void gdpt_nlm_default_demod(GdptNlmDemod *d);   /* {0, 7, 1e-3, {0, 0}}: the layout of a feature render */
/* Device pointers on the current device. guide == NULL here means NO feature term (in the guided entries NULL is the default guide):
 * on the 15 % albedo checker of tests/nlm_guided_ref.py demodulating and also guiding by albedo measured 0.70 - 0.75 of the unfiltered
 * RMSE at k = 0.45 against 0.59 - 0.66 for demodulating alone; the albedo is already divided out, so the guide only takes samples
 * away. A non-NULL guide must have guide->num_channels == num_channels. demod == NULL: gdpt_nlm_default_demod. What
 * gdpt_denoise_nlm_guided_device refuses is refused, and, naming the field: num_channels outside [0, 16]; albedo_channel outside
 * [0, num_channels - 3]; coverage_channel outside [-1, num_channels) or inside the albedo triple; a non-finite floor or floor <= 0;
 * non-zero reserved; NULL d_feat or d_feat_var. Enqueue-only with stats == NULL; scratch as gdpt_denoise_nlm_device. No CPU fallback. */
int gdpt_denoise_nlm_demod_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                  int num_channels, const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: none */,
                                  const GdptNlmDemod *demod /* NULL: defaults */, double *d_out, double *d_var_out /* nullable */, void *stream,
                                  GdptNlmStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm_demod(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                           int num_channels, const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: none */,
                           const GdptNlmDemod *demod /* NULL: defaults */, double *out, double *var_out /* nullable */,
                           GdptNlmStats *stats /* nullable */);
/* The demodulated filter on a session's buffer 0, built as gdpt_progressive_denoise_guided: the session renders its features on its
 * stream (feature_spp samples of the window {budget_spp, 0}; 2 <= feature_spp <= budget_spp) and divides by their albedo; at least 2
 * passes; Path, the primal of GradPath, a group's total. The planes are a feature render's: a guide must have num_channels ==
 * GDPT_FEATURE_CHANNELS, and demod's channels lie within them. Blocking. */
int gdpt_progressive_denoise_demod(GdptProgressive *session, const GdptNlmParams *params /* NULL: defaults */,
                                   const GdptNlmGuide *guide /* NULL: none */, const GdptNlmDemod *demod /* NULL: defaults */, int feature_spp,
                                   int on_device, double *out, double *var_out /* nullable */, double *features /* nullable */,
                                   double *features_var /* nullable */, GdptNlmStats *stats /* nullable */);

/* ---- smoothing the variance that drives the non-local-means filters (not part of the reference) ----
 * The three filters above take their weights from the per-pixel variance of a session's mean, which a session estimates from its K
 * pass means: with K - 1 degrees of freedom the estimate has a relative error of sqrt(2 / (K - 1)), 141 % at K = 2, 82 % at K = 4.
 * Every patch distance divides by v(p) + v(q) and subtracts alpha (v(p) + min(v(q), v(p))), so that noise goes straight into the
 * weights: at 2 passes the filters at their defaults do nothing. The pre-pass here replaces the variance with its mean over a
 * (2 radius + 1)^2 window; the filters are then run, unchanged, on what it writes (DESIGN.md 4.10 has the measurements, and the
 * remedies that lost). Radiance is albedo x illumination, so on a textured surface the variance carries the albedo squared, and a mean
 * in the colour domain smears it across texel edges: with a block GdptNlmDemod the mean is taken of v / a~^2 and a~^2 is multiplied back.
 * Inputs: img, var W*H*3 doubles, interleaved; optionally feat, feat_var, num_channels channel-planar planes, and a block GdptNlmDemod
 * over them (all three or none). 0 <= radius <= GDPT_VAR_SMOOTH_MAX_RADIUS.
 * A pixel is VALID as for gdpt_denoise_nlm (its img and var triples finite, var >= 0); with a demod block it must also be valid as
 * gdpt_denoise_nlm_demod asks without a guide (its albedo triple and, with a coverage channel, its coverage finite, with variances
 * finite and >= 0). a~ is the EFFECTIVE ALBEDO of gdpt_denoise_nlm_demod, max(floor, a_c + (1 - cov)); without a demod block a~ = 1
 * and nothing is multiplied or divided. For valid p, q ranging over the valid pixels of the film with |q - p|_inf <= radius:
 *   n_c(q)       = v_c(q) / (a~_c(q) a~_c(q))
 *   S_c(p)       = sum_q n_c(q): row sums of 2 radius + 1 taps in increasing x, starting from 0.0, then the sum of those row sums in
 *                  increasing y, starting from 0.0; a tap outside the film or on an invalid pixel counts as 0.0
 *   C(p)         = the number of those q   (>= 1: p itself)
 *   var_out_c(p) = (S_c(p) / C(p)) (a~_c(p) a~_c(p))
 * An invalid p keeps its input bits in var_out and is counted in pixels_left_out. sum_var_in and sum_var_out are the sums of var and
 * of var_out over the valid pixels (per pixel (c0 + c1) + c2), reduced in a fixed order: the same call gives the same bits.
 * Exact, bit for bit: radius 0 without a demod block returns var (a variance of -0.0 comes back as +0.0); a var that is one dyadic
 * constant over the film comes back unchanged (the sums of at most 81 equal dyadic terms and their quotient are exact; without a demod
 * block); var times a per-film power of two multiplies var_out by it (short of overflow and subnormals). */
#define GDPT_VAR_SMOOTH_MAX_RADIUS 4
typedef struct GdptVarSmoothParams { int32_t radius; int32_t reserved[3]; } GdptVarSmoothParams;
typedef struct GdptVarSmoothStats  { uint64_t pixels_left_out; double sum_var_in, sum_var_out, smooth_ms; int32_t radius; } GdptVarSmoothStats;
void gdpt_var_smooth_default_params(GdptVarSmoothParams *p);      /* radius 2; every field of a passed struct is taken literally */
/* Device pointers on the current device. d_feat, d_feat_var and demod go together: all NULL (a~ = 1; num_channels is ignored) or all
 * given (NULL demod does NOT mean the default block here). Refused, with a message that names the field, before any device call: NULL
 * d_img, d_var or d_var_out; d_var_out aliasing an input; width or height < 1; radius outside [0, 4]; non-zero reserved; a demod block
 * without d_feat or d_feat_var, or planes without a demod block; what gdpt_denoise_nlm_demod_device refuses in a demod block and
 * num_channels. params == NULL: gdpt_var_smooth_default_params. Enqueued on `stream`; with stats it waits for the stream (the sums and
 * smooth_ms, HIP events, come back), with stats == NULL it only enqueues. Scratch (the block partials of the sums) per (device,
 * stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_variance_smooth_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat /* nullable */,
                                const double *d_feat_var /* nullable */, int num_channels, const GdptVarSmoothParams *params /* NULL: defaults */,
                                const GdptNlmDemod *demod /* NULL: none */, double *d_var_out, void *stream,
                                GdptVarSmoothStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_variance_smooth(int width, int height, const double *img, const double *var, const double *feat /* nullable */,
                         const double *feat_var /* nullable */, int num_channels, const GdptVarSmoothParams *params /* NULL: defaults */,
                         const GdptNlmDemod *demod /* NULL: none */, double *var_out, GdptVarSmoothStats *stats /* nullable */);
/* One of the three session filters on the smoothed variance of buffer 0. By definition the outputs are, bit for bit, those of this
 * chain on the session's stream: gdpt_progressive_read (the mean and variance of buffer 0); for GUIDED and DEMOD
 * gdpt_features_render_device as gdpt_progressive_denoise_guided renders it; gdpt_variance_smooth_device with `smooth` (for DEMOD on the
 * rendered planes with the filter's own demod block, otherwise a~ = 1); then gdpt_denoise_nlm_device (PLAIN),
 * gdpt_denoise_nlm_guided_device (GUIDED) or gdpt_denoise_nlm_demod_device (DEMOD) with the smoothed variance in the place of var.
 * So var_out and stats (sum_var_in and error_in included) are those of the SMOOTHED variance, not of the session's own estimate.
 * smooth, nlm: NULL = defaults. guide: PLAIN must be NULL; GUIDED NULL = the default guide; DEMOD NULL = no feature term. demod: DEMOD
 * only, NULL = the default block. feature_spp, features, features_var: as gdpt_progressive_denoise_guided; PLAIN ignores feature_spp
 * and refuses the two pointers. smoothed_var (nullable) receives the smoothed variance, W*H*3. Requirements and refusals otherwise as
 * the three session calls: at least 2 passes; Path, the primal of GradPath, a group's total. All output pointers are host memory, or
 * device memory with on_device != 0. Blocking. */
#define GDPT_DENOISE_PLAIN 0
#define GDPT_DENOISE_GUIDED 1
#define GDPT_DENOISE_DEMOD 2
int gdpt_progressive_denoise_smoothed(GdptProgressive *session, int kind, const GdptVarSmoothParams *smooth /* NULL: defaults */,
                                      const GdptNlmParams *nlm /* NULL: defaults */, const GdptNlmGuide *guide /* nullable */,
                                      const GdptNlmDemod *demod /* nullable */, int feature_spp, int on_device, double *out,
                                      double *var_out /* nullable */, double *smoothed_var /* nullable */, double *features /* nullable */,
                                      double *features_var /* nullable */, GdptNlmStats *stats /* nullable */,
                                      GdptVarSmoothStats *smooth_stats /* nullable */);

/* ---- a multi-scale (pyramid) form of the non-local-means filters (not part of the reference) ----
 * A window of radius 10 averages at most 441 pixels, so the error of a block mean over 8 x 8 pixels or more passes the three filters
 * almost untouched: the blotches of a smooth wall. Here a pyramid is filtered, and each level's low frequencies are replaced by the
 * filtered coarser level (Burt and Adelson's Laplacian pyramid; Boughida and Boubekeur, "Bayesian collaborative denoising for Monte
 * Carlo rendering", EGSR 2017, section 5). DESIGN.md 4.11 has the measurements.
 * A KIND is GDPT_DENOISE_PLAIN, GUIDED or DEMOD: gdpt_denoise_nlm, gdpt_denoise_nlm_guided or gdpt_denoise_nlm_demod with their blocks,
 * by the conventions of gdpt_progressive_denoise_smoothed: PLAIN takes no block and no planes (guide, demod, feat, feat_var NULL);
 * GUIDED takes a guide (NULL: the default guide) and no demod block; DEMOD takes a demod block (NULL: the default block) and a guide
 * or none (NULL: no feature term). With planes, a guide must have guide->num_channels == num_channels. Level 0 is the call's input:
 * img, var (interleaved) and, for GUIDED and DEMOD, feat, feat_var (num_channels planar planes). A pixel of a level is VALID exactly
 * as the kind's filter defines validity on that level's arrays.
 * DOWN (level l -> l+1): W' = (W + 1) / 2, H' = (H + 1) / 2 in integer division. Coarse pixel (X, Y) covers the fine pixels
 *   (2X + dx, 2Y + dy), dx, dy in {0, 1}, that lie in the film; n of them are valid. Every coarse value (three img, three var, every
 *   feature plane and its variance plane) is summed from 0.0 in the order (dx, dy) = (0,0), (1,0), (0,1), (1,1) over the valid pixels
 *   only; a mean is divided by n, a variance by n n. With n = 0 every coarse value is NaN, so the coarse pixel is invalid for every
 *   kind by the definitions above and no mask is carried.
 * LEVELS: 1 <= levels <= GDPT_NLM_MAX_LEVELS. Level l+1 exists if l + 1 < levels and W_l H_l > 1; the stats report the levels made.
 * FILTER: F_l, VF_l are out and var_out of the kind's filter on level l, with the call's GdptNlmParams, guide and demod unchanged.
 * UP AND COMBINE, from the coarsest level L down: out_L = F_L. For a coarse pixel with n > 0, R(X, Y) = out_{l+1}(X, Y) - DF(X, Y),
 *   DF the Down mean of F_l over the same valid pixels; with n = 0, R = 0.0. For a valid fine pixel (x, y): X = x >> 1,
 *   X* = clamp(X + (x odd ? 1 : -1), 0, W' - 1), Y and Y* likewise, and per channel, in exactly this order and without contraction,
 *     out_l = F_l + (((0.5625 R(X,Y) + 0.1875 R(X*,Y)) + 0.1875 R(X,Y*)) + 0.0625 R(X*,Y*))
 *   An invalid fine pixel keeps its input bits.
 * OUTPUTS: out = out_0. var_out = VF_0, the finest level's: THE CORRECTION IS IGNORED IN IT, it is the variance of the single-scale
 * weighted average with fixed weights, not that of out. pixels_left_out is level 0's.
 * Exact, bit for bit: levels = 1 gives the kind's existing entry point's out, var_out and stats; a film that is one dyadic constant
 * with a dyadic constant variance comes back unchanged at every level count (every sum, quotient and the four dyadic weights are
 * exact; with planes, where they are dyadic constants of variance 0, so that every weight is 1 and the albedo divides exactly); the
 * same call gives the same bits. */
#define GDPT_NLM_MAX_LEVELS 4
typedef struct GdptNlmPyramidOpStats { uint64_t pixels_left_out, cells_empty; double op_ms; int32_t coarse_width, coarse_height; } GdptNlmPyramidOpStats;
typedef struct GdptNlmPyramidStats { int32_t levels, reserved; int32_t width[GDPT_NLM_MAX_LEVELS], height[GDPT_NLM_MAX_LEVELS];
                                     GdptNlmStats level[GDPT_NLM_MAX_LEVELS]; double total_ms; } GdptNlmPyramidStats;
/* Down alone, device pointers on the current device: level (width, height) into d_*_out of ((width + 1) / 2, (height + 1) / 2).
 * d_feat_out, d_feat_var_out go with d_feat, d_feat_var (all four or none; with none num_channels is ignored). Refused, with a message
 * that names the field, before any device call: NULL d_img, d_var, d_img_out or d_var_out; an output aliasing an input or another
 * output; width or height < 1; an unknown kind; blocks or planes that do not fit the kind (above); what the kind's filter refuses in
 * a guide, a demod block and num_channels; missing planes where the kind reads some (GUIDED with groups, DEMOD). Enqueued on `stream`;
 * with stats it waits for the stream (pixels_left_out: the invalid fine pixels; cells_empty: the coarse pixels with n = 0; op_ms, HIP
 * events), with stats == NULL it only enqueues. Scratch per (device, stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_nlm_pyramid_down_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat /* nullable */,
                                 const double *d_feat_var /* nullable */, int num_channels, int kind, const GdptNlmGuide *guide /* nullable */,
                                 const GdptNlmDemod *demod /* nullable */, double *d_img_out, double *d_var_out, double *d_feat_out /* nullable */,
                                 double *d_feat_var_out /* nullable */, void *stream, GdptNlmPyramidOpStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_nlm_pyramid_down(int width, int height, const double *img, const double *var, const double *feat /* nullable */,
                          const double *feat_var /* nullable */, int num_channels, int kind, const GdptNlmGuide *guide /* nullable */,
                          const GdptNlmDemod *demod /* nullable */, double *img_out, double *var_out, double *feat_out /* nullable */,
                          double *feat_var_out /* nullable */, GdptNlmPyramidOpStats *stats /* nullable */);
/* Up and combine alone: the fine level's inputs (read for validity, and img for the bits of an invalid pixel), d_filtered = F_l of
 * (width, height), d_coarse_out = out_{l+1} of the coarse extent, into d_out of (width, height). Refusals as the down entry's, with
 * NULL d_filtered, d_coarse_out or d_out and d_out aliasing an input. cells_empty comes back 0. */
int gdpt_nlm_pyramid_up_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat /* nullable */,
                               const double *d_feat_var /* nullable */, int num_channels, int kind, const GdptNlmGuide *guide /* nullable */,
                               const GdptNlmDemod *demod /* nullable */, const double *d_filtered, const double *d_coarse_out, double *d_out,
                               void *stream, GdptNlmPyramidOpStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_nlm_pyramid_up(int width, int height, const double *img, const double *var, const double *feat /* nullable */,
                        const double *feat_var /* nullable */, int num_channels, int kind, const GdptNlmGuide *guide /* nullable */,
                        const GdptNlmDemod *demod /* nullable */, const double *filtered, const double *coarse_out, double *out,
                        GdptNlmPyramidOpStats *stats /* nullable */);
/* The multi-scale filter. By definition the outputs are, bit for bit, those of the composition on `stream` of
 * gdpt_nlm_pyramid_down_device, the kind's device filter (gdpt_denoise_nlm_device, gdpt_denoise_nlm_guided_device or
 * gdpt_denoise_nlm_demod_device) on every level and gdpt_nlm_pyramid_up_device. Refused, with a message that names the field, before
 * any device call: what the kind's filter refuses; levels outside [1, GDPT_NLM_MAX_LEVELS]; an unknown kind; blocks or planes that do
 * not fit the kind; d_out or d_var_out aliasing an input or each other. params == NULL: gdpt_nlm_default_params. With stats it waits
 * for the stream after every level's filter (a GdptNlmStats per level, the levels made, their extents; total_ms spans the call, HIP
 * events); with stats == NULL it only enqueues. The pyramid and the levels' outputs are kept per (device, stream), dropped by
 * gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_denoise_nlm_multiscale_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat /* nullable */,
                                       const double *d_feat_var /* nullable */, int num_channels, int kind, int levels,
                                       const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* nullable */,
                                       const GdptNlmDemod *demod /* nullable */, double *d_out, double *d_var_out /* nullable */, void *stream,
                                       GdptNlmPyramidStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm_multiscale(int width, int height, const double *img, const double *var, const double *feat /* nullable */,
                                const double *feat_var /* nullable */, int num_channels, int kind, int levels,
                                const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* nullable */,
                                const GdptNlmDemod *demod /* nullable */, double *out, double *var_out /* nullable */,
                                GdptNlmPyramidStats *stats /* nullable */);
/* The multi-scale filter on a session's buffer 0. By definition the outputs are, bit for bit, those of this chain on the session's
 * stream: gdpt_progressive_read (the mean and variance of buffer 0); for GUIDED and DEMOD gdpt_features_render_device as
 * gdpt_progressive_denoise_guided renders it; with smooth != NULL gdpt_variance_smooth_device as gdpt_progressive_denoise_smoothed
 * runs it on level 0 (smooth == NULL: the variance as estimated); then gdpt_denoise_nlm_multiscale_device. nlm, guide, demod,
 * feature_spp, features, features_var: as gdpt_progressive_denoise_smoothed takes them for the kind. Requirements as the three session
 * calls: at least 2 passes; Path, the primal of GradPath, a group's total. All output pointers are host memory, or device memory
 * with on_device != 0. Blocking. */
int gdpt_progressive_denoise_multiscale(GdptProgressive *session, int kind, int levels, const GdptVarSmoothParams *smooth /* NULL: none */,
                                        const GdptNlmParams *nlm /* NULL: defaults */, const GdptNlmGuide *guide /* nullable */,
                                        const GdptNlmDemod *demod /* nullable */, int feature_spp, int on_device, double *out,
                                        double *var_out /* nullable */, double *features /* nullable */, double *features_var /* nullable */,
                                        GdptNlmPyramidStats *stats /* nullable */);

/* ---- choosing among candidate filters per pixel, by the error two half sessions estimate of each (not part of the reference) ----
 * Which denoiser is best changes from region to region and with the sample count (DESIGN.md 4.14 has the measurements). Two
 * independent half sessions A and B of one film give an honest estimate: filter A with a candidate F; u_B is independent of F(A) and
 * has variance v_B, so (F(A) - u_B)^2 - v_B is an unbiased estimate of the squared error of F(A), bias included, and likewise with
 * the halves exchanged (the two-buffer estimate of Rousselle, Manzi and Zwicker, "Robust denoising using feature and color
 * information", 2013, section 5, and of Bitterli et al., "Nonlinearly weighted first-order regression for denoising Monte Carlo
 * renderings", 2016, section 5). Averaged over a small window, the candidate with the smallest estimate is taken per pixel.
 * Inputs: n candidates, 1 <= n <= GDPT_SELECT_MAX_CANDIDATES; every plane W*H*3 doubles, interleaved. uA, vA, uB, vB: the two halves'
 * means and the variances of those means. FA[j], FB[j]: candidate j run on each half. T[j]: the image to deliver for candidate j
 * (the candidate on all samples). 0 <= radius s <= GDPT_SELECT_MAX_RADIUS.
 * A pixel is VALID if its triples of uA, vA, uB, vB and of every FA[j], FB[j], T[j] are finite and its vA and vB are >= 0.
 * For a valid pixel q and channel c, every operation rounded on its own (no contraction):
 *   t_c(q) = 0.5 * (((FA_j,c - uB_c) (FA_j,c - uB_c) - vB_c) + ((FB_j,c - uA_c) (FB_j,c - uA_c) - vA_c))
 *   e_j(q) = ((t_0 + t_1) + t_2) / 3.0
 *   S_j(p) = the sum of e_j(q), C(p) = the number, of the valid q with |q - p|_inf <= s: row sums of 2s + 1 taps in increasing x,
 *            starting from 0.0, then the sum of those row sums in increasing y, starting from 0.0; a tap outside the film or on an
 *            invalid pixel counts as 0.0 (the order of gdpt_variance_smooth)
 *   E_j(p) = S_j(p) / C(p)
 *   sel(p) = the smallest j whose E_j(p) is minimal: j is scanned upward and replaces the best on strict <
 *   out(p) = T[sel(p)](p), bit for bit;  mse(p) = E_sel(p)(p), which may be negative
 * An invalid p has out(p) = T[0](p) bit for bit, sel(p) = -1, mse(p) = NaN (and E_j(p) = NaN) and is counted in pixels_left_out.
 * Stats: chosen[j], the valid pixels with sel = j; sum_e[j], the film sum of the unsmoothed e_j over the valid pixels; sum_mse, the film
 * sum of E_sel; sum_sq_out, that of out squared per pixel; all reduced in a fixed order: the same call gives the same bits.
 * WHAT THE NUMBERS ARE. e_j estimates the error of candidate j run on HALF the samples; the delivered T[j] is the candidate on all of
 * them, and that it is no worse is expected, not measured. mse and sum_mse are minima over noisy estimates and are biased low; by how
 * much, and with what sign the film figure comes out, is not established (DESIGN.md 4.14 has what was measured). sum_e[j], taken before any selection, is the unbiased figure. No stopping rule
 * is built on any of them.
 * Exact, bit for bit: n = 1 returns T[0]; a candidate listed twice never loses to its copy; permuting the candidates permutes sel and
 * leaves out alone where no two E_j are equal; s = 0 gives E = e; every image times 2^m and every variance times 4^m leaves sel alone
 * and multiplies mse by 4^m (short of overflow and subnormals). */
#define GDPT_SELECT_MAX_CANDIDATES 8
#define GDPT_SELECT_MAX_RADIUS 8
typedef struct GdptSelectParams { int32_t radius; int32_t reserved[3]; } GdptSelectParams;
typedef struct GdptSelectStats  { uint64_t pixels_left_out; uint64_t chosen[GDPT_SELECT_MAX_CANDIDATES]; double sum_e[GDPT_SELECT_MAX_CANDIDATES];
                                  double sum_mse, sum_sq_out, select_ms; int32_t radius, num_candidates; } GdptSelectStats;
void gdpt_select_default_params(GdptSelectParams *p);      /* radius 4; every field of a passed struct is taken literally */
/* Device pointers on the current device; d_FA, d_FB, d_T are host arrays of n device pointers. d_sel (int32, W*H), d_mse (W*H) and
 * d_E (n*W*H: plane j holds E_j) are nullable. Refused, with a message that names the field, before any device call: n out of range;
 * a NULL image or d_out; an output that overlaps an input or another output anywhere in its extent; width or height < 1; radius outside [0, 8]; non-zero
 * reserved. params == NULL: gdpt_select_default_params. Enqueued on `stream`: one launch, which writes no plane it reads; with stats
 * it waits for the stream (the sums and select_ms, HIP events, come back), with stats == NULL it only enqueues. Scratch (the block
 * partials of the sums) per (device, stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_filter_select_device(int width, int height, int n, const double *const *d_FA, const double *const *d_FB, const double *const *d_T,
                              const double *d_uA, const double *d_vA, const double *d_uB, const double *d_vB,
                              const GdptSelectParams *params /* NULL: defaults */, double *d_out, int32_t *d_sel /* nullable */,
                              double *d_mse /* nullable */, double *d_E /* nullable */, void *stream, GdptSelectStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_filter_select(int width, int height, int n, const double *const *FA, const double *const *FB, const double *const *T, const double *uA,
                       const double *vA, const double *uB, const double *vB, const GdptSelectParams *params /* NULL: defaults */, double *out,
                       int32_t *sel /* nullable */, double *mse /* nullable */, double *E /* nullable */, GdptSelectStats *stats /* nullable */);

/* The selection among filters of a progressive group, behind one call. A candidate names one of the session filters and its blocks:
 * filter GDPT_SELECT_MEAN (the unfiltered mean; no block), _NLM (gdpt_progressive_denoise), _NLM_GUIDED (_denoise_guided), _NLM_DEMOD
 * (_denoise_demod), _NLM_REGRESS (_denoise_regress), _ATROUS (_denoise_atrous; `atrous` in the place of `nlm`), _NLM_COLLAB
 * (_denoise_collab; the blocks of _NLM_REGRESS; its cand_stats entry carries sum_var_out = error_out = NaN, as that entry's stats do:
 * the selection needs no candidate variance, and is the tool that tells per pixel whether it beats _NLM_REGRESS). var_smooth_radius: -1
 * for none; >= 0 runs the candidate through gdpt_progressive_denoise_smoothed at that radius and is allowed for _NLM, _NLM_GUIDED and
 * _NLM_DEMOD only. NULL pointers mean what they mean in the matching gdpt_progressive_denoise_* entry; a block the filter does not take
 * must be NULL.
 * By definition the outputs are, bit for bit, those of this chain on the total's stream: the halves (gdpt_progressive_group_halves) and
 * the total are made current; for each candidate and each of A, B and the total, the candidate's session entry into a film the group
 * owns (GDPT_SELECT_MEAN: gdpt_progressive_read of buffer 0); gdpt_progressive_read of the halves' means and variances;
 * gdpt_filter_select_device with T[j] the candidate on the total. If any candidate needs feature planes they are rendered once, as
 * gdpt_progressive_denoise_guided renders them, by the first such run on the total, and shared by all 3n runs (the three sessions
 * share one scene, budget and stream). features, features_var (nullable) receive them from that run on the
 * total. Each half needs at least 2 passes: the message names the half and its members. Path groups and the primal of GradPath groups
 * are served. sel (int32, W*H) and mse (W*H) are nullable; cand_stats (nullable, n entries) receives the GdptNlmStats of every
 * candidate's run on the total (zeros for GDPT_SELECT_MEAN). The 3n filtered films and the halves' planes are owned by the group and
 * freed with it. All output pointers are host memory, or device memory on devices[0] with on_device != 0. Refused before any device
 * work, with the field named: n out of range, NULL candidates or out, an unknown filter, a var_smooth_radius outside [-1, 4] or on a
 * filter that does not take one, a block the filter does not take, radius outside [0, 8], non-zero reserved. Blocking. */
#define GDPT_SELECT_MEAN 0
#define GDPT_SELECT_NLM 1
#define GDPT_SELECT_NLM_GUIDED 2
#define GDPT_SELECT_NLM_DEMOD 3
#define GDPT_SELECT_NLM_REGRESS 4
#define GDPT_SELECT_ATROUS 5
#define GDPT_SELECT_NLM_COLLAB 6
typedef struct GdptSelectCandidate { int32_t filter; int32_t var_smooth_radius; const GdptNlmParams *nlm; const GdptAtrousParams *atrous;
                                     const GdptNlmGuide *guide; const GdptNlmDemod *demod; const GdptNlmRegress *regress; } GdptSelectCandidate;
int gdpt_progressive_group_denoise_select(GdptProgressiveGroup *group, const GdptSelectCandidate *candidates, int n,
                                          const GdptSelectParams *select_params /* NULL: defaults */, int feature_spp, int on_device, double *out,
                                          int32_t *sel /* nullable */, double *mse /* nullable */, double *features /* nullable */,
                                          double *features_var /* nullable */, GdptSelectStats *stats /* nullable */,
                                          GdptNlmStats *cand_stats /* nullable */);

/* ---- joint filtering: the non-local-means weights of one film applied to companion films (not part of the reference) ----
 * Every filter above writes one film. A GradPath session holds three that belong together, the assembled c, cx, cy: here the weights
 * are computed once, from a GUIDE FILM and its variance (optionally capped by the feature guide), and applied to n COMPANION FILMS and
 * their variances as well (the joint filtering step of Manzi, Vicini, Zwicker, "Regularizing image reconstruction for gradient-domain
 * rendering with feature patches", Eurographics 2016, and of Rousselle, Jarosz, Novak, "Image-space control variates for rendering",
 * SIGGRAPH Asia 2016, without their regularisers). The filtered variances are what gdpt_reconstruct_weighted takes.
 * The definition extends gdpt_denoise_nlm_guided's; img, var (the guide film), feat, feat_var, GdptNlmParams and GdptNlmGuide are its.
 * comp[j], comp_var[j], 0 <= j < n, 0 <= n <= GDPT_NLM_JOINT_MAX: W*H*3 doubles each, interleaved like every film.
 * A pixel is VALID if it is valid for gdpt_denoise_nlm_guided, every companion triple at it is finite, and every companion variance at
 * it is finite and >= 0. w_o(p) is gdpt_denoise_nlm_guided's weight over THIS validity; out, var_out of the guide film are defined as
 * there, and for every companion, over the same offsets in the same row-major order,
 *   comp_out_j,c(p)     = sum_o w_o(p) a_j,c(p+o) / sum_o w_o(p)
 *   comp_var_out_j,c(p) = sum_o w_o(p)^2 s_j,c(p+o) / (sum_o w_o(p))^2        (a_j = comp[j], s_j = comp_var[j])
 * An invalid p keeps every input triple, the guide film's and the companions', bit for bit, and is counted once in
 * guide.pixels_left_out. GdptNlmJointStats.guide is the GdptNlmStats of the guide film; sum_var_in[j], sum_var_out[j] are the sums of
 * comp_var[j] and comp_var_out[j] over the valid pixels (per pixel (c0 + c1) + c2), reduced in the same fixed order; entries j >= n
 * are 0. Exact, bit for bit:
 *   - with every companion valid everywhere, out, var_out and stats.guide (but filter_ms) are gdpt_denoise_nlm_guided's; so with n = 0,
 *     and with num_groups = 0 they are gdpt_denoise_nlm's;
 *   - a companion that is the guide film itself (comp[j] = img, comp_var[j] = var) comes back as out, var_out;
 *   - r = 0 returns every input. */
#define GDPT_NLM_JOINT_MAX 4
typedef struct GdptNlmJointStats { GdptNlmStats guide; double sum_var_in[GDPT_NLM_JOINT_MAX], sum_var_out[GDPT_NLM_JOINT_MAX]; } GdptNlmJointStats;
/* Device pointers on the current device; d_comp, d_comp_var, d_comp_out, d_comp_var_out are host arrays of n device pointers. What
 * gdpt_denoise_nlm_guided_device refuses is refused, and, naming the field, before any device call: n outside [0, 4]; with n > 0 a NULL
 * d_comp, d_comp_var or d_comp_out, or a NULL entry of one of them (d_comp_var_out, and any entry of it, is nullable); any output whose
 * byte range overlaps an input's or another output's. guide == NULL: gdpt_nlm_default_guide; guide->num_groups == 0 takes NULL d_feat,
 * d_feat_var. Enqueued on `stream`; with stats it waits for the stream, with stats == NULL it only enqueues. Scratch per (device,
 * stream), dropped by gdpt_poisson_forget_stream. No CPU fallback. */
int gdpt_denoise_nlm_joint_device(int width, int height, const double *d_img, const double *d_var, const double *d_feat, const double *d_feat_var,
                                  int n, const double *const *d_comp, const double *const *d_comp_var,
                                  const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                                  double *d_out, double *d_var_out /* nullable */, double *const *d_comp_out,
                                  double *const *d_comp_var_out /* nullable */, void *stream, GdptNlmJointStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_denoise_nlm_joint(int width, int height, const double *img, const double *var, const double *feat, const double *feat_var,
                           int n, const double *const *comp, const double *const *comp_var,
                           const GdptNlmParams *params /* NULL: defaults */, const GdptNlmGuide *guide /* NULL: defaults */,
                           double *out, double *var_out /* nullable */, double *const *comp_out, double *const *comp_var_out /* nullable */,
                           GdptNlmJointStats *stats /* nullable */);
/* The joint filter on a GradPath session, then the reconstruction of what it wrote. By definition the outputs are, bit for bit, those
 * of this chain on the session's stream: the running means assembled into c, cx, cy (gdpt_assemble_device) and the assembled_vars of
 * gdpt_progressive_read; with var_smooth != NULL gdpt_variance_smooth_device (a~ = 1) on (c, var c), its output taking var c's place
 * as the guide film's variance only; with guide != NULL gdpt_features_render_device as gdpt_progressive_denoise_guided renders it
 * (guide == NULL: no feature term and no render; feature_spp is ignored); gdpt_denoise_nlm_joint_device with the guide film (c, var c)
 * and the companions (cx, var cx), (cy, var cy); then, with weighted_recon == NULL, gdpt_reconstruct_device (L2) on the filtered c, cx,
 * cy, otherwise gdpt_reconstruct_weighted_device on them with the FILTERED variances (its recon.norm selects weighted L2 or L1).
 * filtered, filtered_var (nullable; any entry nullable): receive the filtered c, cx, cy and their variances. recon_stats (nullable):
 * with weighted_recon its fields are filled, otherwise recon_stats->recon alone. Needs a GradPath session with at least 2 passes, a
 * group's total and its halves included; an Integrator::Path session is refused by name. All output pointers are host memory, or
 * device memory with on_device != 0. Blocking. */
int gdpt_progressive_denoise_reconstruct(GdptProgressive *session, const GdptNlmParams *nlm /* NULL: defaults */,
                                         const GdptNlmGuide *guide /* NULL: unguided */, int feature_spp,
                                         const GdptVarSmoothParams *var_smooth /* NULL: none */, double dataCost,
                                         const GdptWeightedReconParams *weighted_recon /* NULL: L2 */, int on_device, double *out,
                                         double *const filtered[3] /* nullable */, double *const filtered_var[3] /* nullable */,
                                         GdptNlmJointStats *stats /* nullable */, GdptWeightedReconStats *recon_stats /* nullable */);

/* ---- a new camera on an uploaded scene (not part of the reference) ----
 * Replaces the camera of the handle: renders and feature renders enqueued before the call keep the old camera (the camera travels
 * with each launch as a kernel argument), those enqueued after it use the new one. Everything an upload derives from the camera is
 * derived again by the upload's own code. Refused, naming the field, before any device call and with the handle unchanged: a NULL
 * scene or camera; a width, height, filter_type or filter_param other than the uploaded camera's (the film and everything sized by it
 * stay as uploaded); a non-finite entry of sample_to_cam or cam_to_world; a camera position that would enlarge the extent from which
 * the upload derived the padding of the tree's boxes (max |coordinate| over the scene's bounds, its spheres and the uploaded camera's
 * position): the tree is not rebuilt, and the padding must stay sufficient for rays that start at the camera. For every accepted
 * camera every render and feature entry of the handle returns, bit for bit, what a fresh gdpt_scene_upload of the same description
 * with desc.camera replaced returns. The call takes no lock: it must not run beside another call on the same handle from another
 * thread (a render call reads the camera while it enqueues). A live GdptProgressive session of the handle holds no camera of its own:
 * its passes after the call render with the new camera and fold into the statistics of the old one, so a session is closed, or a new
 * one created, across the call (Temporal.frame and lajolla --frames make one session a frame). */
int gdpt_scene_set_camera(GdptScene *scene, const GdptCamera *camera);

/* ---- temporal reprojection: accumulate frames across a camera move (not part of the reference) ----
 * A progressive session is temporal accumulation under a fixed camera: a running mean with a variance of the mean. This carries the
 * accumulated mean U, its variance of the mean V and the history length N through a camera move: each push reprojects them through
 * the new frame's first-hit depth, rejects history where depth or normal disagree, and blends the new frame in (the temporal half of
 * Schied et al., "Spatiotemporal variance-guided filtering", HPG 2017). The outputs are a mean and a variance of the mean, what every
 * filter above takes. The history holds the unfiltered accumulation; nothing but the camera may move; an environment-map background
 * is not reprojected by direction (background pixels restart every frame); GradPath gradients go through
 * gdpt_temporal_push_gradients (below), not through this push.
 * A handle is bound to (width, height, device, stream) and owns two sets of history planes that alternate, so no launch writes a plane
 * it reads: U and V (W*H*3 doubles, interleaved like the films), N (W*H doubles), the previous frame's unit normal (3 planes), depth
 * and coverage planes, and the previous camera. One kernel per push, enqueued on the handle's stream.
 * Inputs of a push: the frame's camera; img = u, var = v (W*H*3 doubles, interleaved); feat: the GDPT_FEATURE_CHANNELS planes of a
 * feature render of that frame (planar), of which planes 3-5 (normal), 6 (depth) and 7 (coverage) are read.
 * M(camera) = inverse(sample_to_cam) inverse(cam_to_world), 4x4 row-major, computed on the host in fp64 (gdpt_temporal_world_to_sample
 * returns it); org(camera) is the camera position of an upload, cam_to_world (0, 0, 0). For pixel p = (x, y) of the current frame:
 *   LEFT OUT    any of u_c(p), v_c(p) non-finite, or a v_c(p) < 0: out, var_out keep the input's bits, N' = 0, counted in
 *               pixels_left_out; the pixel is never a valid tap later.
 *   BACKGROUND  otherwise, coverage(p) not > 0: out = u, var_out = v, N' = 1, counted in pixels_background; never a valid tap.
 *   SURFACE     otherwise. d = depth(p) / coverage(p) (the depth plane is a mean over hits and misses); n^ = the normal planes
 *               divided by their length, (0, 0, 0) for a length not > 0, which means RESET.
 *     X = org + d dir, (org, dir) the camera ray through the pixel centre: pt = sample_to_cam ((x + 1/2) / W, (y + 1/2) / H, 0)
 *     as a point, dir = normalize(cam_to_world normalize(pt)) as a vector.
 *     (sx, sy, ., w) = M(prev) (X, 1). RESET unless w > 0.
 *     q = (sx / w W - 1/2, sy / w H - 1/2). RESET unless -1 <= q_x <= W and -1 <= q_y <= H (no tap lies in the film otherwise).
 *     i0 = floor(q_x), j0 = floor(q_y), f_x = q_x - i0, f_y = q_y - j0. The taps t = (i0 + a, j0 + b), a, b in {0, 1}, have the
 *     bilinear weights b_t = (a ? f_x : 1 - f_x) (b ? f_y : 1 - f_y). A tap is VALID if it lies in the film, N_prev(t) >= 1,
 *     coverage_prev(t) > 0, |d_prev(t) - e| <= tau_z e with e = |X - org(prev)|, n^_prev(t) is not (0, 0, 0) (a pixel without a
 *     normal is never a tap, at any tau_n), and n^ . n^_prev(t) >= tau_n.
 *     S = sum of b_t over the valid taps, in the order (a, b) = (0,0), (1,0), (0,1), (1,1), as every sum below.
 *     RESET       S < s_min, or the first push after create or reset: out = u, var_out = v, N' = 1, counted in pixels_reset.
 *     otherwise   U = (sum b_t U_prev(t)) / S,  V = (sum (b_t b_t) V_prev(t)) / (S S),  N = (sum b_t N_prev(t)) / S;
 *                 N' = min(N + 1, max_history),  alpha = 1 / N',  out = U + alpha (u - U),
 *                 var_out = ((1 - alpha) (1 - alpha)) V + (alpha alpha) v;  where N' = 1 (alpha = 1) out = u and var_out = v, the
 *                 input's bits, and the pixel is not counted as reset.
 *   The new history is (out, var_out, N', n^, d, coverage) of the pixel (n^ = d = 0 where none was formed).
 * V takes the four taps as independent, the convention of every var_out here: neighbouring history pixels that were themselves
 * interpolated from common taps are correlated, so var_out underestimates. Defaults: tau_z 0.05, tau_n 0.9, s_min 1e-3, max_history
 * 32; apart from max_history the customary SVGF-style values, not tuned on any scene of this project.
 * Identities, exact: max_history = 1 returns the input bits always; so do the first push and the push after a reset, with N' = 1 on
 * every surface and background pixel.
 * GdptTemporalStats: the three pixel counts, sum_history = the sum of N' over the film (fixed order: the same bits every time), push_ms
 * around the kernel. */
typedef struct GdptTemporalParams { double tau_z, tau_n, s_min; int32_t max_history; int32_t reserved[3]; } GdptTemporalParams;
typedef struct GdptTemporalStats  { uint64_t pixels_left_out, pixels_background, pixels_reset; double sum_history, push_ms; } GdptTemporalStats;
typedef struct GdptTemporal GdptTemporal;   /* opaque */
void gdpt_temporal_default_params(GdptTemporalParams *p);   /* 0.05, 0.9, 1e-3, 32; every field of a passed struct is taken literally */
/* stream: a hipStream_t, NULL the null stream. Refused: NULL out, width or height < 1 or a film too large, a negative device index.
 * Makes no device call: the planes are allocated by the first push, which fails on a device that does not exist. */
int gdpt_temporal_create(int width, int height, int device, void *stream, GdptTemporal **out);
void gdpt_temporal_free(GdptTemporal *t);   /* waits for the handle's stream first */
int gdpt_temporal_reset(GdptTemporal *t);   /* the next push is a first push; host only, enqueues nothing */
/* M(camera) of the definition. Refused: NULL arguments, a non-finite entry, a singular matrix. Host only. */
int gdpt_temporal_world_to_sample(const GdptCamera *camera, double M[16]);
/* Device pointers on the handle's device; enqueued on the handle's stream. Refused before any device call, naming the field: a NULL
 * handle, camera, d_img, d_var, d_feat, d_out or d_var_out; an output aliasing an input or another output; a camera whose width or
 * height differs from the handle's, or that gdpt_temporal_world_to_sample refuses; tau_z < 0 or non-finite, tau_n outside [-1, 1],
 * s_min outside (0, 1], max_history < 1; non-zero reserved. d_len (nullable): W*H doubles, receives N'. With stats it waits for the
 * stream; with stats == NULL it only enqueues. No CPU fallback. */
int gdpt_temporal_push_device(GdptTemporal *t, const GdptCamera *camera, const double *d_img, const double *d_var, const double *d_feat,
                              const GdptTemporalParams *params /* NULL: defaults */, double *d_out, double *d_var_out,
                              double *d_len /* nullable */, GdptTemporalStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_temporal_push(GdptTemporal *t, const GdptCamera *camera, const double *img, const double *var, const double *feat,
                       const GdptTemporalParams *params /* NULL: defaults */, double *out, double *var_out, double *len /* nullable */,
                       GdptTemporalStats *stats /* nullable */);

/* ---- temporal reprojection of GradPath gradients (not part of the reference) ----
 * A push that carries, beside the primal, the assembled gradients and their variances of the mean through the camera move, so that
 * the accumulated triple (c, cx, cy) with its three variances is what gdpt_reconstruct_device, gdpt_reconstruct_weighted_device and
 * gdpt_denoise_nlm_joint_device take. The difference convention is the project's (gdpt_assemble_device): cx(x, y) estimates
 * I(x, y) - I(x - 1, y) and cy(x, y) estimates I(x, y) - I(x, y - 1). A gradient is not a colour: under a dolly or a rotation a unit
 * pixel step of the new frame is not a unit pixel step of the old one, so the gathered history gradient is transformed by the
 * Jacobian J of the reprojection q(x, y), taken by backward differences along the local tangent plane.
 * Inputs beside those of gdpt_temporal_push: gx, gy (the assembled cx, cy) and gx_var, gy_var (their variances of the mean), W*H*3
 * doubles each, interleaved. Outputs: gx_out, gx_var_out, gy_out, gy_var_out (the same shape) and glen (nullable, W*H doubles, N_g').
 * The handle gains per history set the accumulated gradients and their variances (12 doubles a pixel, interleaved: G_x, G_y, VG_x,
 * VG_y by channel) and a length plane N_g, allocated by the first gradient push. A plain gdpt_temporal_push makes the gradient
 * history STALE (a host flag); so does gdpt_temporal_reset, beside what it does to the primal. Plain pushes keep their kernel.
 * The primal follows the definition above with the same taps t, weights b_t, validity and S, with one addition: a pixel is LEFT OUT
 * also if any of gx_c, gy_c, gx_var_c, gy_var_c at it is non-finite, or a gradient variance is < 0. With every gradient input valid
 * everywhere, out, var_out, len and the GdptTemporalStats fields (except push_ms) are bit for bit gdpt_temporal_push's on the same
 * sequence of frames. Per pixel, with g_k, v_k the inputs (k in {x, y}, channel by channel):
 *   LEFT OUT: the gradient outputs keep the input's bits, N_g' = 0. BACKGROUND, and a SURFACE pixel whose primal RESETS: the input's
 *   bits, N_g' = 1. A SURFACE pixel whose primal BLENDS, with X, n^, d, dir, q, the taps and S of the primal:
 *     G_k = (sum b_t G_prev,k(t)) / S,  VG_k = (sum (b_t b_t) VG_prev,k(t)) / (S S),  N_g = (sum b_t N_g,prev(t)) / S, in the tap order
 *     of the definition above.
 *     The neighbour rays (org, dir_k) are camera rays like dir: dir_x through the sample ((x - 1/2) / W, (y + 1/2) / H), the centre
 *     of the pixel the x-difference reaches back to, dir_y through ((x + 1/2) / W, (y - 1/2) / H); they are defined by the camera
 *     alone, also at x = 0 and y = 0. They are cut with the plane through X with normal n^:
 *     c0 = n^ . dir,  c_k = n^ . dir_k,  t_k = d (c0 / c_k),  X_k = org + t_k dir_k,
 *     (sx_k, sy_k, ., w_k) = M(prev) (X_k, 1),  q_k = (sx_k / w_k W - 1/2, sy_k / w_k H - 1/2),
 *     (Jxx, Jyx) = q - q_x,  (Jxy, Jyy) = q - q_y.
 *     GRADIENT RESET, counted in pixels_gradient_reset: the outputs are the input's bits and N_g' = 1, if the gradient history is
 *     stale, or |c_k| < cos_min for a k, or not c0 / c_k > 0, or not w_k > 0, or an entry of J is non-finite or |entry| > j_max.
 *     Otherwise H_x = Jxx G_x + Jyx G_y,  H_y = Jxy G_x + Jyy G_y,
 *               VH_x = (Jxx Jxx) VG_x + (Jyx Jyx) VG_y,  VH_y = (Jxy Jxy) VG_x + (Jyy Jyy) VG_y (the pair taken as independent, the
 *               convention of every var_out here),
 *               N_g' = min(N_g + 1, max_history),  alpha = 1 / N_g',  out_k = H_k + alpha (g_k - H_k),
 *               var_out_k = ((1 - alpha) (1 - alpha)) VH_k + (alpha alpha) v_k;  where N_g' = 1 the input's bits.
 *   The new gradient history is the four outputs and N_g' of the pixel.
 * Defaults: j_max = 4, cos_min = 0.02. Both are choices, tuned on nothing: j_max bounds how far a history gradient may be stretched
 * before it is dropped, cos_min keeps the division by c_k away from a grazing plane.
 * GdptTemporalGradStats: base as above; pixels_gradient_reset; sum_gradient_history = the sum of N_g' over the film, in fixed order. */
typedef struct GdptTemporalGradParams { double j_max, cos_min; int32_t reserved[4]; } GdptTemporalGradParams;
typedef struct GdptTemporalGradStats  { GdptTemporalStats base; uint64_t pixels_gradient_reset; double sum_gradient_history; } GdptTemporalGradStats;
void gdpt_temporal_default_grad_params(GdptTemporalGradParams *p);   /* 4, 0.02 */
/* Device pointers on the handle's device; enqueued on the handle's stream. Refused before any device call, naming the field: what
 * gdpt_temporal_push_device refuses; a NULL d_gx, d_gy, d_gx_var, d_gy_var, d_gx_out, d_gx_var_out, d_gy_out or d_gy_var_out; an
 * output (d_glen included) aliasing an input or another output; j_max not finite or < 1, cos_min outside (0, 1], a non-zero reserved
 * field of grad_params. With stats it waits for the stream; with stats == NULL it only enqueues. No CPU fallback. */
int gdpt_temporal_push_gradients_device(GdptTemporal *t, const GdptCamera *camera, const double *d_img, const double *d_var,
                                        const double *d_feat, const double *d_gx, const double *d_gx_var, const double *d_gy,
                                        const double *d_gy_var, const GdptTemporalParams *params /* NULL: defaults */,
                                        const GdptTemporalGradParams *grad_params /* NULL: defaults */, double *d_out, double *d_var_out,
                                        double *d_len /* nullable */, double *d_gx_out, double *d_gx_var_out, double *d_gy_out,
                                        double *d_gy_var_out, double *d_glen /* nullable */,
                                        GdptTemporalGradStats *stats /* nullable: enqueue-only */);
/* Host pointers. Blocking. */
int gdpt_temporal_push_gradients(GdptTemporal *t, const GdptCamera *camera, const double *img, const double *var, const double *feat,
                                 const double *gx, const double *gx_var, const double *gy, const double *gy_var,
                                 const GdptTemporalParams *params /* NULL: defaults */,
                                 const GdptTemporalGradParams *grad_params /* NULL: defaults */, double *out, double *var_out,
                                 double *len /* nullable */, double *gx_out, double *gx_var_out, double *gy_out, double *gy_var_out,
                                 double *glen /* nullable */, GdptTemporalGradStats *stats /* nullable */);

/* ---- output ---- */
/* By suffix: ".pfm" (fp32, header "PF\nW H\n-1\n", rows as stored) or ".exr" (fp16 RGB scanline). */
int gdpt_imwrite(const char *filename, int width, int height, const double *rgb);

/* ---- input images (host only) ----
 * imread1 / imread3 of the reference (src/image.cpp:26-133) for channels = 1 / 3: fp64 texels, row-major, top row
 * first. ".jpg"/".jpeg": own baseline decoder returning stb_image's samples, widened like stbi_loadf; ".pfm"; other
 * suffixes through a pre-decoded "<file>.gdtex" companion. Free with gdpt_image_free. */
int gdpt_imread(const char *filename, int channels, int *width, int *height, double **texels);
void gdpt_image_free(double *texels);

/* ---- diagnostics (host only, no GPU) ----
 * Builds the acceleration structure that gdpt_scene_upload would build over `n` primitive boxes (bounds6 = n x
 * {min xyz, max xyz}, fp32) — the replacement for the reference's Embree commit, src/scene.cpp:20-31 — and verifies it:
 * every primitive sits in exactly one leaf, every child box encloses the boxes below it, in the BVH2 and in the
 * collapsed wide forms (4-wide fp32 boxes; 8-wide boxes quantised on a per-node grid, whose exactly evaluated grid
 * boxes must enclose their subtrees and whose stack bound must hold). stats: [0] BVH2 nodes, [1] BVH2 depth, [2] BVH4
 * nodes, [3] BVH4 node arity used (2..4), [4] traversal-stack bound of the BVH4, [5] leaves, [6] max primitives per
 * leaf, [7] BVH8 nodes. */
int gdpt_bvh_check(const float *bounds6, int n, int32_t stats[8]);
/* The same for the build with spatial splits (host/sbvh.cpp; what gdpt_scene_upload uses for meshes walked from HBM): over `n`
 * fp32 triangles (tri_verts9 = n x 3 vertices x xyz) with `budget` extra references per primitive allowed. Verifies that child
 * boxes enclose the reference boxes below them, that every triangle is referenced, the depth and stack bounds of the collapsed
 * form, and COVERAGE: for `samples_per_tri` points on every triangle (its vertices, edge midpoints, centroid, then points from a
 * fixed lattice), descending from the root through every child box that contains the point reaches a leaf that references the
 * triangle — a ray that hits the triangle there cannot miss it in the tree. stats: [0] BVH2 nodes, [1] BVH2 depth, [2] references
 * (>= n), [3] BVH4 nodes, [4] BVH4 stack bound, [5] leaves, [6] / [7] 1000 x the surface-area cost of the BVH4: inner nodes entered /
 * triangles tested per random line through the root box. */
int gdpt_sbvh_check(const float *tri_verts9, int n, double budget, int samples_per_tri, int32_t stats[8]);

const char *gdpt_last_error(void);
/* "gfx950" etc. of the device the library's kernels were built for, and the running device name. */
const char *gdpt_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* GDPT_H */
