// debug_kat.hip — test instrument (include/gdpt_debug.h: gdpt_debug_kat_*): the per-vertex device functions of the render kernels
// run on arrays of cases, one thread per case, so that a test can compare each of them with a known answer. The kernels include the
// product headers and call their functions as they are; no LDS scene, no traversal (the walks have a family of their own,
// debug_kat_trace.hip). Nothing in lajolla, in bench.py's timed region or in the library calls these entry points.
#include "../../../include/gdpt_debug.h"
#include "../capi_common.h"
#include "render_path.h"
#include "render_phases_general_sets.h"
#include "render_twosided.h"
#include "scene_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

using gdpt::ck;
constexpr int kKatBlock = 256;
constexpr int kKatMaxCases = 1 << 22;
constexpr int kKatEnvmapMaxCases = 1 << 20;

__device__ __forceinline__ gd::D3 ld3(const double *p) { return gd::mk(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(double *p, gd::D3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

__device__ __forceinline__ gd::Vertex kat_vertex(const GdptKatVertex &q, int material_id) {
    gd::Vertex v;
    v.position = gd::splat(0.0);
    v.gn = ld3(q.gn);
    v.frame.x = ld3(q.fx); v.frame.y = ld3(q.fy); v.frame.n = ld3(q.fn);
    v.uv.x = q.uv[0]; v.uv.y = q.uv[1];
    v.uv_screen_size = q.uv_screen_size;
    v.material_id = material_id; v.light_id = -1;
    return v;
}

// ---- bsdf: the dispatch of device_bsdf.h under one <ROUGH, TWOSIDED, MASK> triple ----------------------------------
template <bool ROUGH, bool TWOSIDED, unsigned MASK>
__global__ void __launch_bounds__(kKatBlock) kat_bsdf_kernel(DevSceneView sv, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatBsdfQuery q = in[i];
        GdptKatBsdfResult r;
        memset(&r, 0, sizeof(r));
        const gd::Vertex v = kat_vertex(q.vertex, q.material_id);
        const GdptMaterial &m = sv.materials[q.material_id];
        const gd::D3 din = ld3(q.dir_in);
        gd::D2 ruv; ruv.x = q.ruv[0]; ruv.y = q.ruv[1];
        gd::BsdfSample s;
        s.dir_out = gd::splat(0.0); s.eta = 0; s.roughness = 0;
        r.sample_valid = gd::bsdf_sample<ROUGH, TWOSIDED, MASK>(sv, m, din, v, ruv, q.rw, s) ? 1 : 0;
        if (r.sample_valid) { st3(r.s_dir, s.dir_out); r.s_eta = s.eta; r.s_rough = s.roughness; }
#pragma nounroll
        for (int k = r.sample_valid ? 0 : 1; k < 2; k++) {      // k = 0: the sampled direction, k = 1: dir_out2
            const gd::D3 dout = k == 0 ? s.dir_out : ld3(q.dir_out2);
            const gd::D3 f = gd::bsdf_eval<ROUGH, TWOSIDED, MASK>(sv, m, din, dout, v);
            const double p = gd::bsdf_pdf<ROUGH, TWOSIDED, MASK>(sv, m, din, dout, v);
            gd::D3 ff; double fp;
            gd::bsdf_eval_pdf<ROUGH, TWOSIDED, MASK>(sv, m, din, dout, v, ff, fp);
            st3(r.f[k], f); r.pdf[k] = p; st3(r.fused_f[k], ff); r.fused_pdf[k] = fp;
        }
        out[i] = r;
    }
}

// ---- bsdf, the inline Lambertian of render_device.h: mat_sample / mat_eval_pdf / mat_pdf with LAMBERT = true ----------
// (that path reads TraceCtx::materials alone; it has no separate eval, so f[] is left NaN)
template <int PLAIN>
__global__ void __launch_bounds__(kKatBlock) kat_lambert_kernel(DevSceneView sv, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatBsdfQuery q = in[i];
        GdptKatBsdfResult r;
        memset(&r, 0, sizeof(r));
        const gd::Vertex v = kat_vertex(q.vertex, q.material_id);
        gd::TraceCtx tx;
        memset(&tx, 0, sizeof(tx));
        tx.materials = sv.materials;
        const gd::D3 din = ld3(q.dir_in);
        gd::D2 ruv; ruv.x = q.ruv[0]; ruv.y = q.ruv[1];
        gd::BsdfSample s;
        s.dir_out = gd::splat(0.0); s.eta = 0; s.roughness = 0;
        r.sample_valid = gd::mat_sample<true>(sv, tx, v, din, ruv, q.rw, s) ? 1 : 0;
        if (r.sample_valid) { st3(r.s_dir, s.dir_out); r.s_eta = s.eta; r.s_rough = s.roughness; }
        const double nan = __builtin_nan("");
#pragma nounroll
        for (int k = r.sample_valid ? 0 : 1; k < 2; k++) {
            const gd::D3 dout = k == 0 ? s.dir_out : ld3(q.dir_out2);
            gd::D3 ff; double fp;
            gd::mat_eval_pdf<true, false, false, gd::kAllMaterials, PLAIN>(sv, tx, v, din, dout, ff, fp);
            st3(r.f[k], gd::splat(nan)); r.pdf[k] = gd::mat_pdf<true>(sv, tx, v, din, dout);
            st3(r.fused_f[k], ff); r.fused_pdf[k] = fp;
        }
        out[i] = r;
    }
}

__global__ void __launch_bounds__(kKatBlock) kat_texture_kernel(DevSceneView sv, int n, const GdptKatTextureQuery *in, GdptKatTextureResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatTextureQuery q = in[i];
        GdptKatVertex kv;
        memset(&kv, 0, sizeof(kv));
        kv.uv[0] = q.uv[0]; kv.uv[1] = q.uv[1]; kv.uv_screen_size = q.uv_screen_size;
        const gd::Vertex v = kat_vertex(kv, q.material_id);
        const GdptTexture &t = sv.materials[q.material_id].tex[q.slot];
        GdptKatTextureResult r;
        st3(r.tex3, gd::tex3(sv, t, v));
        r.tex1 = gd::tex1(sv, t, v);
        out[i] = r;
    }
}

__global__ void __launch_bounds__(kKatBlock) kat_filter_kernel(int n, const GdptKatFilterQuery *in, GdptKatFilterResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatFilterQuery q = in[i];
        const gd::D2 o = gd::filter_sample(q.type, q.param, q.u[0], q.u[1]);
        out[i].out[0] = o.x; out[i].out[1] = o.y;
    }
}

template <bool PIXEL_SPACE>
__global__ void __launch_bounds__(kKatBlock) kat_primary_kernel(DevSceneView sv, int n, const GdptKatPrimaryQuery *in, GdptKatPrimaryResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatPrimaryQuery q = in[i];
        const gd::Ray r = gd::sample_primary<PIXEL_SPACE>(sv.cam, q.s[0], q.s[1]);
        st3(out[i].org, r.org); st3(out[i].dir, r.dir);
    }
}

__global__ void __launch_bounds__(kKatBlock) kat_shading_kernel(DevSceneView sv, int n, const GdptKatShadingQuery *in, GdptKatShadingResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatShadingQuery q = in[i];
        gd::D2 st; st.x = q.st[0]; st.y = q.st[1];
        gd::D2 uv; gd::Frame fr; double inv_uv_size;
        if (q.is_sphere) gd::shading_info_sphere(sv.spheres[q.index], st, ld3(q.gn), uv, fr, inv_uv_size);
        else gd::shading_info_tri(sv.tris[q.index], st, ld3(q.gn), q.need_uv != 0, uv, fr, inv_uv_size);
        GdptKatShadingResult r;
        r.uv[0] = uv.x; r.uv[1] = uv.y;
        st3(r.fx, fr.x); st3(r.fy, fr.y); st3(r.fn, fr.n);
        r.inv_uv_size = inv_uv_size;
        out[i] = r;
    }
}

__global__ void __launch_bounds__(kKatBlock) kat_light_kernel(DevSceneView sv, int n, const GdptKatLightQuery *in, GdptKatLightResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatLightQuery q = in[i];
        const DevLight &lt = sv.lights[q.light_id];
        gd::D2 uv; uv.x = q.uv[0]; uv.y = q.uv[1];
        const gd::PointNormal pn = gd::sample_point_on_light(sv, lt, ld3(q.ref), uv, q.w);
        GdptKatLightResult r;
        st3(r.position, pn.position); st3(r.normal, pn.normal);
        r.pdf = gd::pdf_point_on_light(sv, lt, pn, ld3(q.ref));
        out[i] = r;
    }
}

// ---- envmap: the environment-map code of render_path.h on the scene's own map (next-event estimation forms the pdf and the emission of
// a sampled direction from its negative; the miss branches call envmap_emission(-ray.dir) and envmap_pdf(-dir_bsdf)) ----------------------
__global__ void __launch_bounds__(kKatBlock) kat_envmap_kernel(DevSceneView sv, int n, const GdptKatEnvmapQuery *in, GdptKatEnvmapResult *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const GdptKatEnvmapQuery q = in[i];
        gd::D2 rnd; rnd.x = q.rnd[0]; rnd.y = q.rnd[1];
        const gd::D3 dir = ld3(q.dir);
        GdptKatEnvmapResult r;
        const gd::D2 suv = gd::table2d_sample(sv, rnd);
        r.sample_uv[0] = suv.x; r.sample_uv[1] = suv.y;
        const gd::D3 sdir = gd::envmap_sample_dir(sv, rnd);
        st3(r.sample_dir, sdir);
        r.sample_pdf = gd::envmap_pdf(sv, -sdir);
        st3(r.sample_emission, gd::envmap_emission(sv, -sdir));
        const gd::D2 duv = gd::envmap_uv(gd::xform_vector16(sv.env_to_local, dir));
        r.dir_uv[0] = duv.x; r.dir_uv[1] = duv.y;
        r.dir_pdf = gd::envmap_pdf(sv, -dir);
        st3(r.dir_emission, gd::envmap_emission(sv, -dir));
        out[i] = r;
    }
}

// ---- the tables of variants: one row each; the rows give the variants their names and, for bsdf, the triple to Python ----------
dim3 kat_grid(int n) { return dim3((unsigned)((n + kKatBlock - 1) / kKatBlock)); }

typedef void (*BsdfLaunch)(const DevSceneView &, int, const GdptKatBsdfQuery *, GdptKatBsdfResult *, hipStream_t);
template <bool ROUGH, bool TWOSIDED, unsigned MASK>
void launch_bsdf(const DevSceneView &sv, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out, hipStream_t stream) {
    hipLaunchKernelGGL((kat_bsdf_kernel<ROUGH, TWOSIDED, MASK>), kat_grid(n), dim3(kKatBlock), 0, stream, sv, n, in, out);
}
template <int PLAIN>
void launch_lambert(const DevSceneView &sv, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out, hipStream_t stream) {
    hipLaunchKernelGGL((kat_lambert_kernel<PLAIN>), kat_grid(n), dim3(kKatBlock), 0, stream, sv, n, in, out);
}
struct BsdfVariant { GdptKatVariant row; BsdfLaunch launch; };
#define KAT_TRIPLE(name, ROUGH, TWOSIDED, MASK) {{name, MASK, ROUGH, TWOSIDED, 0, 0}, launch_bsdf<ROUGH, TWOSIDED, MASK>}
#define KAT_INLINE(name, PLAIN) {{name, 1u << GDPT_MAT_LAMBERTIAN, 0, 0, 1, PLAIN}, launch_lambert<PLAIN>}
const BsdfVariant kBsdfVariants[] = {
    KAT_TRIPLE("full", true, true, gd::kAllMaterials),                        // render_path.h, render_reconnect.h, the straight loops
    KAT_TRIPLE("one_sided", false, false, gd::kAllMaterials),                 // render_device.h: lane_consume, every one-sided lobe
    KAT_TRIPLE("set_disney_diffuse", false, false, gdpt::kSetDisneyDiffuse),  // render_phases_general_sets_a.hip
    KAT_TRIPLE("set_disney_metal", false, false, gdpt::kSetDisneyMetal),
    KAT_TRIPLE("set_disney_clearcoat", false, false, gdpt::kSetDisneyClearcoat),   // render_phases_general_sets_b.hip
    KAT_TRIPLE("set_disney_sheen", false, false, gdpt::kSetDisneySheen),
    KAT_TRIPLE("two_sided", false, true, gd::kAllMaterials),                  // render_twosided.h, base path and replay of offsets
    KAT_TRIPLE("two_sided_glass", false, true, gd::kSetGlass),
    KAT_INLINE("lambert_inline", 0),
    KAT_INLINE("lambert_inline_const_tex", gd::kPlainConstTex),
};
#undef KAT_TRIPLE
#undef KAT_INLINE

const GdptKatVariant kOneVariant[] = {{"product", 0, 0, 0, 0, 0}};
const GdptKatVariant kPrimaryVariants[] = {{"screen", 0, 0, 0, 0, 0}, {"pixel_space", 0, 0, 0, 0, 0}};

int family_variants(const std::string &family, std::vector<GdptKatVariant> &rows) {
    rows.clear();
    if (family == "bsdf") { for (const BsdfVariant &b : kBsdfVariants) rows.push_back(b.row); return 0; }
    if (family == "primary") { rows.assign(kPrimaryVariants, kPrimaryVariants + 2); return 0; }
    if (family == "texture" || family == "filter" || family == "shading" || family == "light" || family == "envmap") { rows.assign(kOneVariant, kOneVariant + 1); return 0; }
    if (family == "trace") {       // (the table itself: debug_kat_trace.hip)
        std::vector<GdptKatTraceVariant> t((size_t)std::max(0, gdpt_debug_kat_trace_variants(nullptr, 0)));
        if (gdpt_debug_kat_trace_variants(t.data(), (int)t.size()) != (int)t.size()) return 1;
        for (const GdptKatTraceVariant &r : t) rows.push_back(GdptKatVariant{r.name, 0, 0, 0, 0, 0});
        return 0;
    }
    return 1;
}

// ---- host side of an entry: argument checks, then copy in, launch on the scene's stream, copy out, wait --------------------------
void check_common(const std::string &who, const GdptScene *scene, const char *family, int variant, int n, const void *in, const void *out) {
    if (!scene) throw std::runtime_error(who + ": null scene handle");
    if (n < 0 || n > kKatMaxCases) throw std::runtime_error(who + ": n must be in [0, " + std::to_string(kKatMaxCases) + "]");
    if (n > 0 && (!in || !out)) throw std::runtime_error(who + ": null query or result array");
    std::vector<GdptKatVariant> rows;
    family_variants(family, rows);
    if (variant < 0 || variant >= (int)rows.size()) throw std::runtime_error(who + ": variant " + std::to_string(variant) + " is not in the table of " + std::to_string(rows.size()) + " variants");
}
void check_index(const std::string &who, int i, const char *what, int value, int size) {
    if (value < 0 || value >= size) throw std::runtime_error(who + ": case " + std::to_string(i) + ": " + what + " " + std::to_string(value) + " is outside the uploaded scene's table of " + std::to_string(size));
}

template <class Q, class R, class LAUNCH>
void run_cases(const GdptScene *scene, int n, const Q *in, R *out, LAUNCH &&launch) {
    if (n == 0) return;
    ck(hipSetDevice(scene->device), "hipSetDevice");
    const hipStream_t stream = scene->render_stream[0];
    gdpt::DeviceBuffer<Q> d_in;
    gdpt::DeviceBuffer<R> d_out;
    d_in.alloc((size_t)n, "hipMalloc(kat queries)");
    d_out.alloc((size_t)n, "hipMalloc(kat results)");
    ck(hipMemcpyAsync(d_in, in, (size_t)n * sizeof(Q), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(kat queries)");
    launch(scene->view, n, (const Q *)d_in, (R *)d_out, stream);
    ck(hipGetLastError(), "kat kernel launch");
    ck(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(R), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(kat results)");
    ck(hipStreamSynchronize(stream), "hipStreamSynchronize(kat)");
}

// the uploaded material table, read back: which lobe a material is and which of its textures are constant
std::vector<GdptMaterial> read_materials(const GdptScene *scene) {
    std::vector<GdptMaterial> m((size_t)scene->view.num_materials);
    if (m.empty()) return m;
    ck(hipSetDevice(scene->device), "hipSetDevice");
    ck(hipMemcpy(m.data(), scene->view.materials, m.size() * sizeof(GdptMaterial), hipMemcpyDeviceToHost), "hipMemcpy(materials)");
    return m;
}

} // namespace

extern "C" {

int gdpt_debug_kat_variants(const char *family, GdptKatVariant *out, int capacity) {
    int count = -1;
    const int rc = gdpt::guarded([&]() {
        if (!family) throw std::runtime_error("gdpt_debug_kat_variants: null family");
        std::vector<GdptKatVariant> rows;
        if (family_variants(family, rows)) throw std::runtime_error(std::string("gdpt_debug_kat_variants: unknown family '") + family + "' (bsdf, texture, filter, primary, shading, light, envmap, trace)");
        if (out) {
            if (capacity < (int)rows.size()) throw std::runtime_error("gdpt_debug_kat_variants: capacity too small");
            for (size_t i = 0; i < rows.size(); i++) out[i] = rows[i];
        }
        count = (int)rows.size();
    });
    return rc ? -1 : count;
}

int gdpt_debug_kat_bsdf(const GdptScene *scene, int variant, int n, const GdptKatBsdfQuery *in, GdptKatBsdfResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_bsdf";
        check_common(who, scene, "bsdf", variant, n, in, out);
        const BsdfVariant &bv = kBsdfVariants[variant];
        const std::vector<GdptMaterial> mats = n > 0 ? read_materials(scene) : std::vector<GdptMaterial>();
        for (int i = 0; i < n; i++) {
            check_index(who, i, "material id", in[i].material_id, scene->view.num_materials);
            if (!bv.row.inline_lambert) continue;
            const GdptMaterial &m = mats[(size_t)in[i].material_id];
            if (m.type != GDPT_MAT_LAMBERTIAN) throw std::runtime_error(who + ": case " + std::to_string(i) + ": variant '" + bv.row.name + "' takes Lambertian materials only");
            if ((bv.row.plain & gd::kPlainConstTex) && m.tex[0].type != GDPT_TEX_CONSTANT)
                throw std::runtime_error(who + ": case " + std::to_string(i) + ": variant '" + bv.row.name + "' takes constant reflectances only");
        }
        run_cases(scene, n, in, out, bv.launch);
    });
}

int gdpt_debug_kat_texture(const GdptScene *scene, int variant, int n, const GdptKatTextureQuery *in, GdptKatTextureResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_texture";
        check_common(who, scene, "texture", variant, n, in, out);
        const std::vector<GdptMaterial> mats = n > 0 ? read_materials(scene) : std::vector<GdptMaterial>();
        for (int i = 0; i < n; i++) {
            check_index(who, i, "material id", in[i].material_id, scene->view.num_materials);
            check_index(who, i, "texture slot", in[i].slot, GDPT_MAT_MAX_TEX);
            const GdptTexture &t = mats[(size_t)in[i].material_id].tex[in[i].slot];
            if (t.type == GDPT_TEX_IMAGE) check_index(who, i, "image id", t.image_id, scene->view.num_images);
        }
        run_cases(scene, n, in, out, [](const DevSceneView &sv, int m, const GdptKatTextureQuery *q, GdptKatTextureResult *r, hipStream_t s) {
            hipLaunchKernelGGL(kat_texture_kernel, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
        });
    });
}

int gdpt_debug_kat_filter(const GdptScene *scene, int variant, int n, const GdptKatFilterQuery *in, GdptKatFilterResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_filter";
        check_common(who, scene, "filter", variant, n, in, out);
        for (int i = 0; i < n; i++) check_index(who, i, "filter type", in[i].type, GDPT_FILTER_GAUSSIAN + 1);
        run_cases(scene, n, in, out, [](const DevSceneView &, int m, const GdptKatFilterQuery *q, GdptKatFilterResult *r, hipStream_t s) {
            hipLaunchKernelGGL(kat_filter_kernel, kat_grid(m), dim3(kKatBlock), 0, s, m, q, r);
        });
    });
}

int gdpt_debug_kat_primary(const GdptScene *scene, int variant, int n, const GdptKatPrimaryQuery *in, GdptKatPrimaryResult *out) {
    return gdpt::guarded([&]() {
        check_common("gdpt_debug_kat_primary", scene, "primary", variant, n, in, out);
        run_cases(scene, n, in, out, [variant](const DevSceneView &sv, int m, const GdptKatPrimaryQuery *q, GdptKatPrimaryResult *r, hipStream_t s) {
            if (variant == 0) hipLaunchKernelGGL(kat_primary_kernel<false>, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
            else hipLaunchKernelGGL(kat_primary_kernel<true>, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
        });
    });
}

int gdpt_debug_kat_shading(const GdptScene *scene, int variant, int n, const GdptKatShadingQuery *in, GdptKatShadingResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_shading";
        check_common(who, scene, "shading", variant, n, in, out);
        for (int i = 0; i < n; i++) {
            if (in[i].is_sphere) check_index(who, i, "sphere index", in[i].index, scene->view.num_spheres);
            else check_index(who, i, "triangle id", in[i].index, scene->view.num_tris);
        }
        run_cases(scene, n, in, out, [](const DevSceneView &sv, int m, const GdptKatShadingQuery *q, GdptKatShadingResult *r, hipStream_t s) {
            hipLaunchKernelGGL(kat_shading_kernel, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
        });
    });
}

int gdpt_debug_kat_light(const GdptScene *scene, int variant, int n, const GdptKatLightQuery *in, GdptKatLightResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_light";
        check_common(who, scene, "light", variant, n, in, out);
        for (int i = 0; i < n; i++) {
            check_index(who, i, "light id", in[i].light_id, scene->view.num_lights);
            if (scene->view.has_envmap && in[i].light_id == scene->view.env_light_id) throw std::runtime_error(who + ": case " + std::to_string(i) + ": the environment map is no area emitter");
        }
        run_cases(scene, n, in, out, [](const DevSceneView &sv, int m, const GdptKatLightQuery *q, GdptKatLightResult *r, hipStream_t s) {
            hipLaunchKernelGGL(kat_light_kernel, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
        });
    });
}

int gdpt_debug_kat_envmap(const GdptScene *scene, int variant, int n, const GdptKatEnvmapQuery *in, GdptKatEnvmapResult *out) {
    return gdpt::guarded([&]() {
        const std::string who = "gdpt_debug_kat_envmap";
        check_common(who, scene, "envmap", variant, n, in, out);
        if (n > kKatEnvmapMaxCases) throw std::runtime_error(who + ": n must be in [0, " + std::to_string(kKatEnvmapMaxCases) + "]");
        const DevSceneView &v = scene->view;
        if (!v.has_envmap || v.env_w < 1 || v.env_h < 1 || v.env_image_id < 0 || v.env_image_id >= v.num_images)
            throw std::runtime_error(who + ": the scene has no environment map");
        for (int i = 0; i < n; i++) {
            const GdptKatEnvmapQuery &q = in[i];
            for (double x : {q.rnd[0], q.rnd[1], q.dir[0], q.dir[1], q.dir[2]})
                if (!std::isfinite(x)) throw std::runtime_error(who + ": case " + std::to_string(i) + ": a number that is not finite");
            for (double x : q.rnd)
                if (x < 0 || x > 1) throw std::runtime_error(who + ": case " + std::to_string(i) + ": a random number outside [0, 1]");
            if (q.dir[0] == 0 && q.dir[1] == 0 && q.dir[2] == 0) throw std::runtime_error(who + ": case " + std::to_string(i) + ": dir is zero");
            for (int k = 0; k < 3; k++)        // the local direction (xform_vector16): a NaN there would index the tables
                if (!std::isfinite(v.env_to_local[4 * k] * q.dir[0] + v.env_to_local[4 * k + 1] * q.dir[1] + v.env_to_local[4 * k + 2] * q.dir[2]))
                    throw std::runtime_error(who + ": case " + std::to_string(i) + ": a number that is not finite in the map's frame");
        }
        run_cases(scene, n, in, out, [](const DevSceneView &sv, int m, const GdptKatEnvmapQuery *q, GdptKatEnvmapResult *r, hipStream_t s) {
            hipLaunchKernelGGL(kat_envmap_kernel, kat_grid(m), dim3(kKatBlock), 0, s, sv, m, q, r);
        });
    });
}

} // extern "C"
