// scene_prepare.cpp — see scene_prepare.h. Replaces Scene::Scene (src/scene.cpp:4-53) up to the point where the tables go to a device.
#include "scene_prepare.h"
#include "bvh.h"
#include "tri_precompute.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace gdpt {
namespace {

constexpr double kSbvhBudget = 1.0;       // extra references / primitives the spatial-split build may add (it adds ~0.1-0.35; knob sbvh overrides)
constexpr double kPresplitBudget = 0.0;   // extra references / primitives (knob presplit overrides)

// The primitives in input order (gid order, spheres last), as the tree builders take them.
struct Flat {
    std::vector<DevPrim> prim_in;
    std::vector<PrimBounds> bounds;
    std::vector<float> tri_verts;          // the fp32 triangles the intersection test sees (9 floats each), for presplit
    float lb[3], ub[3];                    // fp32 scene bounds
};

void table_1d(const std::vector<double> &f, std::vector<double> &pmf, std::vector<double> &cdf) {   // src/table_dist.cpp:3-25
    pmf = f;
    cdf.assign(f.size() + 1, 0.0);
    for (size_t i = 0; i < f.size(); i++) cdf[i + 1] = cdf[i] + pmf[i];
    const double total = cdf.back();
    if (total > 0) { for (size_t i = 0; i < pmf.size(); i++) { pmf[i] /= total; cdf[i] /= total; } }
    else {
        for (size_t i = 0; i < pmf.size(); i++) { pmf[i] = 1.0 / (double)pmf.size(); cdf[i] = (double)i / (double)pmf.size(); }
        cdf.back() = 1;
    }
}

void check_description(const GdptSceneDesc *desc) {
    const GdptCamera &cam = desc->camera;
    if (cam.width <= 0 || cam.height <= 0) throw std::runtime_error("gdpt_scene_upload: empty film");
    for (int m = 0; m < desc->num_materials; m++) {
        int t = desc->materials[m].type;
        if (t < 0 || t > GDPT_MAT_DISNEY_BSDF) throw std::runtime_error("gdpt_scene_upload: unknown material type");
        for (int k = 0; k < GDPT_MAT_MAX_TEX; k++) {
            const GdptTexture &tx = desc->materials[m].tex[k];
            if (tx.type == GDPT_TEX_IMAGE && (tx.image_id < 0 || tx.image_id >= desc->num_images))
                throw std::runtime_error("gdpt_scene_upload: texture references a missing image");
        }
    }
}

// ---- flatten primitives: triangles in (shape, triangle) order = global id; spheres after them ----
Flat flatten(const GdptSceneDesc *desc, PreparedScene *ps) {
    Flat f;
    std::vector<DevTriShade> &tris = ps->tris;
    std::vector<DevSphere> &spheres = ps->spheres;
    std::vector<DevPrim> &prim_in = f.prim_in;
    std::vector<PrimBounds> &bounds = f.bounds;
    std::vector<float> &tri_verts = f.tri_verts;
    float *lb = f.lb, *ub = f.ub;
    for (int k = 0; k < 3; k++) { lb[k] = std::numeric_limits<float>::infinity(); ub[k] = -lb[k]; }
    for (int s = 0; s < desc->num_shapes; s++) {
        const GdptShape &sh = desc->shapes[s];
        if (sh.material_id < 0 || sh.material_id >= desc->num_materials) throw std::runtime_error("gdpt_scene_upload: shape without a valid material");
        if (sh.area_light_id >= desc->num_lights) throw std::runtime_error("gdpt_scene_upload: bad area light id");
        if (sh.type != GDPT_SHAPE_TRIMESH) continue;
        if (!sh.positions || !sh.indices) throw std::runtime_error("gdpt_scene_upload: mesh without positions/indices");
        for (int i = 0; i < sh.num_vertices; i++)
            for (int k = 0; k < 3; k++) { float p = (float)sh.positions[3 * i + k]; lb[k] = std::min(lb[k], p); ub[k] = std::max(ub[k], p); }
        for (int t = 0; t < sh.num_triangles; t++) {
            DevTriShade ts{};
            DevPrim pr{};
            PrimBounds pb;
            float v[3][3];
            double pos64[3][3];
            for (int k = 0; k < 3; k++) { pb.bmin[k] = std::numeric_limits<float>::infinity(); pb.bmax[k] = -pb.bmin[k]; }
            for (int i = 0; i < 3; i++) {
                int vi = sh.indices[3 * t + i];
                if (vi < 0 || vi >= sh.num_vertices) throw std::runtime_error("gdpt_scene_upload: mesh index out of range");
                for (int k = 0; k < 3; k++) {
                    pos64[i][k] = sh.positions[3 * vi + k];
                    v[i][k] = (float)sh.positions[3 * vi + k];
                    pb.bmin[k] = std::min(pb.bmin[k], v[i][k]); pb.bmax[k] = std::max(pb.bmax[k], v[i][k]);
                    if (sh.normals) ts.n[i][k] = sh.normals[3 * vi + k];
                }
                if (sh.uvs) { ts.uv[i][0] = sh.uvs[2 * vi]; ts.uv[i][1] = sh.uvs[2 * vi + 1]; }
            }
            if (!sh.uvs) { // src/shapes/triangle_mesh.inl:86-90
                ts.uv[0][0] = 0; ts.uv[0][1] = 0; ts.uv[1][0] = 1; ts.uv[1][1] = 0; ts.uv[2][0] = 1; ts.uv[2][1] = 1;
            }
            ts.shape_id = s; ts.prim_id = t; ts.material_id = sh.material_id; ts.light_id = sh.area_light_id;
            ts.has_normals = sh.normals != nullptr; ts.has_uvs = sh.uvs != nullptr;
            for (int k = 0; k < 3; k++) { pr.v0[k] = v[0][k]; pr.e1[k] = v[1][k] - v[0][k]; pr.e2[k] = v[2][k] - v[0][k]; }
            for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) tri_verts.push_back(v[i][k]);
            precompute_tri_constants(pos64, pr.e1, pr.e2, &ts);
            pr.gid = (uint32_t)tris.size();
            tris.push_back(ts); prim_in.push_back(pr); bounds.push_back(pb);
        }
    }
    if (tris.size() >= (size_t)GDPT_SPHERE_FLAG / 8) throw std::runtime_error("gdpt_scene_upload: too many triangles");
    for (int s = 0; s < desc->num_shapes; s++) {
        const GdptShape &sh = desc->shapes[s];
        if (sh.type != GDPT_SHAPE_SPHERE) continue;
        DevSphere sp{};
        DevPrim pr{};
        PrimBounds pb;
        for (int k = 0; k < 3; k++) {
            sp.center[k] = sh.center[k];
            // scene bounds as Embree sees them: sphere_bounds_func stores double -> float (src/shapes/sphere.inl:1-10)
            lb[k] = std::min(lb[k], (float)(sh.center[k] - sh.radius)); ub[k] = std::max(ub[k], (float)(sh.center[k] + sh.radius));
            // BVH bounds: rounded outward so the box always contains the fp64 sphere
            pb.bmin[k] = std::nextafterf((float)(sh.center[k] - sh.radius), -std::numeric_limits<float>::infinity());
            pb.bmax[k] = std::nextafterf((float)(sh.center[k] + sh.radius), std::numeric_limits<float>::infinity());
        }
        sp.radius = sh.radius; sp.shape_id = s; sp.material_id = sh.material_id; sp.light_id = sh.area_light_id;
        pr.gid = GDPT_SPHERE_FLAG | (uint32_t)spheres.size();
        spheres.push_back(sp); prim_in.push_back(pr); bounds.push_back(pb);
    }
    return f;
}

// ---- the trees: BVH2 (presplit or spatial splits), padded, and its wide forms; the primitive records in leaf order ----
void build_tree(const GdptCamera &cam, const Flat &f, const PrepareOptions &opt, PreparedScene *ps) {
    const std::vector<DevTriShade> &tris = ps->tris;
    const std::vector<DevSphere> &spheres = ps->spheres;
    const std::vector<PrimBounds> &bounds = f.bounds;
    const std::vector<float> &tri_verts = f.tri_verts;
    const float *lb = f.lb, *ub = f.ub;
    SceneTraits &tr = ps->traits;
    // large triangles of big meshes are referenced from several smaller boxes (host/presplit.cpp); scenes small enough
    // for LDS keep one reference per primitive
    std::vector<PrimBounds> refs;
    std::vector<uint32_t> ref_prim;
    {
        const double budget = opt.presplit >= 0 ? opt.presplit : tris.size() >= 4096 ? kPresplitBudget : 0.0;
        presplit_triangles(bounds, tri_verts, budget, &refs, &ref_prim);
    }
    // spatial splits inside the SAH build (host/sbvh.cpp) for meshes that are walked from HBM; `sbvh` = extra references allowed
    // per primitive (test knob; 0 = the plain object-split build)
    const double sbvh_budget = opt.sbvh >= 0 ? opt.sbvh : tris.size() >= 4096 ? kSbvhBudget : 0.0;
    BvhBuildResult bvh = sbvh_budget > 0 ? build_sbvh(bounds, tri_verts, sbvh_budget, &ref_prim) : build_bvh(refs);
    {   // widen every child box: the traversal's slab test then needs no per-test padding (device_trace.h: box_hit)
        float ext = 0.f;
        for (int k = 0; k < 3; k++) if (ub[k] >= lb[k]) ext = std::max(ext, std::max(std::fabs(ub[k]), std::fabs(lb[k])));
        for (auto &sp : spheres) for (int k = 0; k < 3; k++) ext = std::max(ext, (float)(std::fabs(sp.center[k]) + sp.radius));
        // ray origins: surface points (inside the bounds) and the camera position, xform_point(cam_to_world, 0)
        ext = std::max(ext, camera_extent(cam));
        tr.pad_extent = ext;
        const float pad = ext * 1e-6f + 1e-30f;
        for (auto &n : bvh.nodes)
            for (int k = 0; k < 3; k++) {
                if (n.lmin[k] <= n.lmax[k]) { n.lmin[k] -= pad; n.lmax[k] += pad; }
                if (n.rmin[k] <= n.rmax[k]) { n.rmin[k] -= pad; n.rmax[k] += pad; }
            }
    }
    // wide form for scenes walked from HBM (same padded boxes); narrower nodes if the stack bound would not hold
    // (the 8-wide quantised form is built, verified and uploaded only by the GDPT_HBM_BVH8 A/B library: a product upload neither
    // pays for it nor can fail on it)
    WideBvh wide = collapse_for_traversal(bvh.nodes, opt.with_bvh8);
    if (wide.stack_need > GDPT_BVH_MAX_DEPTH) throw std::runtime_error("gdpt_scene_upload: BVH deeper than the traversal stack (builder bug)");
    if (wide.stack_need8 > GDPT_BVH_MAX_DEPTH + GDPT_STACK_OVERFLOW) throw std::runtime_error("gdpt_scene_upload: BVH8 deeper than the traversal stack (builder bug)");
    static_assert(sizeof(DevBvh8Node) == 128 && sizeof(DevBvh4Node) == 128, "wide BVH nodes are one 128-byte line");
    tr.wide_stack_need = wide.stack_need;
    tr.wide8_stack_need = wide.stack_need8;
    std::vector<DevPrim> &prims = ps->prims;
    prims.resize(bvh.order.size());
    for (size_t i = 0; i < bvh.order.size(); i++) prims[i] = f.prim_in[ref_prim[bvh.order[i]]];
    tr.bvh_depth = bvh.depth;
    for (const DevBvhNode &n : bvh.nodes)
        for (int32_t ch : {n.left, n.right}) if (ch < 0 && ch != GDPT_CHILD_EMPTY) tr.leaf_hist[~(unsigned)ch & 3u]++;
    if (bvh.depth > GDPT_BVH_MAX_DEPTH) throw std::runtime_error("gdpt_scene_upload: BVH deeper than the traversal stack (builder bug)");
    ps->nodes = std::move(bvh.nodes);
    ps->nodes4 = std::move(wide.nodes);
    ps->nodes8 = std::move(wide.nodes8);
    if (opt.with_q4) ps->nodes4q = quantise_bvh4(ps->nodes4);
}

// ---- textures: fp64 mip chains exactly as make_mipmap builds them (src/mipmap.h:27-48) ----
void build_textures(const GdptSceneDesc *desc, PreparedScene *ps) {
    std::vector<DevImage> &images = ps->images;
    std::vector<double> &texels = ps->texels;
    for (int i = 0; i < desc->num_images; i++) {
        const GdptImage &im = desc->images[i];
        if (im.width <= 0 || im.height <= 0 || (im.channels != 1 && im.channels != 3) || !im.texels)
            throw std::runtime_error("gdpt_scene_upload: bad image");
        DevImage di{};
        di.channels = im.channels;
        int size = std::max(im.width, im.height);
        int num_levels = std::min((int)std::ceil(std::log2((double)size) + 1), 8);
        di.num_levels = num_levels;
        int pw = im.width, ph = im.height;
        size_t prev_off = texels.size();
        di.width[0] = pw; di.height[0] = ph; di.offset[0] = (int64_t)prev_off;
        texels.insert(texels.end(), im.texels, im.texels + (size_t)pw * ph * im.channels);
        for (int l = 1; l < num_levels; l++) {
            int nw = std::max(pw / 2, 1), nh = std::max(ph / 2, 1);
            size_t off = texels.size();
            texels.resize(off + (size_t)nw * nh * im.channels);
            auto P = [&](int x, int y, int c) { x = std::min(x, pw - 1); y = std::min(y, ph - 1); return texels[prev_off + ((size_t)y * pw + x) * im.channels + c]; };
            for (int y = 0; y < nh; y++) for (int x = 0; x < nw; x++) for (int c = 0; c < im.channels; c++)
                texels[off + ((size_t)y * nw + x) * im.channels + c] =
                    (P(2 * x, 2 * y, c) + P(2 * x + 1, 2 * y, c) + P(2 * x, 2 * y + 1, c) + P(2 * x + 1, 2 * y + 1, c)) / 4.0;
            di.width[l] = nw; di.height[l] = nh; di.offset[l] = (int64_t)off;
            prev_off = off; pw = nw; ph = nh;
        }
        images.push_back(di);
    }
}

// ---- Integrator::Path emitter tables (same formulas and operation order as the reference); returns every emitter's power, the
// environment map's slot still 0 ----
std::vector<double> build_emitters(const GdptSceneDesc *desc, PreparedScene *ps) {
    std::vector<DevLight> &dlights = ps->lights;
    std::vector<double> &light_tri_cdf = ps->light_tri_cdf, &light_tri_pos = ps->light_tri_pos, &light_tri_nrm = ps->light_tri_nrm;
    std::vector<int> sphere_index_of_shape((size_t)desc->num_shapes, -1);
    { int k = 0; for (int s = 0; s < desc->num_shapes; s++) if (desc->shapes[s].type == GDPT_SHAPE_SPHERE) sphere_index_of_shape[(size_t)s] = k++; }
    std::vector<double> power;
    for (int l = 0; l < desc->num_lights; l++) {
        const GdptLight &lt = desc->lights[l];
        if (lt.shape_id < 0 && desc->has_envmap && l == desc->envmap.light_id) {      // environment map: power filled in by build_envmap
            dlights.push_back(DevLight{});
            power.push_back(0.0);
            continue;
        }
        if (lt.shape_id < 0 || lt.shape_id >= desc->num_shapes) throw std::runtime_error("gdpt_scene_upload: light without a shape");
        const GdptShape &sh = desc->shapes[lt.shape_id];
        DevLight dl{};
        for (int k = 0; k < 3; k++) dl.intensity[k] = lt.intensity[k];
        if (sh.type == GDPT_SHAPE_SPHERE) {
            dl.is_sphere = 1; dl.sphere_index = sphere_index_of_shape[(size_t)lt.shape_id];
            dl.area = 4 * 3.14159265358979323846 * sh.radius * sh.radius;                 // sphere.inl:207-209
        } else {
            dl.tri_first = (int)(light_tri_pos.size() / 9); dl.tri_count = sh.num_triangles;
            dl.cdf_first = (int)light_tri_cdf.size(); dl.has_normals = sh.normals ? 1 : 0;
            std::vector<double> areas((size_t)sh.num_triangles), pmf, cdf;
            double total = 0;
            for (int t = 0; t < sh.num_triangles; t++) {
                const int *ix = sh.indices + 3 * t;
                double p[3][3];
                for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) { p[i][k] = sh.positions[3 * ix[i] + k]; light_tri_pos.push_back(p[i][k]); }
                for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) light_tri_nrm.push_back(sh.normals ? sh.normals[3 * ix[i] + k] : 0.0);
                const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                areas[(size_t)t] = std::sqrt(cx * cx + cy * cy + cz * cz) / 2;               // triangle_mesh.inl:70
                total += areas[(size_t)t];
            }
            table_1d(areas, pmf, cdf);
            light_tri_cdf.insert(light_tri_cdf.end(), cdf.begin(), cdf.end());
            dl.area = total;
        }
        const double lum = lt.intensity[0] * 0.212671 + lt.intensity[1] * 0.715160 + lt.intensity[2] * 0.072169;   // src/spectrum.h:33-35
        power.push_back(lum * dl.area * 3.14159265358979323846);                              // diffuse_area_light.inl:1-3
        dlights.push_back(dl);
    }
    return power;
}

// ---- the camera, the view's scalars and the traits that choose the route; returns the radius of the fp32 scene bounds ----
double fill_view_and_traits(const GdptSceneDesc *desc, const Flat &f, PreparedScene *ps) {
    const GdptCamera &cam = desc->camera;
    const std::vector<GdptMaterial> &materials = ps->materials;
    const float *lb = f.lb, *ub = f.ub;
    SceneTraits &tr = ps->traits;
    DevSceneView &v = ps->view;
    fill_camera(cam, &v.cam);
    v.num_nodes = (int)ps->nodes.size(); v.num_nodes4 = (int)ps->nodes4.size(); v.num_nodes8 = (int)ps->nodes8.size(); v.num_prims = (int)ps->prims.size();
    v.num_tris = (int)ps->tris.size(); v.num_spheres = (int)ps->spheres.size();
    v.num_materials = desc->num_materials; v.num_lights = desc->num_lights; v.num_images = desc->num_images;
    v.max_depth = desc->max_depth; v.rr_depth = desc->rr_depth;
    v.all_textures_constant = 1;
    for (auto &m : materials) for (auto &t : m.tex) if (t.type != GDPT_TEX_CONSTANT) v.all_textures_constant = 0;
    for (auto &m : materials) {
        tr.material_mask |= 1u << m.type;
        if (m.type != GDPT_MAT_LAMBERTIAN) tr.lambert_only = false;
        if (m.type == GDPT_MAT_ROUGHPLASTIC || m.type == GDPT_MAT_ROUGHDIELECTRIC) tr.has_rough = true;
        if (m.type == GDPT_MAT_DISNEY_GLASS || m.type == GDPT_MAT_DISNEY_BSDF || m.type == GDPT_MAT_ROUGHDIELECTRIC) tr.one_sided = false;   // two-sided lobes
    }
    // scenes with a refractive lobe (DisneyGlass, RoughDielectric): paths through glass are long-tailed, the work items are cut smaller
    // (render_kernels.hip: make_chunk_plan; disney_glass +9..15 %, matpreview's Integrator::Path +7 %; DisneyBSDF and the opaque scenes are flat)
    if (tr.material_mask & ((1u << GDPT_MAT_DISNEY_GLASS) | (1u << GDPT_MAT_ROUGHDIELECTRIC))) tr.plan_take_pct = 40;
    // get_intersection_epsilon (src/scene.h:100-102) from Embree-style fp32 scene bounds (src/scene.cpp:29-33)
    double dx = (double)ub[0] - (double)lb[0], dy = (double)ub[1] - (double)lb[1], dz = (double)ub[2] - (double)lb[2];
    double radius = ps->prims.empty() ? 0.0 : std::sqrt(dx * dx + dy * dy + dz * dz) / 2;
    for (int k = 0; k < 3; k++) { tr.bounds[k] = lb[k]; tr.bounds[3 + k] = ub[k]; }
    v.isect_eps = std::min(radius * 1e-5, 0.01);
    return radius;
}

// ---- environment map (Integrator::Path): TableDist2D over luminance * sin(elevation) of the level-0 image
// (init_sampling_dist, src/lights/envmap.inl:66-83; make_table_dist_2d, src/table_dist.cpp:40-112) and its power
// (envmap.inl:1-5), which goes into its slot of `light_power` ----
void build_envmap(const GdptSceneDesc *desc, double radius, std::vector<double> &light_power, PreparedScene *ps) {
    DevSceneView &v = ps->view;
    const int env_power_slot = desc->has_envmap ? desc->envmap.light_id : -1;
    v.has_envmap = 0; v.env_light_id = -1;
    if (desc->has_envmap) {
        const GdptEnvmap &e = desc->envmap;
        if (e.image_id < 0 || e.image_id >= desc->num_images || desc->images[e.image_id].channels != 3)
            throw std::runtime_error("gdpt_scene_upload: environment map without a 3-channel image");
        const GdptImage &im = desc->images[e.image_id];
        const int w = im.width, h = im.height;
        auto texel = [&](int x, int y) { const double *p = im.texels + ((size_t)y * w + x) * 3; return p; };
        auto modulo = [](int a, int b) { int r = a % b; return r < 0 ? r + b : r; };
        std::vector<double> f((size_t)w * h);
        size_t i = 0;
        for (int y = 0; y < h; y++) {
            const double vv = (y + 0.5) / (double)h;
            const double sin_elevation = std::sin(3.14159265358979323846 * vv);
            for (int x = 0; x < w; x++) {
                const double uu = (x + 0.5) / (double)w;
                // lookup(mipmap, u, v, 0): bilinear at level 0 with repeat wrap (src/mipmap.h:51-72)
                double u = uu * w - 0.5, vq = vv * h - 0.5;
                int ufi = modulo((int)u, w), vfi = modulo((int)vq, h);
                int uci = modulo(ufi + 1, w), vci = modulo(vfi + 1, h);
                double u_off = u - ufi, v_off = vq - vfi;
                double rgb[3];
                for (int c = 0; c < 3; c++)
                    rgb[c] = texel(ufi, vfi)[c] * (1 - u_off) * (1 - v_off) + texel(ufi, vci)[c] * (1 - u_off) * v_off +
                             texel(uci, vfi)[c] * u_off * (1 - v_off) + texel(uci, vci)[c] * u_off * v_off;
                f[i++] = (rgb[0] * 0.212671 + rgb[1] * 0.715160 + rgb[2] * 0.072169) * sin_elevation;
            }
        }
        std::vector<double> &cdf_rows = ps->env_cdf_rows, &pdf_rows = ps->env_pdf_rows, &cdf_m = ps->env_cdf_marginals, &pdf_m = ps->env_pdf_marginals;
        cdf_rows.assign((size_t)h * (w + 1), 0.0); pdf_rows.assign((size_t)h * w, 0.0); cdf_m.assign((size_t)h + 1, 0.0); pdf_m.assign((size_t)h, 0.0);
        for (int y = 0; y < h; y++) {
            double *cdf = &cdf_rows[(size_t)y * (w + 1)];
            cdf[0] = 0;
            for (int x = 0; x < w; x++) cdf[x + 1] = cdf[x] + f[(size_t)y * w + x];
            const double integral = cdf[w];
            if (integral > 0) {
                for (int x = 0; x < w; x++) cdf[x] /= integral;
                for (int x = 0; x < w; x++) pdf_rows[(size_t)y * w + x] = f[(size_t)y * w + x] / integral;
            } else {
                for (int x = 0; x < w; x++) { pdf_rows[(size_t)y * w + x] = 1.0 / (double)w; cdf[x] = (double)x / (double)w; }
                cdf[w] = 1;
            }
        }
        cdf_m[0] = 0;
        for (int y = 0; y < h; y++) cdf_m[(size_t)y + 1] = cdf_m[(size_t)y] + cdf_rows[(size_t)y * (w + 1) + w];
        const double total_values = cdf_m.back();
        if (total_values > 0) {
            for (int y = 0; y < h; y++) cdf_m[(size_t)y] /= total_values;
            cdf_m[(size_t)h] = 1;
            for (int y = 0; y < h; y++) pdf_m[(size_t)y] = cdf_rows[(size_t)y * (w + 1) + w] / total_values;
        } else {
            for (int y = 0; y < h; y++) { pdf_m[(size_t)y] = 1.0 / (double)h; cdf_m[(size_t)y] = (double)y / (double)h; }
            cdf_m[(size_t)h] = 1;
        }
        for (int y = 0; y < h; y++) cdf_rows[(size_t)y * (w + 1) + w] = 1;
        v.has_envmap = 1; v.env_light_id = e.light_id; v.env_image_id = e.image_id; v.env_w = w; v.env_h = h; v.env_scale = e.scale;
        std::memcpy(v.env_to_world, e.to_world, sizeof(v.env_to_world));
        std::memcpy(v.env_to_local, e.to_local, sizeof(v.env_to_local));
        if (env_power_slot >= 0 && env_power_slot < (int)light_power.size())
            light_power[(size_t)env_power_slot] = 3.14159265358979323846 * radius * radius * total_values / ((double)w * (double)h);
    }
}

} // namespace

void fill_camera(const GdptCamera &cam, DevCamera *out) {
    DevCamera &c = *out;
    std::memcpy(c.sample_to_cam, cam.sample_to_cam, sizeof(c.sample_to_cam));
    std::memcpy(c.cam_to_world, cam.cam_to_world, sizeof(c.cam_to_world));
    {   // xform_point(cam_to_world, (0,0,0)), src/camera.cpp:42
        const double *m = cam.cam_to_world;
        double inv_w = 1.0 / m[15];
        c.org[0] = m[3] * inv_w; c.org[1] = m[7] * inv_w; c.org[2] = m[11] * inv_w;
    }
    c.width = cam.width; c.height = cam.height; c.filter_type = cam.filter_type; c.filter_param = cam.filter_param;
    c.pow2_film = ((cam.width & (cam.width - 1)) == 0 && (cam.height & (cam.height - 1)) == 0) ? 1 : 0;
    c.inv_width = 1.0 / (double)cam.width; c.inv_height = 1.0 / (double)cam.height;
}

float camera_extent(const GdptCamera &cam) {
    const double *m = cam.cam_to_world;
    float ext = 0.f;
    for (int k = 0; k < 3; k++) ext = std::max(ext, (float)std::fabs(m[4 * k + 3] / m[15]) * 1.0000002f);
    return ext;
}

PreparedScene prepare_scene(const GdptSceneDesc &desc, const PrepareOptions &opt) {
    PreparedScene ps;
    check_description(&desc);
    const Flat f = flatten(&desc, &ps);
    build_tree(desc.camera, f, opt, &ps);
    build_textures(&desc, &ps);
    ps.materials.assign(desc.materials, desc.materials + desc.num_materials);
    for (int l = 0; l < desc.num_lights; l++) for (int k = 0; k < 3; k++) ps.light_intensity.push_back(desc.lights[l].intensity[k]);
    std::vector<double> light_power = build_emitters(&desc, &ps);
    const double radius = fill_view_and_traits(&desc, f, &ps);
    build_envmap(&desc, radius, light_power, &ps);
    // only now the light selection table (src/scene.cpp:44-53)
    if (!light_power.empty()) table_1d(light_power, ps.light_pmf, ps.light_cdf);
    return ps;
}

} // namespace gdpt
