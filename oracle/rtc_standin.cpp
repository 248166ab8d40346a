// rtc_standin.cpp — a brute-force stand-in for the 21 rtc* entry points the reference calls.
//
// Built only where the reference tree is present (oracle/Makefile target `ref_samples`), against the Embree 4 HEADERS
// that lie in that tree; the library itself is not available. Everything in this file is this repository's own code.
//
// The closest hit is the project's definition: fp32 Moller-Trumbore from brute_hit.h, which oracle.cpp
// includes as well, the smallest t, ties to the lowest id (triangles of all meshes in geometry order, then the user
// geometries), t in [tnear, tfar), Ng = e1 x e2 in fp32. With equal fp32 rays the oracle and this file return equal bits.
// User geometries (the reference's spheres) are answered by the reference's own bounds / intersect / occluded callbacks,
// called with a valid RTCRayQueryContext and, each time, with the ray's original tfar.
//
// While answering, every ray also records how close its answer was to changing (`margin`, see note_* below); the
// generator reads the minimum over a sample's rays to tell well-conditioned samples from the others.
#include <embree4/rtcore.h>

#include "brute_hit.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Geometry {
    RTCGeometryType type = RTC_GEOMETRY_TYPE_TRIANGLE;
    int refs = 1;
    std::vector<char> vertex_bytes, index_bytes;
    size_t vertex_stride = 0, vertex_count = 0, index_stride = 0, index_count = 0;
    void *user = nullptr;
    unsigned int user_prims = 0;
    RTCBoundsFunction bounds = nullptr;
    RTCIntersectFunctionN intersect = nullptr;
    RTCOccludedFunctionN occluded = nullptr;
};

struct UserPrim { unsigned int geom_id, prim_id; Geometry *g; float center[3], radius; };

struct SceneImpl {
    int refs = 1;
    std::vector<Geometry *> geoms;          // index = geomID
    std::vector<brute::Tri> tris;           // gid order; shape_id = geomID, prim_id = primID
    std::vector<UserPrim> users;            // gid = tris.size() + k
    float lower[3], upper[3];
};

int g_device_token;
thread_local double g_margin = std::numeric_limits<double>::infinity();

thread_local int g_kind = -1;
thread_local bool g_have_first = false;     // the first ray answered since the last reset (the generator's check of the draw order)
thread_local float g_first[6];
enum { KIND_EDGE = 0, KIND_RUNNER_UP = 1, KIND_NEAR_MISS = 2, KIND_INTERVAL = 3, KIND_SILHOUETTE = 4 };

inline void note(double m, int kind) { if (m < g_margin) { g_margin = m; g_kind = kind; } }      // NaN never lowers the margin

void release(Geometry *g) { if (--g->refs == 0) delete g; }

inline float edge_distance(float u, float v) { return std::min(std::min(u, v), 1.0f - u - v); }

// Relative distance of a candidate's t to the ends of the ray's interval (a candidate inside the triangle only).
inline void note_interval(float t, float tnear, float tfar) {
    if (std::isfinite(tfar)) note(std::fabs((double)t - tfar) / std::max((double)std::fabs(tfar), (double)FLT_MIN), KIND_INTERVAL);
    note(std::fabs((double)t - tnear) / std::max(std::max((double)std::fabs(tnear), (double)std::fabs(t)), (double)FLT_MIN), KIND_INTERVAL);
}

// A user primitive's silhouette, from its bounds callback's sphere: by what angle the fp32 direction, or by what
// share of its size the fp32 origin, would have to move for the ray's line to change sides of the silhouette. With b the
// distance of the line from the centre and s the length along the ray to the point nearest the centre, a rotation by
// phi moves b by s phi and a shift of the origin by at most itself. (The callback decides in fp64; what can differ
// between two computations of one sample is the last fp32 bit of the ray.)
inline void note_sphere(const UserPrim &p, const float o[3], const float d[3]) {
    double v[3] = {(double)p.center[0] - o[0], (double)p.center[1] - o[1], (double)p.center[2] - o[2]};
    double dd = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
    if (!(dd > 0) || !(p.radius > 0)) return;
    double s = (v[0] * d[0] + v[1] * d[1] + v[2] * d[2]) / dd;
    double q[3] = {v[0] - s * d[0], v[1] - s * d[1], v[2] - s * d[2]};
    double b = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    double lever = std::max(std::fabs(s) * std::sqrt(dd), (double)std::max(std::fabs(o[0]), std::max(std::fabs(o[1]), std::fabs(o[2]))));
    note(std::fabs(b - p.radius) / std::max(lever, (double)FLT_MIN), KIND_SILHOUETTE);
}

struct Best { bool valid = false; float t = 0, u = 0, v = 0, ng[3] = {0, 0, 0}; int gid = -1; unsigned int geom_id = 0, prim_id = 0; };

// One ray against everything. any_hit only changes what is recorded as margin, not the search: the oracle answers
// occluded() with its closest-hit search too, and "some primitive accepts the ray" does not depend on the order.
Best trace(const SceneImpl &sc, const float o[3], const float d[3], float tnear, float tfar, bool any_hit) {
    Best best;
    if (!g_have_first) { g_have_first = true; for (int k = 0; k < 3; k++) { g_first[k] = o[k]; g_first[3 + k] = d[k]; } }
    if (!(tnear < tfar)) return best;       // no t satisfies tnear <= t < tfar (grad_path_tracing's four tnear = tfar = 0 rays)
    const int ntri = (int)sc.tris.size();
    float runner_up = std::numeric_limits<float>::infinity();       // the second smallest accepted t
    std::vector<std::pair<float, float>> rejected;                  // (t, distance outside) of near misses inside the interval
    for (int gid = 0; gid < ntri; gid++) {
        float t, u, v;
        brute::TriProbe pr;
        bool hit = brute::tri_hit(o, d, tnear, tfar, sc.tris[gid], &t, &u, &v, &pr);
        if (!(pr.det != 0.0f)) continue;
        float e = edge_distance(pr.u, pr.v);
        if (e >= 0.0f) note_interval(pr.t, tnear, tfar);
        if (!hit) {
            if (pr.t >= tnear && pr.t < tfar && e < 0.0f) {
                if (any_hit) note(-(double)e, KIND_NEAR_MISS);
                else if (-e < 1e-3f) rejected.emplace_back(pr.t, -e);
            }
            continue;
        }
        if (any_hit) note(e, KIND_EDGE);
        if (brute::replaces(t, gid, best.valid, best.t, best.gid)) {
            if (best.valid) runner_up = std::min(runner_up, best.t);
            best.valid = true; best.t = t; best.u = u; best.v = v; best.gid = gid;
            best.geom_id = (unsigned int)sc.tris[gid].shape_id; best.prim_id = (unsigned int)sc.tris[gid].prim_id;
            brute::tri_ng(sc.tris[gid], best.ng);
        } else {
            runner_up = std::min(runner_up, t);
        }
    }
    for (size_t k = 0; k < sc.users.size(); k++) {
        const UserPrim &p = sc.users[k];
        const int gid = ntri + (int)k;
        note_sphere(p, o, d);
        RTCRayHit rh;
        std::memset(&rh, 0, sizeof(rh));
        rh.ray.org_x = o[0]; rh.ray.org_y = o[1]; rh.ray.org_z = o[2]; rh.ray.tnear = tnear;
        rh.ray.dir_x = d[0]; rh.ray.dir_y = d[1]; rh.ray.dir_z = d[2]; rh.ray.time = 0.f; rh.ray.tfar = tfar;
        rh.ray.mask = (unsigned int)(-1);
        rh.hit.geomID = rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
        rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
        RTCRayQueryContext ctx;
        rtcInitRayQueryContext(&ctx);
        int valid = -1;
        RTCIntersectFunctionNArguments a;
        a.valid = &valid; a.geometryUserPtr = p.g->user; a.primID = p.prim_id; a.context = &ctx;
        a.rayhit = (RTCRayHitN *)&rh; a.N = 1; a.geomID = p.geom_id;
        if (!p.g->intersect) { fprintf(stderr, "rtc_standin: user geometry without an intersect callback\n"); abort(); }
        p.g->intersect(&a);
        if (rh.hit.geomID == RTC_INVALID_GEOMETRY_ID) continue;
        float t = rh.ray.tfar;
        note_interval(t, tnear, tfar);
        if (any_hit && p.g->occluded) {     // the reference's occluded callback must agree with its intersect callback
            RTCRay r = rh.ray; r.tfar = tfar;
            RTCOccludedFunctionNArguments oa;
            oa.valid = &valid; oa.geometryUserPtr = p.g->user; oa.primID = p.prim_id; oa.context = &ctx;
            oa.ray = (RTCRayN *)&r; oa.N = 1; oa.geomID = p.geom_id;
            p.g->occluded(&oa);
            if (!(r.tfar < 0)) { fprintf(stderr, "rtc_standin: occluded and intersect callbacks disagree\n"); abort(); }
        }
        if (brute::replaces(t, gid, best.valid, best.t, best.gid)) {
            if (best.valid) runner_up = std::min(runner_up, best.t);
            best.valid = true; best.t = t; best.u = rh.hit.u; best.v = rh.hit.v; best.gid = gid;
            best.geom_id = p.geom_id; best.prim_id = p.prim_id;
            best.ng[0] = rh.hit.Ng_x; best.ng[1] = rh.hit.Ng_y; best.ng[2] = rh.hit.Ng_z;
        } else {
            runner_up = std::min(runner_up, t);
        }
    }
    if (!any_hit) {
        if (best.valid) {
            if (best.gid < ntri) note(edge_distance(best.u, best.v), KIND_EDGE);
            if (std::isfinite(runner_up)) note(((double)runner_up - best.t) / std::max((double)std::fabs(best.t), (double)FLT_MIN), KIND_RUNNER_UP);
        }
        // a near miss matters where it would have been the closest hit
        for (const auto &r : rejected) if (!best.valid || r.first <= best.t) note(r.second, KIND_NEAR_MISS);
    }
    return best;
}

} // namespace

extern "C" {

// ---- read by the generator (not part of Embree's interface) ----
void rtc_standin_margin_reset(void) { g_margin = std::numeric_limits<double>::infinity(); g_kind = -1; g_have_first = false; }
int rtc_standin_first_ray(float org_dir[6]) { if (g_have_first) std::memcpy(org_dir, g_first, sizeof(g_first)); return g_have_first; }
double rtc_standin_margin(void) { return g_margin; }
int rtc_standin_margin_kind(void) { return g_kind; }      // which of the KIND_* gave the minimum (-1: no ray recorded anything)

RTC_API RTCDevice rtcNewDevice(const char *) { return (RTCDevice)&g_device_token; }
RTC_API void rtcReleaseDevice(RTCDevice) {}

RTC_API RTCScene rtcNewScene(RTCDevice) { return (RTCScene) new SceneImpl(); }
RTC_API void rtcReleaseScene(RTCScene s) {
    SceneImpl *sc = (SceneImpl *)s;
    if (--sc->refs == 0) { for (Geometry *g : sc->geoms) release(g); delete sc; }
}
RTC_API void rtcSetSceneBuildQuality(RTCScene, enum RTCBuildQuality) {}
RTC_API void rtcSetSceneFlags(RTCScene, enum RTCSceneFlags) {}

RTC_API unsigned int rtcAttachGeometry(RTCScene s, RTCGeometry g) {
    SceneImpl *sc = (SceneImpl *)s;
    ((Geometry *)g)->refs++;
    sc->geoms.push_back((Geometry *)g);
    return (unsigned int)(sc->geoms.size() - 1);
}

RTC_API void rtcCommitScene(RTCScene s) {
    SceneImpl *sc = (SceneImpl *)s;
    sc->tris.clear(); sc->users.clear();
    for (int k = 0; k < 3; k++) { sc->lower[k] = std::numeric_limits<float>::infinity(); sc->upper[k] = -sc->lower[k]; }
    for (size_t gi = 0; gi < sc->geoms.size(); gi++) {
        Geometry *g = sc->geoms[gi];
        if (g->type != RTC_GEOMETRY_TYPE_TRIANGLE) continue;
        auto P = [&](unsigned int i) { return (const float *)(g->vertex_bytes.data() + (size_t)i * g->vertex_stride); };
        for (size_t t = 0; t < g->index_count; t++) {
            const unsigned int *ix = (const unsigned int *)(g->index_bytes.data() + t * g->index_stride);
            for (int i = 0; i < 3; i++) if (ix[i] >= g->vertex_count) { fprintf(stderr, "rtc_standin: index out of range\n"); abort(); }
            sc->tris.push_back(brute::make_tri(P(ix[0]), P(ix[1]), P(ix[2]), (int)gi, (int)t));
        }
        for (size_t i = 0; i < g->vertex_count; i++) for (int k = 0; k < 3; k++) {      // the bounds cover the vertex buffer
            float p = P((unsigned int)i)[k]; sc->lower[k] = std::min(sc->lower[k], p); sc->upper[k] = std::max(sc->upper[k], p);
        }
    }
    for (size_t gi = 0; gi < sc->geoms.size(); gi++) {
        Geometry *g = sc->geoms[gi];
        if (g->type != RTC_GEOMETRY_TYPE_USER) continue;
        for (unsigned int pi = 0; pi < g->user_prims; pi++) {
            RTCBounds b;
            std::memset(&b, 0, sizeof(b));
            RTCBoundsFunctionArguments a;
            a.geometryUserPtr = g->user; a.primID = pi; a.timeStep = 0; a.bounds_o = &b;
            if (!g->bounds) { fprintf(stderr, "rtc_standin: user geometry without a bounds callback\n"); abort(); }
            g->bounds(&a);
            const float lo[3] = {b.lower_x, b.lower_y, b.lower_z}, hi[3] = {b.upper_x, b.upper_y, b.upper_z};
            UserPrim p; p.geom_id = (unsigned int)gi; p.prim_id = pi; p.g = g;
            for (int k = 0; k < 3; k++) {
                sc->lower[k] = std::min(sc->lower[k], lo[k]); sc->upper[k] = std::max(sc->upper[k], hi[k]);
                p.center[k] = 0.5f * (lo[k] + hi[k]);
            }
            p.radius = 0.5f * (hi[0] - lo[0]);
            sc->users.push_back(p);
        }
    }
}

RTC_API void rtcGetSceneBounds(RTCScene s, struct RTCBounds *o) {
    SceneImpl *sc = (SceneImpl *)s;
    std::memset(o, 0, sizeof(*o));
    o->lower_x = sc->lower[0]; o->lower_y = sc->lower[1]; o->lower_z = sc->lower[2];
    o->upper_x = sc->upper[0]; o->upper_y = sc->upper[1]; o->upper_z = sc->upper[2];
}

RTC_API RTCGeometry rtcNewGeometry(RTCDevice, enum RTCGeometryType type) {
    if (type != RTC_GEOMETRY_TYPE_TRIANGLE && type != RTC_GEOMETRY_TYPE_USER) { fprintf(stderr, "rtc_standin: geometry type %d\n", (int)type); abort(); }
    Geometry *g = new Geometry();
    g->type = type;
    return (RTCGeometry)g;
}
RTC_API void rtcReleaseGeometry(RTCGeometry g) { release((Geometry *)g); }
RTC_API void rtcCommitGeometry(RTCGeometry) {}
RTC_API void rtcSetGeometryVertexAttributeCount(RTCGeometry, unsigned int) {}

RTC_API void *rtcSetNewGeometryBuffer(RTCGeometry gg, enum RTCBufferType type, unsigned int slot, enum RTCFormat format, size_t byteStride, size_t itemCount) {
    Geometry *g = (Geometry *)gg;
    if (slot != 0) { fprintf(stderr, "rtc_standin: buffer slot %u\n", slot); abort(); }
    if (type == RTC_BUFFER_TYPE_VERTEX && format == RTC_FORMAT_FLOAT3) {
        g->vertex_stride = byteStride; g->vertex_count = itemCount;
        g->vertex_bytes.assign(byteStride * itemCount + 16, 0);
        return g->vertex_bytes.data();
    }
    if (type == RTC_BUFFER_TYPE_INDEX && format == RTC_FORMAT_UINT3) {
        g->index_stride = byteStride; g->index_count = itemCount;
        g->index_bytes.assign(byteStride * itemCount + 16, 0);
        return g->index_bytes.data();
    }
    fprintf(stderr, "rtc_standin: buffer type %d format %d\n", (int)type, (int)format);
    abort();
}

RTC_API void rtcSetGeometryUserPrimitiveCount(RTCGeometry g, unsigned int n) { ((Geometry *)g)->user_prims = n; }
RTC_API void rtcSetGeometryUserData(RTCGeometry g, void *p) { ((Geometry *)g)->user = p; }
RTC_API void rtcSetGeometryBoundsFunction(RTCGeometry g, RTCBoundsFunction f, void *) { ((Geometry *)g)->bounds = f; }
RTC_API void rtcSetGeometryIntersectFunction(RTCGeometry g, RTCIntersectFunctionN f) { ((Geometry *)g)->intersect = f; }
RTC_API void rtcSetGeometryOccludedFunction(RTCGeometry g, RTCOccludedFunctionN f) { ((Geometry *)g)->occluded = f; }

RTC_API void rtcIntersect1(RTCScene s, struct RTCRayHit *rh, struct RTCIntersectArguments *) {
    const float o[3] = {rh->ray.org_x, rh->ray.org_y, rh->ray.org_z}, d[3] = {rh->ray.dir_x, rh->ray.dir_y, rh->ray.dir_z};
    Best b = trace(*(SceneImpl *)s, o, d, rh->ray.tnear, rh->ray.tfar, false);
    if (!b.valid) return;
    rh->ray.tfar = b.t;
    rh->hit.Ng_x = b.ng[0]; rh->hit.Ng_y = b.ng[1]; rh->hit.Ng_z = b.ng[2];
    rh->hit.u = b.u; rh->hit.v = b.v;
    rh->hit.geomID = b.geom_id; rh->hit.primID = b.prim_id;
    rh->hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
}

RTC_API void rtcOccluded1(RTCScene s, struct RTCRay *r, struct RTCOccludedArguments *) {
    const float o[3] = {r->org_x, r->org_y, r->org_z}, d[3] = {r->dir_x, r->dir_y, r->dir_z};
    Best b = trace(*(SceneImpl *)s, o, d, r->tnear, r->tfar, true);
    if (b.valid) r->tfar = -std::numeric_limits<float>::infinity();
}

} // extern "C"
