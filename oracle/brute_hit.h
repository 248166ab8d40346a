// brute_hit.h — the project's definition of a ray/triangle hit and of "closest", in one place.
//
// TEST INFRASTRUCTURE ONLY. Included by oracle.cpp (the CPU oracle) and by rtc_standin.cpp (the brute-force stand-in
// that the reference's own sources are linked against when fixtures are generated), so that with equal fp32 rays both
// return equal bits: same triangle test, same tie-break, same normal. Both are compiled with -ffp-contract=off.
#ifndef GDPT_ORACLE_BRUTE_HIT_H
#define GDPT_ORACLE_BRUTE_HIT_H

namespace brute {

struct Tri {            // fp32 traversal copy (src/shapes/triangle_mesh.inl:11-14) + ids
    float v0[3], e1[3], e2[3];
    int shape_id, prim_id;
};

inline Tri make_tri(const float a[3], const float b[3], const float c[3], int shape_id, int prim_id) {
    Tri tr; tr.shape_id = shape_id; tr.prim_id = prim_id;
    for (int k = 0; k < 3; k++) { tr.v0[k] = a[k]; tr.e1[k] = b[k] - a[k]; tr.e2[k] = c[k] - a[k]; }
    return tr;
}

// What Moller-Trumbore computes before any decision is taken: det == 0 leaves the rest unset.
struct TriProbe { float det, u, v, t; };

// ---- fp32 ray/triangle (normative definition shared with the HIP kernel, bit for bit) -----------
// Moller-Trumbore, two-sided, every product and sum rounded separately (no FMA), left-to-right sums.
// `probe`, when given, receives every quantity that was computed before the test returned (NaN for the others).
inline bool tri_hit(const float o[3], const float d[3], float tnear, float tfar, const Tri &tr, float *t_out, float *u_out, float *v_out,
                    TriProbe *probe = nullptr) {
    const float *e1 = tr.e1, *e2 = tr.e2;
    const float qnan = __builtin_nanf("");
    float px = d[1] * e2[2] - d[2] * e2[1];
    float py = d[2] * e2[0] - d[0] * e2[2];
    float pz = d[0] * e2[1] - d[1] * e2[0];
    float det = e1[0] * px + e1[1] * py + e1[2] * pz;
    if (probe) { probe->det = det; probe->u = probe->v = probe->t = qnan; }
    if (!(det != 0.0f)) return false;
    float inv = 1.0f / det;
    float sx = o[0] - tr.v0[0], sy = o[1] - tr.v0[1], sz = o[2] - tr.v0[2];
    float u = (sx * px + sy * py + sz * pz) * inv;
    float qx = sy * e1[2] - sz * e1[1];
    float qy = sz * e1[0] - sx * e1[2];
    float qz = sx * e1[1] - sy * e1[0];
    if (probe) {        // the same expressions as below, evaluated regardless of the earlier exits
        probe->u = u;
        probe->v = (d[0] * qx + d[1] * qy + d[2] * qz) * inv;
        probe->t = (e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv;
    }
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    float v = (d[0] * qx + d[1] * qy + d[2] * qz) * inv;
    if (!(v >= 0.0f && u + v <= 1.0f)) return false;
    float t = (e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv;
    if (!(t >= tnear && t < tfar)) return false;
    *t_out = t; *u_out = u; *v_out = v;
    return true;
}

// Ng = e1 x e2 in fp32 (Embree reports an unnormalised fp32 Ng), one rounding per op
inline void tri_ng(const Tri &tr, float ng[3]) {
    ng[0] = tr.e1[1] * tr.e2[2] - tr.e1[2] * tr.e2[1];
    ng[1] = tr.e1[2] * tr.e2[0] - tr.e1[0] * tr.e2[2];
    ng[2] = tr.e1[0] * tr.e2[1] - tr.e1[1] * tr.e2[0];
}

// Closest: the smallest t, ties to the lowest id (gid: triangles of all meshes in shape order, then the spheres).
inline bool replaces(float t, int gid, bool have_best, float best_t, int best_gid) {
    return !have_best || t < best_t || (t == best_t && gid < best_gid);
}

} // namespace brute
#endif
