// nlm_device.h — the device helpers the non-local-means kernels share (denoise_nlm.hip, nlm_regress.hip): the tile constants, the
// guide's and the divisor's blocks, the tiled form's LDS sizing, a pixel's validity and loading, the pair distance, the thread's own
// features, a pixel's weighted sums (Accum, finish_pixel: nlm_joint.hip shares them with denoise_nlm.hip) and the film sums. `A` is a
// kernel's argument block: the fields of nlm::Args (denoise_nlm.hip), kGuided / kDemod, and with them `gd` / `dm`.
#pragma once
#include "../../../include/gdpt.h"
#include "image_kernels.h"
#include "denoise_nlm.h"

namespace nlm {

using namespace film;             // kBlock, kMaxBlocks, TileGrid, leave_block_sum

constexpr int kTile = gdpt::kNlmTile;
constexpr int kMaxR = GDPT_NLM_MAX_WINDOW_RADIUS, kMaxF = GDPT_NLM_MAX_PATCH_RADIUS;
constexpr int kMaxGroups = GDPT_NLM_MAX_GROUPS, kMaxChannels = GDPT_NLM_MAX_CHANNELS;
static_assert(kTile * kTile == kBlock, "one thread per tile pixel");
static_assert((kTile + 2 * kMaxF) * (kTile + 2 * kMaxF) <= 2 * kBlock, "a thread computes at most two pair distances per offset");

// the guide of a guided call: planes `feat`, `fvar` of `plane` doubles each; group j compares channels [first[j], first[j] + count[j])
struct Guide {
    const double *feat, *fvar;
    size_t plane;
    int groups, first[kMaxGroups], count[kMaxGroups];
    unsigned used;               // bit c: some group names channel c
    double tau[kMaxGroups], kf2, alpha_f;
};
// the divisor of a demodulated call: planes `feat`, `fvar` of `plane` doubles each; the albedo is planes albedo .. albedo + 2, the
// coverage plane `coverage` (< 0: none)
struct Demod {
    const double *feat, *fvar;
    size_t plane;
    int albedo, coverage;
    double floor;
};

// pitch of the e plane for patches of ew = 16 + 2f points a row
__host__ __device__ inline int e_pitch(int f) { return f == 0 ? kTile : 48; }
// doubles, then ints, of the tiled kernel's LDS
__host__ __device__ inline int lds_doubles(int r, int f) {
    const int sw = kTile + 2 * (r + f), ew = kTile + 2 * f;
    return 6 * sw * sw + e_pitch(f) * ew + kTile * ew;
}
__host__ __device__ inline int lds_ints(int r, int f) {
    const int sw = kTile + 2 * (r + f), ew = kTile + 2 * f;
    return sw * sw + e_pitch(f) * ew + kTile * ew;
}

__device__ __forceinline__ bool valid_triples(const double u[3], const double v[3]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) ok = ok && isfinite(u[c]) && isfinite(v[c]) && v[c] >= 0.0;
    return ok;
}

// e_o(x) of two valid pixels a = x, b = x + o
__device__ __forceinline__ double pair_distance(const double ua[3], const double va[3], const double ub[3], const double vb[3], double k2,
                                                double alpha, double eps) {
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double d = ua[c] - ub[c];
        t[c] = (d * d - alpha * (va[c] + fmin(vb[c], va[c]))) / (eps + k2 * (va[c] + vb[c]));
    }
    return ((t[0] + t[1]) + t[2]) / 3.0;
}

struct Sums {
    double var_in = 0.0, sq_in = 0.0, var_out = 0.0, sq_out = 0.0, left_out = 0.0;
};

// the effective albedo a~ of pixel p (film index y w + x); returns whether its albedo and coverage values are valid
__device__ __forceinline__ bool effective_albedo(const Demod &dm, size_t p, double al[3]) {
    bool ok = true;
    double miss = 0.0;               // 1 - cov; without a coverage plane cov = 1
    if (dm.coverage >= 0) {
        const double cov = dm.feat[dm.coverage * dm.plane + p], sc = dm.fvar[dm.coverage * dm.plane + p];
        ok = isfinite(cov) && isfinite(sc) && sc >= 0.0;
        miss = 1.0 - cov;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double g = dm.feat[(dm.albedo + c) * dm.plane + p], sg = dm.fvar[(dm.albedo + c) * dm.plane + p];
        ok = ok && isfinite(g) && isfinite(sg) && sg >= 0.0;
        al[c] = fmax(dm.floor, g + miss);
    }
    return ok;
}

template <class A>
__device__ __forceinline__ void keep_pixel(const A &a, size_t i, const double u[3], const double v[3], Sums &s) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.out[i + c] = u[c];
        if (a.var_out) a.var_out[i + c] = v[c];
    }
    s.left_out += 1.0;
}

template <class A>
__device__ __forceinline__ void leave_partials(const A &a, const Sums &s, double *red) {
    leave_block_sum(a.partials, 0, s.var_in, red);
    leave_block_sum(a.partials, 1, s.sq_in, red);
    const double out = block_sum(s.left_out, red);      // (one sum, left for both reductions)
    if (threadIdx.x == 0) { a.partials[2 * gridDim.x + blockIdx.x] = out; a.partials[5 * gridDim.x + blockIdx.x] = out; }
    leave_block_sum(a.partials, 3, s.var_out, red);
    leave_block_sum(a.partials, 4, s.sq_out, red);
}

// whether every feature channel some group names is finite at pixel i, with variance >= 0
__device__ __forceinline__ bool valid_features(const Guide &gd, size_t i) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < kMaxChannels; c++)
        if (gd.used >> c & 1u) {
            const double g = gd.feat[c * gd.plane + i], s = gd.fvar[c * gd.plane + i];
            ok = ok && isfinite(g) && isfinite(s) && s >= 0.0;
        }
    return ok;
}

// the triples of film pixel (x, y), which is inside the film; returns whether it is valid. A demodulated kernel gets the quotients
// u / a~, v / a~^2 of a valid pixel, and the input bits of an invalid one.
template <class A>
__device__ __forceinline__ bool load_pixel(const A &a, int x, int y, double u[3], double v[3]) {
    const size_t i = ((size_t)y * a.g.w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) { u[c] = a.img[i + c]; v[c] = a.var[i + c]; }
    bool ok = valid_triples(u, v);
    if constexpr (A::kGuided) ok = ok && valid_features(a.gd, (size_t)y * a.g.w + x);
    if constexpr (A::kDemod) {
        double al[3];
        const bool oka = effective_albedo(a.dm, (size_t)y * a.g.w + x, al);
        ok = ok && oka;
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double al2 = al[c] * al[c];
                u[c] = u[c] / al[c];
                v[c] = v[c] / al2;
            }
        }
    }
    return ok;
}

// A thread's own pixel in registers: the feature values and variances of the channels in use (0 elsewhere). Every loop over groups and
// channels below runs to the caps with static indices, under wave-uniform conditions.
struct OwnFeatures {
    double g[kMaxChannels], s[kMaxChannels];
    __device__ __forceinline__ void load(const Guide &gd, size_t i) {
#pragma unroll
        for (int c = 0; c < kMaxChannels; c++) {
            g[c] = 0.0; s[c] = 0.0;
            if (gd.used >> c & 1u) { g[c] = gd.feat[c * gd.plane + i]; s[c] = gd.fvar[c * gd.plane + i]; }
        }
    }
    // D^f of the pair (own pixel, valid pixel iq)
    __device__ __forceinline__ double distance(const Guide &gd, size_t iq) const {
        double Df = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxGroups; j++) {
            if (j >= gd.groups) continue;
            double phi = 0.0;
#pragma unroll
            for (int c = 0; c < kMaxChannels; c++) {
                if (c < gd.first[j] || c >= gd.first[j] + gd.count[j]) continue;
                const double gq = gd.feat[c * gd.plane + iq], sq = gd.fvar[c * gd.plane + iq];
                const double d = g[c] - gq;
                phi += (d * d - gd.alpha_f * (s[c] + fmin(sq, s[c]))) / (gd.kf2 * fmax(gd.tau[j], s[c] + sq));
            }
            Df = fmax(Df, phi / (double)gd.count[j]);
        }
        return Df;
    }
};

// one term of a pixel's weighted sums: the triples u, v of p+o under the weight wgt. The one copy of these two expressions: the filtered
// film's sums and the companions' (nlm_joint.hip) both come from it, so equal inputs give equal bits.
__device__ __forceinline__ void add_term(double num[3], double vnum[3], double wgt, const double u[3], const double v[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) { num[c] += wgt * u[c]; vnum[c] += (wgt * wgt) * v[c]; }
}

struct Accum {
    double num[3] = {0.0, 0.0, 0.0}, vnum[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
    // Df (guided kernels): the pair's feature distance, >= 0. Returns the weight w_o(p).
    template <bool GUIDED = false>
    __device__ __forceinline__ double add(double S, int C, const double u[3], const double v[3], double Df = 0.0) {
        double D = S / (double)C;
        D = D > 0.0 ? D : 0.0;
        if (GUIDED) D = fmax(D, Df);
        const double wgt = exp(-D);
        wsum += wgt;
        add_term(num, vnum, wgt, u, v);
        return wgt;
    }
};

// the pixel's outputs and its terms of the film sums; u, v: its valid input triples (what load_pixel gave). A demodulated kernel
// multiplies the pixel's own a~ back and takes the sums' input terms from the original triples in global memory.
template <class A>
__device__ __forceinline__ void finish_pixel(const A &a, size_t i, const double u[3], const double v[3], const Accum &acc, Sums &s) {
    double o[3], vo[3];
    const double w2 = acc.wsum * acc.wsum;
    if constexpr (A::kDemod) {
        double al[3], uo[3], vi[3];
        effective_albedo(a.dm, i / 3, al);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double oc = acc.num[c] / acc.wsum, voc = acc.vnum[c] / w2, al2 = al[c] * al[c];
            o[c] = oc * al[c];
            vo[c] = voc * al2;
            a.out[i + c] = o[c];
            if (a.var_out) a.var_out[i + c] = vo[c];
            uo[c] = a.img[i + c]; vi[c] = a.var[i + c];
        }
        s.var_in += (vi[0] + vi[1]) + vi[2];
        s.sq_in += (uo[0] * uo[0] + uo[1] * uo[1]) + uo[2] * uo[2];
        s.var_out += (vo[0] + vo[1]) + vo[2];
        s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = acc.num[c] / acc.wsum;
        vo[c] = acc.vnum[c] / w2;
        a.out[i + c] = o[c];
        if (a.var_out) a.var_out[i + c] = vo[c];
    }
    s.var_in += (v[0] + v[1]) + v[2];
    s.sq_in += (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    s.var_out += (vo[0] + vo[1]) + vo[2];
    s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
}

} // namespace nlm
