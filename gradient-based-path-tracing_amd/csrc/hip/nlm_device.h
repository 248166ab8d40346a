// nlm_device.h — the device code the non-local-means family shares (denoise_nlm.hip, nlm_joint.hip, nlm_regress.hip, nlm_collab.hip;
// denoise_atrous.hip takes the pixel helpers): the tile constants, the argument blocks, the guide's and the divisor's blocks, a pixel's
// validity and loading, the pair distance and the pair weight, the direct form's tap loop (patch_distance), the tiled form's LDS stage
// with its loop over the window offsets (Stage), the thread's own features, a pixel's weighted sums (Accum, finish_pixel) and the film
// sums. `A` is a kernel's argument block: the fields of nlm::Args, kGuided / kDemod, and with them `gd` / `dm`.
#pragma once
#include "../../../include/gdpt.h"
#include "image_kernels.h"
#include "denoise_nlm.h"

#include <type_traits>

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

// the argument block of a kernel; the guided and demodulated ones add their blocks
struct Args {
    static constexpr bool kGuided = false, kDemod = false;
    TileGrid g;                  // 16 x 16 tiles
    int r, f;
    double k2, alpha, eps;
    const double *img, *var;
    double *out, *var_out;       // var_out nullable
    double *partials;            // [0] sum var in, [1] sum u^2 in, [2] pixels left out, [3] sum var out, [4] sum u^2 out, [5] = [2]; gridDim.x doubles each
};
struct GuidedArgs : Args {
    static constexpr bool kGuided = true;
    Guide gd;
};
struct DemodArgs : Args {
    static constexpr bool kDemod = true;
    Demod dm;
};
struct GuidedDemodArgs : GuidedArgs {
    static constexpr bool kDemod = true;
    Demod dm;
};
template <bool GUIDED, bool DEMOD>
using ArgsOf = typename std::conditional<GUIDED, typename std::conditional<DEMOD, GuidedDemodArgs, GuidedArgs>::type,
                                         typename std::conditional<DEMOD, DemodArgs, Args>::type>::type;

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
// a finished pixel's terms of the film sums: its input triples u, v and its outputs o, vo
__device__ __forceinline__ void add_sums(Sums &s, const double u[3], const double v[3], const double o[3], const double vo[3]) {
    s.var_in += (v[0] + v[1]) + v[2];
    s.sq_in += (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    s.var_out += (vo[0] + vo[1]) + vo[2];
    s.sq_out += (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
}

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

// direct form: S_o, C_o of the valid pair (x, y), (x + ox, y + oy), tap by tap from global memory; load(x, y, u, v) is the kernel's
// pixel loader
template <class A, class Load>
__device__ __forceinline__ void patch_distance(const A &a, Load load, int x, int y, int ox, int oy, double &S, int &C) {
    const int f = a.f;
    S = 0.0; C = 0;
    for (int ny = -f; ny <= f; ny++)
        for (int nx = -f; nx <= f; nx++) {
            const int ax = x + nx, ay = y + ny, bx = ax + ox, by = ay + oy;
            if (ax < 0 || ay < 0 || ax >= a.g.w || ay >= a.g.h || bx < 0 || by < 0 || bx >= a.g.w || by >= a.g.h) continue;
            double ua[3], va[3], ub[3], vb[3];
            const bool oka = load(ax, ay, ua, va), okb = load(bx, by, ub, vb);
            if (!oka || !okb) continue;
            S += pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
            C++;
        }
}

// The tiled form's stage: the tile with a halo of r + f pixels in LDS, plane by plane (three u, three v, a validity flag; out-of-film
// and invalid entries are u = v = 0, flag 0), sized by the call's r and f: (16 + 2(r+f))^2 entries of 52 bytes, 42 x 42 = 91.7 KB at
// r = 10, f = 3 (108 624 bytes with the planes below). Per window offset: e_o and its count on the (16 + 2f)^2 points the tile's
// patches touch, into LDS; row sums of 2f + 1 taps; column sums of the row sums (the separable box of box_kernel, recon_spread.hip).
// (16 + 2f)^2 pair distances per offset and tile instead of 256 (2f+1)^2: 484 against 12544 at f = 3.
// LDS banking: every plane is a plane of doubles or of ints, so consecutive lanes read consecutive elements. In the row pass a
// half-wave covers two rows of 16 outputs; the e plane's pitch is 16 (f = 0) or 48 doubles, = 16 mod 32, which puts the second row's
// 16 doubles on the other half of the 64 banks. In the column pass a half-wave reads 32 consecutive doubles of the row sums (pitch 16).
struct Stage {
    int r, f, sw, sn, ew, ep, taps, tid, pc;
    double *su, *sv, *pe, *ph;
    int *sflag, *ce, *ch;
    int ia[2], ie[2], jrow[2];

    // the stage of a call's r and f in the block's dynamic LDS (lds_doubles, lds_ints)
    __device__ __forceinline__ void lay_out(int r_, int f_, double *lds) {
        r = r_; f = f_;
        const int halo = r + f;
        sw = kTile + 2 * halo; sn = sw * sw;           // the stage: the tile and its halo
        ew = kTile + 2 * f;                            // the points the tile's patches touch, a row
        const int en = ew * ew;
        ep = e_pitch(f); taps = 2 * f + 1;
        su = lds; sv = lds + 3 * sn;                   // plane c at su + c sn, sv + c sn
        pe = lds + 6 * sn;                             // e_o of the current offset, pitch ep
        ph = pe + ep * ew;                             // its row sums, pitch 16
        sflag = (int *)(ph + kTile * ew);
        ce = sflag + sn; ch = ce + ep * ew;
        tid = threadIdx.x;
        const int lx = tid & (kTile - 1), ly = tid / kTile;
        // the (at most two) pair distances and row sums of an offset that fall to this thread
        for (int k = 0; k < 2; k++) {
            const int q = tid + k * kBlock;
            const int qy = q / ew, qx = q - qy * ew;
            ia[k] = q < en ? (qy + r) * sw + qx + r : -1;
            ie[k] = qy * ep + qx;
            jrow[k] = q < kTile * ew ? (q / kTile) * ep + (q & (kTile - 1)) : -1;
        }
        pc = (ly + halo) * sw + lx + halo;             // the thread's own pixel in the stage
    }

    // the tile at (x0, y0) with its halo into the stage, through the kernel's pixel loader load(x, y, u, v); the caller's barriers
    // stand before (the previous tile's stage has been read) and after
    template <class Load>
    __device__ __forceinline__ void fill(const TileGrid &g, int x0, int y0, Load load) const {
        const int halo = r + f;
        for (int k = tid; k < sn; k += kBlock) {
            const int ry = k / sw, rx = k - ry * sw;
            const int gx = x0 - halo + rx, gy = y0 - halo + ry;
            double u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
            bool ok = false;
            if (gx >= 0 && gy >= 0 && gx < g.w && gy < g.h) ok = load(gx, gy, u, v);
#pragma unroll
            for (int c = 0; c < 3; c++) { su[c * sn + k] = ok ? u[c] : 0.0; sv[c * sn + k] = ok ? v[c] : 0.0; }
            sflag[k] = ok ? 1 : 0;
        }
    }

    // the staged triples of entry i
    __device__ __forceinline__ void mean(int i, double u[3]) const { u[0] = su[i]; u[1] = su[sn + i]; u[2] = su[2 * sn + i]; }
    __device__ __forceinline__ void variance(int i, double v[3]) const { v[0] = sv[i]; v[1] = sv[sn + i]; v[2] = sv[2 * sn + i]; }

    // The loop over the window offsets: tap(iq, S, C, oy, ox) is called for the thread's own pixel p (`ok`: whether it is valid) and
    // every valid partner q = p + o, with the partner's index iq in the stage and S_o, C_o of the pair. FROM_PARTNER swaps the roles
    // of an offset's two pixels: S and C are those of the fit centred at q for its offset -o, that is the pair distances
    // e(q + n, p + n) with q's triple first, over the same patch taps n and summed in the same separable order.
    template <bool FROM_PARTNER = false, class Tap>
    __device__ __forceinline__ void sweep(double k2, double alpha, double eps, bool ok, Tap tap) const {
        for (int oy = -r; oy <= r; oy++)
            for (int ox = -r; ox <= r; ox++) {
                const int shift = oy * sw + ox;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (ia[k] < 0) continue;
                    const int i0 = ia[k], i1 = i0 + shift;
                    const int both = sflag[i0] & sflag[i1];
                    double e = 0.0;
                    if (both) {
                        const int ja = FROM_PARTNER ? i1 : i0, jb = FROM_PARTNER ? i0 : i1;
                        double ua[3], va[3], ub[3], vb[3];
#pragma unroll
                        for (int c = 0; c < 3; c++) { ua[c] = su[c * sn + ja]; va[c] = sv[c * sn + ja]; ub[c] = su[c * sn + jb]; vb[c] = sv[c * sn + jb]; }
                        e = pair_distance(ua, va, ub, vb, k2, alpha, eps);
                    }
                    pe[ie[k]] = e; ce[ie[k]] = both;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (jrow[k] < 0) continue;
                    double S = 0.0;
                    int C = 0;
                    for (int n = 0; n < taps; n++) { S += pe[jrow[k] + n]; C += ce[jrow[k] + n]; }
                    ph[tid + k * kBlock] = S; ch[tid + k * kBlock] = C;
                }
                __syncthreads();
                const int iq = pc + shift;
                if (ok && sflag[iq] != 0) {            // (a set flag: p + o is inside the film)
                    double S = 0.0;
                    int C = 0;
                    for (int n = 0; n < taps; n++) { S += ph[tid + n * kTile]; C += ch[tid + n * kTile]; }
                    tap(iq, S, C, oy, ox);
                }
            }
    }
};

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

// w_o(p) of a valid pair with C >= 1; Df (guided kernels): the pair's feature distance, >= 0
template <bool GUIDED = true>
__device__ __forceinline__ double pair_weight(double S, int C, double Df) {
    double D = S / (double)C;
    D = D > 0.0 ? D : 0.0;
    if (GUIDED) D = fmax(D, Df);
    return exp(-D);
}

struct Accum {
    double num[3] = {0.0, 0.0, 0.0}, vnum[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
    // Returns the weight w_o(p).
    template <bool GUIDED = false>
    __device__ __forceinline__ double add(double S, int C, const double u[3], const double v[3], double Df = 0.0) {
        const double wgt = pair_weight<GUIDED>(S, C, Df);
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
        add_sums(s, uo, vi, o, vo);
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[c] = acc.num[c] / acc.wsum;
        vo[c] = acc.vnum[c] / w2;
        a.out[i + c] = o[c];
        if (a.var_out) a.var_out[i + c] = vo[c];
    }
    add_sums(s, u, v, o, vo);
}

} // namespace nlm
