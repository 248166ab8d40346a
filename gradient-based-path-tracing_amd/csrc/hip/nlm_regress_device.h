// nlm_regress_device.h — the device code the first-order regression (nlm_regress.hip) and its collaborative form (nlm_collab.hip) share:
// the kernels' argument block, the regressors and a pair's design vector, the pair weight, the normal equations of a pixel (Fit), their
// LDL^T in the header's order (include/gdpt.h: gdpt_denoise_nlm_regress*), the direct form's patch distance and the tiled form's stage
// with its loop over the window offsets. Moved here from nlm_regress.hip as it stood: the regression kernels' machine code is what it
// was before the move.
#pragma once
#include "../../../include/gdpt.h"
#include "image_kernels.h"
#include "denoise_nlm.h"
#include "nlm_device.h"

namespace nlmr {

using namespace nlm;              // nlm_device.h; and film's kBlock, TileGrid, leave_block_sum through it

constexpr int kMaxM = GDPT_NLM_MAX_REGRESSORS, kD = 1 + kMaxM, kTri = kD * (kD + 1) / 2;

// the regressors: planes ch[0 .. m) of the guide's, divided by scale[]
struct Regress {
    int m, ch[kMaxM];
    double scale[kMaxM], ridge;
};
struct Args {
    static constexpr bool kGuided = true, kDemod = false;
    TileGrid g;                  // 16 x 16 tiles
    int r, f;
    double k2, alpha, eps;
    const double *img, *var;
    double *out, *var_out;       // var_out nullable
    double *partials;            // as denoise_nlm.hip's: six sums, gridDim.x doubles each
    int second;                  // whether the second sweep runs (var_out or the sums are asked for)
    Guide gd;                    // `used`: the channels some group or some regressor names
    Regress rg;
};

// w_o(p) of a valid pair with C >= 1; Df: the pair's feature distance, >= 0
__device__ __forceinline__ double pair_weight(double S, int C, double Df) {
    double D = S / (double)C;
    D = D > 0.0 ? D : 0.0;
    D = fmax(D, Df);
    return exp(-D);
}

// The thread's own regressor values, and the design vector of a pair. Unused regressors (j >= m) have z = 0.
struct OwnRegressors {
    double g[kMaxM];
    __device__ __forceinline__ void load(const Regress &rg, const Guide &gd, size_t i) {
#pragma unroll
        for (int j = 0; j < kMaxM; j++) g[j] = j < rg.m ? gd.feat[rg.ch[j] * gd.plane + i] : 0.0;
    }
    // z(p, o) for the valid pixel iq = p + o
    __device__ __forceinline__ void design(const Regress &rg, const Guide &gd, size_t iq, double z[kD]) const {
        z[0] = 1.0;
#pragma unroll
        for (int j = 0; j < kMaxM; j++) {
            z[j + 1] = 0.0;
            if (j < rg.m) {
                const double d = gd.feat[rg.ch[j] * gd.plane + iq] - g[j];
                z[j + 1] = rg.scale[j] == 1.0 ? d : d / rg.scale[j];      // (d / 1.0 is d: the division is skipped, not changed)
            }
        }
    }
};

__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // i >= j

// The normal equations of one pixel: the lower triangle of A, packed by rows, and the three right-hand sides.
struct Fit {
    double A[kTri], b[3][kD];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < kTri; k++) A[k] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int i = 0; i < kD; i++) b[c][i] = 0.0;
    }
    __device__ __forceinline__ void add(double w, const double z[kD], const double u[3]) {
#pragma unroll
        for (int i = 0; i < kD; i++) {
            const double wz = w * z[i];
#pragma unroll
            for (int j = 0; j <= i; j++) A[tri(i, j)] += wz * z[j];
#pragma unroll
            for (int c = 0; c < 3; c++) b[c][i] += wz * u[c];
        }
    }
};

// L (unit lower triangle, packed as A) and D of A = L D L^T, in the header's order; A's ridge has been added
struct Ldlt {
    double L[kTri], D[kD];
    __device__ __forceinline__ void factor(const double A[kTri]) {
#pragma unroll
        for (int j = 0; j < kD; j++) {
            double t[kD];
#pragma unroll
            for (int k = 0; k < j; k++) t[k] = L[tri(j, k)] * D[k];
            double dj = A[tri(j, j)];
#pragma unroll
            for (int k = 0; k < j; k++) dj -= L[tri(j, k)] * t[k];
            D[j] = dj;
#pragma unroll
            for (int i = j + 1; i < kD; i++) {
                double s = A[tri(i, j)];
#pragma unroll
                for (int k = 0; k < j; k++) s -= L[tri(i, k)] * t[k];
                L[tri(i, j)] = s / dj;
            }
        }
    }
    // x: the right-hand side in, the solution out
    __device__ __forceinline__ void solve(double x[kD]) const {
#pragma unroll
        for (int i = 0; i < kD; i++)
#pragma unroll
            for (int k = 0; k < i; k++) x[i] -= L[tri(i, k)] * x[k];
#pragma unroll
        for (int i = 0; i < kD; i++) x[i] = x[i] / D[i];
#pragma unroll
        for (int i = kD - 1; i >= 0; i--)
#pragma unroll
            for (int k = i + 1; k < kD; k++) x[i] -= L[tri(k, i)] * x[k];
    }
};

// direct form: S_o, C_o of the valid pair (x, y), (x + ox, y + oy), tap by tap from global memory
__device__ __forceinline__ void patch_distance(const Args &a, int x, int y, int ox, int oy, double &S, int &C) {
    const int f = a.f;
    S = 0.0; C = 0;
    for (int ny = -f; ny <= f; ny++)
        for (int nx = -f; nx <= f; nx++) {
            const int ax = x + nx, ay = y + ny, bx = ax + ox, by = ay + oy;
            if (ax < 0 || ay < 0 || ax >= a.g.w || ay >= a.g.h || bx < 0 || by < 0 || bx >= a.g.w || by >= a.g.h) continue;
            double ua[3], va[3], ub[3], vb[3];
            const bool oka = load_pixel(a, ax, ay, ua, va), okb = load_pixel(a, bx, by, ub, vb);
            if (!oka || !okb) continue;
            S += pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
            C++;
        }
}

// The tiled form's stage and its loop over the window offsets, which both sweeps run: tap(iq, S, C, oy, ox) is called for the
// thread's own pixel and every valid partner p + o, with the partner's index iq in the stage.
struct Stage {
    int r, f, sw, sn, ew, ep, taps, tid, pc;
    double *su, *sv, *pe, *ph;
    int *sflag, *ce, *ch;
    int ia[2], ie[2], jrow[2];

    template <class Tap>
    __device__ __forceinline__ void sweep(const Args &a, bool okp, Tap tap) const {
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
                        double ua[3], va[3], ub[3], vb[3];
#pragma unroll
                        for (int c = 0; c < 3; c++) { ua[c] = su[c * sn + i0]; va[c] = sv[c * sn + i0]; ub[c] = su[c * sn + i1]; vb[c] = sv[c * sn + i1]; }
                        e = pair_distance(ua, va, ub, vb, a.k2, a.alpha, a.eps);
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
                if (okp && sflag[iq] != 0) {
                    double S = 0.0;
                    int C = 0;
                    for (int n = 0; n < taps; n++) { S += ph[tid + n * kTile]; C += ch[tid + n * kTile]; }
                    tap(iq, S, C, oy, ox);
                }
            }
    }
};

} // namespace nlmr
