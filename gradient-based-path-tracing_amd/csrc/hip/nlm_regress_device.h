// nlm_regress_device.h — the device code the first-order regression (nlm_regress.hip) and its collaborative form (nlm_collab.hip) share
// beside nlm_device.h: the kernels' argument block, the regressors and a pair's design vector, the normal equations of a pixel (Fit) and
// their LDL^T in the header's order (include/gdpt.h: gdpt_denoise_nlm_regress*).
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
// a regression kernel is a guided, not demodulated kernel to the helpers of nlm_device.h; gd.used: the channels some group or some
// regressor names
struct Args : GuidedArgs {
    int second;                  // whether the second sweep runs (var_out or the sums are asked for)
    Regress rg;
};

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

} // namespace nlmr
