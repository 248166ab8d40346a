// image_kernels.hip — the home of the one kernel image_kernels.h declares a launch for.
#include "image_kernels.h"

namespace film {

// one block: three runs of nb block partials, each reduced in the fixed order of image_kernels.h
__global__ __launch_bounds__(kBlock) void finish_kernel(int nb, const double *partials, Estimate *est) {
    __shared__ double red[kBlock / 64];
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = reduce_partials(partials + k * nb, nb, red);
    if (threadIdx.x == 0) { est->sum_var = r[0]; est->sum_mean2 = r[1]; est->left_out = r[2]; }
}

void launch_finish(int nb, const double *partials, Estimate *est, hipStream_t stream) {
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, stream, nb, partials, est);
}

// one block: `runs` runs of nb block partials, each reduced in the fixed order of image_kernels.h
__global__ __launch_bounds__(kBlock) void finish_runs_kernel(int nb, int runs, const double *partials, double *sums) {
    __shared__ double red[kBlock / 64];
    for (int k = 0; k < runs; k++) {
        const double r = reduce_partials(partials + (size_t)k * nb, nb, red);
        if (threadIdx.x == 0) sums[k] = r;
    }
}

void launch_finish_runs(int nb, int runs, const double *partials, double *sums, hipStream_t stream) {
    hipLaunchKernelGGL(finish_runs_kernel, dim3(1), dim3(kBlock), 0, stream, nb, runs, partials, sums);
}

} // namespace film
