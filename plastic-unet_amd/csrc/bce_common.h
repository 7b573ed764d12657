// What plastic.hip (bce_partial_kernel, bce_final_kernel) and metrics.hip (seg_metrics_partial_kernel,
// seg_metrics_finish_kernel) share: the element expression of nn.BCELoss, the grid of a sum over n
// elements and the finish (over common.h's block_tree256).  One copy of each, so the mean BCE of a
// sample has the same bits whichever entry point computes it.
#pragma once

#include "common.h"

#include <math.h>

namespace pu {

constexpr int BCE_BLOCKS = 512;

// blocks of 256 threads of a grid-stride sum over n elements: ceil(n / 256), at most BCE_BLOCKS
inline int bce_grid(long long n) {
    long long g = (n + 255) / 256;
    if (g > BCE_BLOCKS) g = BCE_BLOCKS;
    if (g < 1) g = 1;
    return (int)g;
}

// ATen: (t - 1) * max(log1p(-y), -100) - t * max(log(y), -100)
__device__ __forceinline__ float bce_element(float yy, float tt) {
#pragma clang fp contract(off)
    return (tt - 1.f) * fmaxf(log1pf(-yy), -100.f) - tt * fmaxf(logf(yy), -100.f);
}

// the np block partials -> the mean over n, valid in thread 0 of the one block that calls it
__device__ __forceinline__ float bce_finish(const double* __restrict__ partial, int np, long long n) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += partial[i];
    return (float)(block_tree256(s) / (double)n);
}

}  // namespace pu
