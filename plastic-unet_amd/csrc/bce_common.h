// What plastic.hip (bce_partial_kernel, bce_final_kernel) and metrics.hip (seg_metrics_partial_kernel,
// seg_metrics_finish_kernel) share: the element expression of nn.BCELoss, the grid of a sum over n
// elements, the 256-wide fp64 tree and the finish.  One copy of each, so the mean BCE of a sample has
// the same bits whichever entry point computes it.
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

// sum over the block's 256 threads by a halving tree through LDS, valid in thread 0; every thread of
// the block calls it
__device__ __forceinline__ double bce_block_tree(double s) {
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// the np block partials -> the mean over n, valid in thread 0 of the one block that calls it
__device__ __forceinline__ float bce_finish(const double* __restrict__ partial, int np, long long n) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += partial[i];
    return (float)(bce_block_tree(s) / (double)n);
}

}  // namespace pu
