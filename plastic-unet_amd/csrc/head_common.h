// What the plastic head's kernels (head_fwd.h, head_bwd.h, both included by plastic.hip) share: the
// tile constants and one copy of every expression that two kernels must evaluate to the same bits.
#pragma once

#include "common.h"

#include <math.h>

namespace pu {

constexpr int HK = 16;   // k chunk the VALU GEMMs stage through LDS

// The VALU GEMMs (head_fwd_kernel, head_dx_kernel, head_dw_kernel) compute a T x T tile per
// 256-thread block, a T/16 x T/16 micro-tile per thread (T = 64: 4x4; T = 32: 2x2, for grids that
// would not fill the chip, e.g. bs 32 x 128^2 -> 512 blocks instead of 128).

__device__ __forceinline__ float sigmoid(float a) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-a));
}

__device__ __forceinline__ float trace_rule(float h, float x0, float y0, float eta, float one_m_eta, int rule) {
#pragma clang fp contract(off)
    // unet_p.py:82 (Hebb) and :84 (Oja), in the reference's operation order
    return rule == PU_RULE_HEBB ? one_m_eta * h + eta * (x0 * y0) : h + eta * ((x0 - h * y0) * y0);
}

// G = dy * (1 - y) * y   (ATen sigmoid_backward: grad * (1 - out) * out)
__device__ __forceinline__ float sig_bwd(float dy, float y) {
#pragma clang fp contract(off)
    return dy * (1.f - y) * y;
}

// one k step of a thread's M x M micro-tile: acc[q][r] += a[q] * b[r]
template <int M>
__device__ __forceinline__ void tile_fma(float (&acc)[M][M], const float (&a)[M], const float (&b)[M]) {
#pragma unroll
    for (int q = 0; q < M; ++q)
#pragma unroll
        for (int r = 0; r < M; ++r) acc[q][r] = fmaf(a[q], b[r], acc[q][r]);
}

// dY[o] as the backward GEMMs read it.  EX (the trace backward's extras, pu_plastic_bwd_trace): dY
// may be null (zeros), and dy0[r0] is added where the element lies in row 0 of its slot.
template <bool EX>
__device__ __forceinline__ float load_dy(const float* __restrict__ dY, const float* __restrict__ dy0, long long o,
                                         bool row0, long long r0) {
#pragma clang fp contract(off)
    if constexpr (EX) {
        float v = dY ? dY[o] : 0.f;
        if (row0) v += dy0[r0];
        return v;
    } else {
        return dY[o];
    }
}

}  // namespace pu
