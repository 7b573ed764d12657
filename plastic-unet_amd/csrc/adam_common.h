// What adam.hip (adam_kernel) and clip.hip (grad_sumsq_kernel, adam_clip_kernel) share: the tensor
// table of a launch, the per-element update and the host loop that cuts a tensor list into launches.
#pragma once

#include "common.h"

#include <math.h>

namespace pu {

constexpr int ADAM_MAX_T = 32;
constexpr int ADAM_CHUNK = 256 * 4 * 4;   // elements per block (256 threads x 4 float4)

struct AdamBatch {
    float* p[ADAM_MAX_T];
    const float* g[ADAM_MAX_T];
    float* m[ADAM_MAX_T];
    float* v[ADAM_MAX_T];
    long long n[ADAM_MAX_T];
    int block_start[ADAM_MAX_T + 1];
    int count;
};

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2,
                                          float eps, float wd, float step_size, float bc2s) {
#pragma clang fp contract(off)
    if (wd != 0.f) g = g + wd * p;
    // ATen lerp (weight < 0.5): self + weight * (end - self)
    m = m + omb1 * (g - m);
    v = v * b2 + omb2 * g * g;
    const float denom = sqrtf(v) / bc2s + eps;
    p = p + (-step_size) * (m / denom);
    return p;
}

// The whole list is checked before the first launch: a bad tensor past the first 32 must not leave
// the ones before it stepped.  grad_only: the entry reads `grad` and `numel` alone.
inline int adam_check_list(const char* what, const pu_adam_tensor* tensors, int n_tensors, bool grad_only) {
    PU_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors), "%s: bad tensor list", what);
    for (int k = 0; k < n_tensors; ++k) {
        const pu_adam_tensor& t = tensors[k];
        PU_REQUIRE(t.numel >= 0, "%s: tensor %d", what, k);
        PU_REQUIRE(t.numel == 0 || (t.grad && (grad_only || (t.param && t.exp_avg && t.exp_avg_sq))), "%s: tensor %d",
                   what, k);
    }
    return PU_OK;
}

// launch(batch, blocks) once per 32 non-empty tensors, one block per ADAM_CHUNK elements of a tensor
template <typename Launch>
inline int adam_for_each_launch(const char* what, const pu_adam_tensor* tensors, int n_tensors, Launch&& launch) {
    int i = 0;
    while (i < n_tensors) {
        AdamBatch b;
        b.count = 0;
        int blocks = 0;
        while (i < n_tensors && b.count < ADAM_MAX_T) {
            const pu_adam_tensor& t = tensors[i++];
            if (t.numel == 0) continue;     // an empty tensor has no storage: its pointers are null (torch)
            b.p[b.count] = t.param; b.g[b.count] = t.grad; b.m[b.count] = t.exp_avg; b.v[b.count] = t.exp_avg_sq;
            b.n[b.count] = t.numel;
            b.block_start[b.count] = blocks;
            blocks += (int)((t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
            b.count++;
        }
        b.block_start[b.count] = blocks;
        if (b.count == 0) continue;
        launch(b, blocks);
        int st = check_launch(what);
        if (st != PU_OK) return st;
    }
    return PU_OK;
}

}  // namespace pu
