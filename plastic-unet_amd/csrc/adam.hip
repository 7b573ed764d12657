// Multi-tensor Adam: one launch for every parameter tensor of the model.
//
// Replaces torch.optim.Adam(net.parameters(), lr).step() (yaricom/Plastic-UNet src/train.py:66,111),
// whose single-tensor update is, per element (amsgrad=False, maximize=False):
//   g += wd * p (if weight_decay) ; m = lerp(m, g, 1-beta1) ; v = v*beta2 + (1-beta2)*g*g
//   p = p - step_size * m / (sqrt(v)/bc2_sqrt + eps),  step_size = lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t)
// HBM-bound: 4 reads + 3 writes of 4 bytes per element, float4 per lane.
#include "adam_common.h"

namespace pu {

__global__ __launch_bounds__(256) void adam_kernel(const AdamBatch batch, float omb1, float b2, float omb2, float eps, float wd,
                                                   float step_size, float bc2s) {
    // locate this block's tensor (count <= 32: linear scan of the prefix table)
    int t = 0;
    while (t + 1 < batch.count && (int)blockIdx.x >= batch.block_start[t + 1]) ++t;
    const long long n = batch.n[t];
    const long long base = (long long)(blockIdx.x - batch.block_start[t]) * ADAM_CHUNK;
    float* P = batch.p[t];
    const float* G = batch.g[t];
    float* M = batch.m[t];
    float* V = batch.v[t];
    const bool aligned = ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const long long i = base + ((long long)it * 256 + threadIdx.x) * 4;
        if (i >= n) break;
        if (aligned && i + 3 < n) {
            f32x4 p = *reinterpret_cast<f32x4*>(P + i);
            f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
            f32x4 m = *reinterpret_cast<f32x4*>(M + i);
            f32x4 v = *reinterpret_cast<f32x4*>(V + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam_one(pe, g[e], me, ve, omb1, b2, omb2, eps, wd, step_size, bc2s);
                p[e] = pe; m[e] = me; v[e] = ve;
            }
            *reinterpret_cast<f32x4*>(P + i) = p;
            *reinterpret_cast<f32x4*>(M + i) = m;
            *reinterpret_cast<f32x4*>(V + i) = v;
        } else {
            for (long long e = i; e < i + 4 && e < n; ++e) adam_one(P[e], G[e], M[e], V[e], omb1, b2, omb2, eps, wd, step_size, bc2s);
        }
    }
}

}  // namespace pu

using namespace pu;

extern "C" int pu_adam_multi(const pu_adam_tensor* tensors, int n_tensors, double beta1, double beta2, double eps,
                             double weight_decay, double step_size, double bc2_sqrt, void* stream) {
    int st = adam_check_list("pu_adam_multi", tensors, n_tensors, false);
    if (st != PU_OK) return st;
    return adam_for_each_launch("pu_adam_multi", tensors, n_tensors, [&](const AdamBatch& b, int blocks) {
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), b, (float)(1.0 - beta1),
                           (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)step_size,
                           (float)bc2_sqrt);
    });
}
