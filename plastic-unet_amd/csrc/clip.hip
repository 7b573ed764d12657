// Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, norm_type 2), on the device and
// folded into the Adam step:
//   grad_sumsq_kernel        sum of squares of every 4096-element chunk of every gradient, in fp64
//   grad_norm_finish_kernel  the chunk sums -> out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6))
//   adam_clip_kernel         adam_kernel on g * out[1]; the gradients are read, never written
// Every sum has one fixed order (per thread in element order, a fixed shuffle tree per wave, the four
// waves in wave order, the chunks in index order) and no atomics, so the norm has the same bits on
// every call, at every pointer alignment and on every rank that holds the same gradients.
// HBM-bound: 4 B per element for the norm (+ 8 B per chunk of partials), 28 B per element for Adam.
#include "adam_common.h"

namespace pu {

// adam_kernel's block mapping: the block of a launch -> its tensor (count <= 32: linear scan of the
// prefix table) and the first element of its chunk
__device__ __forceinline__ int adam_locate(const int* block_start, int count, long long* base) {
    int t = 0;
    while (t + 1 < count && (int)blockIdx.x >= block_start[t + 1]) ++t;
    *base = (long long)(blockIdx.x - block_start[t]) * ADAM_CHUNK;
    return t;
}

// sum over the block's 256 threads, valid in thread 0: lanes by a fixed shuffle tree, then the four
// waves through LDS in wave order
__device__ __forceinline__ double block_sum_fixed(double s) {
    __shared__ double wave_sum[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// One block per chunk, as adam_kernel; thread t owns elements base + (it*256 + t)*4 .. +3, it = 0..3,
// and adds their squares (exact in fp64) in element order - the same on the float4 and the scalar path.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamBatch batch, double* __restrict__ partials) {
    long long base;
    const int t = adam_locate(batch.block_start, batch.count, &base);
    const long long n = batch.n[t];
    const float* G = batch.g[t];
    const bool aligned = (((uintptr_t)G) & 15) == 0;
    double s = 0.0;
    if (aligned && base + ADAM_CHUNK <= n) {
        // a whole aligned chunk (all but a tensor's last): the four loads in flight together, then
        // the same adds in the same order
        f32x4 g[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) g[it] = *reinterpret_cast<const f32x4*>(G + base + (it * 256 + (int)threadIdx.x) * 4);
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += (double)g[it][e] * (double)g[it][e];
    } else {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long long i = base + ((long long)it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            if (aligned && i + 3 < n) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += (double)g[e] * (double)g[e];
            } else {
                for (long long e = i; e < i + 4 && e < n; ++e) s += (double)G[e] * (double)G[e];
            }
        }
    }
    s = block_sum_fixed(s);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, long long n_partials,
                                                               float max_norm, float* __restrict__ out) {
#pragma clang fp contract(off)
    // thread t adds partials[t], partials[t + 256], ... in index order; eight loads in flight at a time
    // (the one block would otherwise wait out one L2 round trip per partial)
    double s = 0.0;
    long long i = threadIdx.x;
    for (; i + 7 * 256 < n_partials; i += 8 * 256) {
        double p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = partials[i + k * 256];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += p[k];
    }
    for (; i < n_partials; i += 256) s += partials[i];
    s = block_sum_fixed(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0).  The comparison, not fminf: a NaN
        // norm must give a NaN coefficient.
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;
    }
}

// one fp32 rounding of its own: with contraction off the product cannot fuse into adam_one's first operation
__device__ __forceinline__ float scaled_grad(float g, float scale) {
#pragma clang fp contract(off)
    return g * scale;
}

__global__ __launch_bounds__(256) void adam_clip_kernel(const AdamBatch batch, float omb1, float b2, float omb2, float eps,
                                                        float wd, float step_size, float bc2s,
                                                        const float* __restrict__ grad_scale) {
    long long base;
    const int t = adam_locate(batch.block_start, batch.count, &base);
    const long long n = batch.n[t];
    float* P = batch.p[t];
    const float* G = batch.g[t];
    float* M = batch.m[t];
    float* V = batch.v[t];
    const float scale = grad_scale[0];
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
                adam_one(pe, scaled_grad(g[e], scale), me, ve, omb1, b2, omb2, eps, wd, step_size, bc2s);
                p[e] = pe; m[e] = me; v[e] = ve;
            }
            *reinterpret_cast<f32x4*>(P + i) = p;
            *reinterpret_cast<f32x4*>(M + i) = m;
            *reinterpret_cast<f32x4*>(V + i) = v;
        } else {
            for (long long e = i; e < i + 4 && e < n; ++e)
                adam_one(P[e], scaled_grad(G[e], scale), M[e], V[e], omb1, b2, omb2, eps, wd, step_size, bc2s);
        }
    }
}

static long long grad_norm_chunks(const pu_adam_tensor* tensors, int n_tensors) {
    long long chunks = 0;
    for (int k = 0; k < n_tensors; ++k)
        if (tensors[k].numel > 0) chunks += (tensors[k].numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return chunks;
}

}  // namespace pu

using namespace pu;

extern "C" size_t pu_grad_norm_workspace_bytes(const pu_adam_tensor* tensors, int n_tensors) {
    const long long chunks = tensors && n_tensors > 0 ? grad_norm_chunks(tensors, n_tensors) : 0;
    return sizeof(double) * (size_t)(chunks > 1 ? chunks : 1);
}

extern "C" int pu_grad_norm(const pu_adam_tensor* tensors, int n_tensors, double max_norm, float* out2, void* ws,
                            size_t ws_bytes, void* stream) {
    int st = adam_check_list("pu_grad_norm", tensors, n_tensors, true);
    if (st != PU_OK) return st;
    PU_REQUIRE(max_norm > 0.0, "pu_grad_norm: max_norm %g (must be > 0; +inf measures without clipping)", max_norm);
    PU_REQUIRE(out2, "pu_grad_norm: out2 is null");
    PU_REQUIRE(ws && (((uintptr_t)ws) & 7) == 0 && ws_bytes >= pu_grad_norm_workspace_bytes(tensors, n_tensors),
               "pu_grad_norm: workspace of %zu bytes at %p, needs %zu, 8-byte aligned", ws_bytes, ws,
               pu_grad_norm_workspace_bytes(tensors, n_tensors));
    double* partials = static_cast<double*>(ws);
    long long first = 0;        // the first chunk of the launch in the list's chunk order
    st = adam_for_each_launch("pu_grad_norm", tensors, n_tensors, [&](const AdamBatch& b, int blocks) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), b, partials + first);
        first += blocks;
    });
    if (st != PU_OK) return st;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, first,
                       (float)max_norm, out2);
    return check_launch("pu_grad_norm");
}

extern "C" int pu_adam_multi_clipped(const pu_adam_tensor* tensors, int n_tensors, double beta1, double beta2, double eps,
                                     double weight_decay, double step_size, double bc2_sqrt, const float* grad_scale,
                                     void* stream) {
    int st = adam_check_list("pu_adam_multi_clipped", tensors, n_tensors, false);
    if (st != PU_OK) return st;
    PU_REQUIRE(grad_scale, "pu_adam_multi_clipped: grad_scale is null");
    return adam_for_each_launch("pu_adam_multi_clipped", tensors, n_tensors, [&](const AdamBatch& b, int blocks) {
        hipLaunchKernelGGL(adam_clip_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), b, (float)(1.0 - beta1),
                           (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)step_size,
                           (float)bc2_sqrt, grad_scale);
    });
}
