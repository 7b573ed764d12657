// Phase 2 of every weight gradient: the fixed-order fp64 reductions of the split partials.
// Part of wgrad.hip, which includes it once, after its parameter block and shared helpers.
#pragma once

namespace pu {

// ------------------------------------------------------------------ phase 2: the split reduction
// Every slab row is Kcp = ceil4(Kc) floats (plan_dims), so the reduction works on quads of 4
// consecutive entries of one row.
//
// The one summation order of phase 2.  `count` partials, `stride` elements of V apart, go into 4
// fp64 chains: partial i to chain i & 3 while i < 4 * (count / 4), the remainder to chain 0; the
// result is (s0 + s1) + (s2 + s3).  V is float, double or a quad of either (summed per
// component).  DEPTH (4 or 8) is only how many loads are issued before their adds: 8 takes two
// chain rounds at once, then one round of 4 if it is left - the same order, so every kernel below
// gives the same bits for the same sequence of partials.
typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double widen(float v) { return (double)v; }
__device__ __forceinline__ double widen(double v) { return v; }
__device__ __forceinline__ f64x4 widen(f32x4 v) { return __builtin_convertvector(v, f64x4); }
__device__ __forceinline__ f64x4 widen(f64x4 v) { return v; }

template <int R, typename V, typename A>
__device__ __forceinline__ void chain_round(A (&s)[4], const V* p, long long stride) {
    V v[R];
#pragma unroll
    for (int c = 0; c < R; ++c) v[c] = p[c * stride];
#pragma unroll
    for (int c = 0; c < R; ++c) s[c & 3] += widen(v[c]);
}

template <int DEPTH, typename V>
__device__ __forceinline__ auto sum_chains(const V* p, int count, long long stride) -> decltype(widen(*p)) {
    static_assert(DEPTH == 4 || DEPTH == 8, "sum_chains: 4 or 8 loads in flight");
    decltype(widen(*p)) s[4] = {};
    int i = 0;
    for (; i + DEPTH <= count; i += DEPTH, p += DEPTH * stride) chain_round<DEPTH>(s, p, stride);
    if (DEPTH == 8 && i + 4 <= count) {
        chain_round<4>(s, p, stride);
        i += 4;
        p += 4 * stride;
    }
    for (; i < count; ++i, p += stride) s[0] += widen(*p);
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// entry (n, k) of the reduced slab -> dweight[n][c][r][ss] (k = tap * C + c, tap = r * kw + ss), or
// dbias[n] for the bias column k == K of bias_mode 1; the pad columns above it are dropped
__device__ __forceinline__ void store_oihw(int n, int k, float v, int K, int C, int kh, int kw, int bias_mode,
                                           float* __restrict__ dw, float* __restrict__ db, int accumulate) {
    if (k < K) {
        const int tap = k / C, c = k - tap * C;
        const int r = tap / kw, ss = tap - r * kw;
        float* o = dw + (((long long)n * C + c) * kh + r) * kw + ss;
        *o = accumulate ? *o + v : v;
    } else if (bias_mode == 1 && k == K) {
        db[n] = accumulate ? db[n] + v : v;
    }
}

// pass 1 of the grouped form: part[g][idx] = sum over splits z = g, g + G, ... of slab[z][idx], a
// quad per thread with 8 x 16-B loads in flight (4 x 4 B per thread ran at ~1.3 TB/s)
__global__ __launch_bounds__(256) void wgrad_sum_splits4_kernel(const float* __restrict__ slab, int splits,
                                                                long long total, int G, double* __restrict__ part) {
    const long long idx = 4 * (blockIdx.x * (long long)blockDim.x + threadIdx.x);
    if (idx >= total) return;
    const int g = blockIdx.y;
    const f64x4 s = sum_chains<8>(reinterpret_cast<const f32x4*>(slab + (long long)g * total + idx),
                                  (splits - g + G - 1) / G, G * (total >> 2));
    double* o = part + (long long)g * total + idx;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = s[e];
}

// pass 2, quad finisher: sum the G partials of 4 consecutive entries of one slab row (8 quads in
// flight) and scatter them to PyTorch's [n][c][kh][kw] + bias.  Threads [0, total / 4) take the
// quads, threads [total / 4, total / 4 + C) the ConvT bias (mode 2).
// T = double: the G pass-1 partials;  T = float: the slab itself (G = splits, single pass).
// The ConvT bias (mode 2: entries t*C + c of row N over every tap t and partial g) has an order
// of its own: 4 interleaved fp64 chains over the flattened (t, g) sequence with 8 loads in flight,
// everything after the last whole 8-round on chain 0 (one dependent chain of taps x G loads was a
// latency tail, 17.7 us for a 64-channel ConvT in C2).  It is deterministic run to run (fixed
// order; pinned by tests/test_kernels_gpu.py::test_convT_bias_grad_run_to_run_bitwise).
template <typename T>
__global__ __launch_bounds__(256) void wgrad_finish4_kernel(const T* __restrict__ part, int G, int Nr, int Kc, int N,
                                                            int K, int C, int kh, int kw, int bias_mode,
                                                            float* __restrict__ dw, float* __restrict__ db,
                                                            int accumulate) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const long long total = (long long)Nr * Kc;
    const long long nq = total >> 2;
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q < nq) {
        const long long idx = 4 * q;
        const int n = int(idx / Kc);
        const int k0 = int(idx - (long long)n * Kc);
        if (n >= N) return;
        const f64x4 s = sum_chains<8>(reinterpret_cast<const t4*>(part + idx), G, nq);
#pragma unroll
        for (int e = 0; e < 4; ++e) store_oihw(n, k0 + e, (float)s[e], K, C, kh, kw, bias_mode, dw, db, accumulate);
    } else if (bias_mode == 2 && q < nq + C) {
        const int c = int(q - nq);
        const int J = kh * kw * G;                       // j = t * G + g
        const T* bp = part + (long long)N * Kc + c;
        auto at = [&](int j) {
            const int t = j / G, gg = j - t * G;
            return (double)bp[(long long)gg * total + t * C];
        };
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        int j = 0;
        for (; j + 7 < J; j += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = at(j + u);
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u & 3] += v[u];
        }
        for (; j < J; ++j) s[0] += at(j);
        const float v = (float)((s[0] + s[1]) + (s[2] + s[3]));
        db[c] = accumulate ? db[c] + v : v;
    }
}

// pass 2 with coalesced stores: block (chunk of 256 channels, row n) sums slab[.][n][tap*C + c]
// for its channels x taps (thread = (tap, 4 channels): 1-KB float4 reads per wave and split),
// transposes through LDS and stores the contiguous [c][kh][kw] run of dweight[n] as float4 (the
// scatter above writes 4 B at a 4*taps-byte stride).  The same sum_chains per entry as the quad
// finisher (4 loads in flight), so bit-identical to it.  C % 4 == 0, 16-B aligned rows;
// bias_mode 0/1 (the ConvT bias, mode 2, stays on wgrad_finish4_kernel).
template <typename T>
__global__ __launch_bounds__(576) void wgrad_finish_t_kernel(const T* __restrict__ part, int G, int Nr, int Kc, int K,
                                                              int C, int taps, int bias_mode, float* __restrict__ dw,
                                                              float* __restrict__ db, int accumulate) {
    __shared__ float tr[256 * 9];
    typedef T t4 __attribute__((ext_vector_type(4)));
    const long long total = (long long)Nr * Kc;
    const int n = blockIdx.y;
    const int c0 = blockIdx.x * 256;
    const int tap = threadIdx.x >> 6, cq = (threadIdx.x & 63) * 4;
    const int cn = min(256, C - c0);
    if (cq < cn) {
        const long long idx = (long long)n * Kc + tap * C + c0 + cq;
        const f64x4 s = sum_chains<4>(reinterpret_cast<const t4*>(part) + (idx >> 2), G, total >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) tr[(cq + e) * taps + tap] = (float)s[e];
    }
    if (bias_mode == 1 && blockIdx.x == 0 && threadIdx.x == 0) {
        const float v = (float)sum_chains<4>(part + (long long)n * Kc + K, G, total);
        db[n] = accumulate ? db[n] + v : v;
    }
    __syncthreads();
    // dweight[n][c0 .. c0+cn)[taps] is cn * taps contiguous floats; 16-B aligned when C*taps and
    // c0*taps are multiples of 4 (C % 4 == 0)
    float* o = dw + ((long long)n * C + c0) * taps;
    const int run = cn * taps;
    for (int i = threadIdx.x * 4; i < run; i += blockDim.x * 4) {
        f32x4 v = {tr[i], tr[i + 1], tr[i + 2], tr[i + 3]};
        if (accumulate) v += *reinterpret_cast<const f32x4*>(o + i);
        *reinterpret_cast<f32x4*>(o + i) = v;
    }
}

// `count` values v(0), v(1), ... in sum_chains' order: value i to chain i & 3 while
// i < 4 * (count / 4), the remainder to chain 0, result (s0 + s1) + (s2 + s3).  v(i) returns NV quads.
template <int NV, typename F>
__device__ __forceinline__ void chain_values(int count, F&& v, f64x4 (&out)[NV]) {
    f64x4 s[NV][4] = {};
    int i = 0;
    for (; i + 4 <= count; i += 4) {
        f32x4 q[4][NV];
#pragma unroll
        for (int u = 0; u < 4; ++u) v(i + u, q[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < NV; ++e) s[e][u] += widen(q[u][e]);
    }
    for (; i < count; ++i) {
        f32x4 q[NV];
        v(i, q);
#pragma unroll
        for (int e = 0; e < NV; ++e) s[e][0] += widen(q[e]);
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) out[e] = (s[e][0] + s[e][1]) + (s[e][2] + s[e][3]);
}

// phase 2 of the column plans (wgrad_wino_cols_x6_kernel): page 4 z + j of the slab holds
// R[r][j] = sum_a G[a][r] M[a][j] of tile split z at column r C + c, exactly the fp32 values
// wgrad_wino_x6_kernel forms before its waves exchange halves.  This kernel finishes that kernel's
// transform per split in fp32, in its order - P0 from columns 0, 1, P1 from columns 2, 3,
// dW[r][s] = P0[s] + P1[s] - and sums the splits in fp64 in the order that kernel's plan would
// take: G groups of splits g, g + G, ... in sum_chains' order, then (G > 1) the G partials again in
// sum_chains' order; one rounding to fp32.  G is the 64 x 64 plan's group count (1 or 2 for
// these shapes), so the result is bit-identical to wgrad_wino_x6_kernel + wgrad_reduce.
// Block (chunk of 256 channels, row n), thread (group lane g, r, 4 channels); the partials of
// G = 2 meet in LDS.  Transposed through LDS to the contiguous [c][3][3] run of dweight[n]:
// float4 when `vec` (16-byte aligned dweight), scalar otherwise.  The bias is column 3 C of the
// pages of column 1, the only blocks that read all four dZ pixels of a tile.
__global__ __launch_bounds__(384) void wgrad_finish_cols_kernel(const float* __restrict__ slab, int zs, int G, int Nr,
                                                                 int Kcp, int C, int bias_mode, float* __restrict__ dw,
                                                                 float* __restrict__ db, int accumulate, int vec) {
#pragma clang fp contract(off)
    __shared__ float tr[256 * 9];
    __shared__ double pp[2][9][256];
    __shared__ double pb[2];
    const long long total = (long long)Nr * Kcp;
    const int n = blockIdx.y;
    const int c0 = blockIdx.x * 256;
    const int g = threadIdx.x / 192, t = threadIdx.x - g * 192;
    const int r = t >> 6, cq = (t & 63) * 4;
    const int cn = min(256, C - c0);
    const int count = (zs - g + G - 1) / G;           // splits g, g + G, ...
    f64x4 acc[3];
    if (cq < cn) {
        const float* base = slab + (long long)n * Kcp + r * C + c0 + cq;
        chain_values<3>(count, [&](int i, f32x4 (&q)[3]) {
            const float* pz = base + (long long)(4 * (g + i * G)) * total;
            const f32x4 R0 = *reinterpret_cast<const f32x4*>(pz), R1 = *reinterpret_cast<const f32x4*>(pz + total);
            const f32x4 R2 = *reinterpret_cast<const f32x4*>(pz + 2 * total), R3 = *reinterpret_cast<const f32x4*>(pz + 3 * total);
            const f32x4 h1 = 0.5f * R1, h2 = 0.5f * R2;
            q[0] = (R0 + h1) + h2;
            q[1] = h1 + (-0.5f * R2);
            q[2] = h1 + (h2 + R3);
        }, acc);
        if (G > 1) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) pp[g][3 * r + s][cq + e] = acc[s][e];
        }
    }
    double bacc = 0.0;
    const bool bias_thread = bias_mode == 1 && blockIdx.x == 0 && t == 0;
    if (bias_thread) {
        const float* bp = slab + total + (long long)n * Kcp + 3 * C;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        int i = 0;
        for (; i + 4 <= count; i += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) s4[u] += (double)bp[(long long)(4 * (g + (i + u) * G)) * total];
        for (; i < count; ++i) s4[0] += (double)bp[(long long)(4 * (g + i * G)) * total];
        bacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        if (G > 1) pb[g] = bacc;
    }
    __syncthreads();
    if (g == 0) {
        if (cq < cn) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    double v = acc[s][e];
                    if (G > 1) {                      // two partials: both on chain 0
                        double c4[4] = {0.0, 0.0, 0.0, 0.0};
                        c4[0] += pp[0][3 * r + s][cq + e];
                        c4[0] += pp[1][3 * r + s][cq + e];
                        v = (c4[0] + c4[1]) + (c4[2] + c4[3]);
                    }
                    tr[(cq + e) * 9 + 3 * r + s] = (float)v;
                }
        }
        if (bias_thread) {
            double v = bacc;
            if (G > 1) {
                double c4[4] = {0.0, 0.0, 0.0, 0.0};
                c4[0] += pb[0];
                c4[0] += pb[1];
                v = (c4[0] + c4[1]) + (c4[2] + c4[3]);
            }
            db[n] = accumulate ? db[n] + (float)v : (float)v;
        }
    }
    __syncthreads();
    float* o = dw + ((long long)n * C + c0) * 9;
    const int run = cn * 9;
    if (vec) {
        for (int i = threadIdx.x * 4; i < run; i += blockDim.x * 4) {
            f32x4 v = {tr[i], tr[i + 1], tr[i + 2], tr[i + 3]};
            if (accumulate) v += *reinterpret_cast<const f32x4*>(o + i);
            *reinterpret_cast<f32x4*>(o + i) = v;
        }
    } else {
        for (int i = threadIdx.x; i < run; i += blockDim.x) o[i] = accumulate ? o[i] + tr[i] : tr[i];
    }
}

// One-launch reduction for the direct small-channel / stem weight gradients: up to 1024 split
// rows of a few thousand entries, where the two-pass form's per-thread chains over 64 splits were
// latency rounds, not bytes.  Block = 16 entries (4 float4 quads) x 64 split lanes: lane s sums
// splits s, s + 64, ... in 4 fp64 chains, then thread e < 16 sums the 64 lanes in order and
// scatters entry e into [n][c][kh][kw] (bias at column K) - a fixed order, deterministic.
constexpr int WR_E = 16, WR_S = 64;
__global__ __launch_bounds__(256) void wgrad_reduce_wide_kernel(const float* __restrict__ slab, int splits,
                                                                 long long total, int N, int Kcp, int K, int C,
                                                                 int kh, int kw, int bias_mode, float* __restrict__ dw,
                                                                 float* __restrict__ db, int accumulate) {
    __shared__ double part[WR_S][WR_E];
    const int quad = threadIdx.x & 3, sl = threadIdx.x >> 2;
    const long long idx0 = (long long)blockIdx.x * WR_E + 4 * quad;
    f64x4 a = {};
    if (idx0 < total)                                 // whole quads: total % 4 == 0
        a = sum_chains<4>(reinterpret_cast<const f32x4*>(slab + (long long)sl * total + idx0),
                          (splits - sl + WR_S - 1) / WR_S, WR_S * (total >> 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) part[sl][4 * quad + e] = a[e];
    __syncthreads();
    if (threadIdx.x >= WR_E) return;
    const long long idx = (long long)blockIdx.x * WR_E + threadIdx.x;
    if (idx >= total) return;
    double sum = 0.0;
    for (int l = 0; l < WR_S; ++l) sum += part[l][threadIdx.x];
    const int n = (int)(idx / Kcp), k = (int)(idx - (long long)n * Kcp);
    if (n >= N) return;
    store_oihw(n, k, (float)sum, K, C, kh, kw, bias_mode, dw, db, accumulate);
}

}  // namespace pu
