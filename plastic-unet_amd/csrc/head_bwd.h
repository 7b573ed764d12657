// Backward kernels of the plastic head (included by plastic.hip, whose entry points launch them):
// head_dx_kernel, head_dw_kernel and head_dw_reduce_kernel (the backward of Y = sigmoid(X Weff)),
// trace_bwd_partial_kernel and trace_bwd_finish_kernel (the backward of the trace rule) and
// head_dh_kernel (dL/dH of a slot).
#pragma once

#include "head_common.h"

namespace pu {

// dX[b][i][k] = sum_j G[b][i][j] * Weff_b[k][j]      grid (N/T, N/T, B)
// EX (the trace backward's extras, pu_plastic_bwd_trace): dY may be null (zeros), dy0 [B][N] is
// added to row 0 of dY before the sigmoid backward and dx0 [B][N] to row 0 of dX.
template <int T, bool EX = false>
__global__ __launch_bounds__(256) void head_dx_kernel(const float* __restrict__ Yv, const float* __restrict__ dY,
                                                      const float* __restrict__ H, const float* __restrict__ w,
                                                      const float* __restrict__ alpha, float* __restrict__ dX, int N,
                                                      const float* __restrict__ dy0, const float* __restrict__ dx0) {
#pragma clang fp contract(off)
    constexpr int M = T / 16;         // micro-tile side
    __shared__ float gs[HK][T + 4];   // gs[j][i]
    __shared__ float ws[HK][T + 4];   // ws[j][k]
    const int b = blockIdx.z;
    const int i0 = blockIdx.y * T, k0 = blockIdx.x * T;
    const long long off = (long long)b * N * N;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[M][M] = {};
    // the next chunk's operands are loaded into registers before this chunk's FMAs (raw values;
    // out-of-range entries load as 0, which the expressions below map to the 0 the tile needs)
    constexpr int E = HK * T / 256;
    static_assert(HK * T % 256 == 0, "whole loader rounds");
    float rdy[E], ryv[E], rw[E], ra[E], rh[E];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int jj = e % HK, rr = e / HK;
            const int gj = j0 + jj, gi = i0 + rr, gk = k0 + rr;
            rdy[u] = ryv[u] = rw[u] = ra[u] = rh[u] = 0.f;
            if (gi < N && gj < N) {
                const long long o = off + (long long)gi * N + gj;
                rdy[u] = load_dy<EX>(dY, dy0, o, gi == 0, (long long)b * N + gj);
                ryv[u] = Yv[o];
            }
            if (gk < N && gj < N) {
                const long long o = (long long)gk * N + gj;
                rw[u] = w[o];
                ra[u] = alpha[o];
                rh[u] = H[off + o];
            }
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < N; j0 += HK) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int jj = e % HK, rr = e / HK;
            gs[jj][rr] = sig_bwd(rdy[u], ryv[u]);
            ws[jj][rr] = rw[u] + ra[u] * rh[u];
        }
        __syncthreads();
        if (j0 + HK < N) fetch(j0 + HK);
#pragma unroll
        for (int jj = 0; jj < HK; ++jj) {
            float a[M], bb[M];
#pragma unroll
            for (int q = 0; q < M; ++q) { a[q] = gs[jj][ty * M + q]; bb[q] = ws[jj][tx * M + q]; }
            tile_fma<M>(acc, a, bb);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < M; ++q) {
        int gi = i0 + ty * M + q;
        if (gi >= N) continue;
#pragma unroll
        for (int r = 0; r < M; ++r) {
            int gk = k0 + tx * M + r;
            if (gk < N) {
                float v = acc[q][r];
                if constexpr (EX) {
                    if (gi == 0) v += dx0[(long long)b * N + gk];
                }
                dX[off + (long long)gi * N + gk] = v;
            }
        }
    }
}

// T_b[k][j] = sum_i X[b][i][k] * G[b][i][j];  per slot: partial[b] = (T_b, T_b * H_b).
// grid (N/T, N/T, B); the slot sum is a separate fixed-order pass (deterministic)
// EX: as head_dx_kernel (dY may be null, dy0 added to its row 0)
template <int T, bool EX = false>
__global__ __launch_bounds__(256) void head_dw_kernel(const float* __restrict__ X, const float* __restrict__ Yv,
                                                      const float* __restrict__ dY, const float* __restrict__ H,
                                                      float* __restrict__ partial, int N,
                                                      const float* __restrict__ dy0) {
#pragma clang fp contract(off)
    constexpr int M = T / 16;         // micro-tile side
    __shared__ float xs[HK][T + 4];   // xs[i][k]
    __shared__ float gs[HK][T + 4];   // gs[i][j]
    const int k0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const int b = blockIdx.z;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long off = (long long)b * N * N;
    float t[M][M] = {};
    // next chunk's raw operands in registers during this chunk's FMAs (as head_dx_kernel)
    constexpr int E = HK * T / 256;
    static_assert(HK * T % 256 == 0, "whole loader rounds");
    float rx[E], rdy[E], ryv[E];
    auto fetch = [&](int i0) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int cc = e % T, ii = e / T;
            const int gi = i0 + ii, gk = k0 + cc, gj = j0 + cc;
            rx[u] = (gi < N && gk < N) ? X[off + (long long)gi * N + gk] : 0.f;
            rdy[u] = ryv[u] = 0.f;
            if (gi < N && gj < N) {
                const long long o = off + (long long)gi * N + gj;
                rdy[u] = load_dy<EX>(dY, dy0, o, gi == 0, (long long)b * N + gj);
                ryv[u] = Yv[o];
            }
        }
    };
    fetch(0);
    for (int i0 = 0; i0 < N; i0 += HK) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int cc = e % T, ii = e / T;
            xs[ii][cc] = rx[u];
            gs[ii][cc] = sig_bwd(rdy[u], ryv[u]);
        }
        __syncthreads();
        if (i0 + HK < N) fetch(i0 + HK);
#pragma unroll
        for (int ii = 0; ii < HK; ++ii) {
            float a[M], bb[M];
#pragma unroll
            for (int q = 0; q < M; ++q) { a[q] = xs[ii][ty * M + q]; bb[q] = gs[ii][tx * M + q]; }
            tile_fma<M>(t, a, bb);
        }
        __syncthreads();
    }
    float* pw = partial + (long long)b * 2 * N * N;
    float* pa = pw + (long long)N * N;
#pragma unroll
    for (int q = 0; q < M; ++q) {
        int gk = k0 + ty * M + q;
        if (gk >= N) continue;
#pragma unroll
        for (int r = 0; r < M; ++r) {
            int gj = j0 + tx * M + r;
            if (gj < N) {
                const long long o = (long long)gk * N + gj;
                pw[o] = t[q][r];
                pa[o] = t[q][r] * H[off + o];
            }
        }
    }
}

// dw = sum_b T_b, dalpha = sum_b T_b * H_b, slots summed in order 0..B-1
__global__ void head_dw_reduce_kernel(const float* __restrict__ partial, int B, int N, float* __restrict__ dw,
                                      float* __restrict__ da) {
#pragma clang fp contract(off)
    const long long nn = (long long)N * N;
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= nn) return;
    float sw = 0.f, sa = 0.f;
    for (int z = 0; z < B; ++z) {
        sw += partial[(long long)z * 2 * nn + idx];
        sa += partial[(long long)z * 2 * nn + nn + idx];
    }
    dw[idx] = sw;
    da[idx] = sa;
}

// ------------------------------------------------------------------- backward of the trace rule
// Given P = dL/dH' (pu_plastic_bwd_trace), per slot b with x0 = X_b[0,:], y0 = Y_b[0,:]:
//   hebb  H' = (1-eta) H + eta x0[k] y0[j]            oja  H' = H + eta (x0[k] - H y0[j]) y0[j]
//   dx0[k] = eta sum_j P y0[j]                         (both rules)
//   dy0[j] = eta sum_k P x0[k]                         oja: eta sum_k P (x0[k] - 2 H y0[j])
//   deta   = sum_bkj P (x0[k] y0[j] - H)               oja: sum_bkj P y0[j] (x0[k] - H y0[j])
// One read of P and H (8 B N^2 bytes).  A block is 8 groups of 32 lanes; a group walks rows
// k0 + g, k0 + g + 8 of a TB_ROWS-row chunk, a lane owns V adjacent columns of a 32 V column
// strip (V = 4: float4 loads).  Row sums: xor tree over the group's lanes -> rowp[b][k][strip];
// column sums: lane registers over the group's rows, then the 8 groups in order through LDS ->
// colp[b][chunk][j]; deta: fp64 per lane, LDS tree -> etap[block].  trace_bwd_finish_kernel sums
// the partials in index order (no atomics anywhere: deterministic).
constexpr int TB_ROWS = 16;

template <int V>
__global__ __launch_bounds__(256) void trace_bwd_partial_kernel(const float* __restrict__ P, const float* __restrict__ H,
                                                                const float* __restrict__ X, const float* __restrict__ Y,
                                                                int N, int rule, float* __restrict__ rowp,
                                                                float* __restrict__ colp, double* __restrict__ etap) {
#pragma clang fp contract(off)
    __shared__ float cs[8][32 * V];
    const int strip = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int nstrips = gridDim.x, nchunks = gridDim.y;
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const long long off = (long long)b * N * N;
    const int j = strip * 32 * V + l * V;
    const bool jin = j < N;                       // V = 4 runs only with N % 4 == 0: j < N covers j + 3
    float y0[V], col[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        y0[e] = jin ? Y[off + j + e] : 0.f;
        col[e] = 0.f;
    }
    double es = 0.0;
    for (int it = 0; it < TB_ROWS / 8; ++it) {
        const int k = chunk * TB_ROWS + it * 8 + g;
        const bool in = jin && k < N;
        float p[V], h[V];
        if constexpr (V == 4) {
            f32x4 pv = {0.f, 0.f, 0.f, 0.f}, hv = pv;
            if (in) {
                pv = *reinterpret_cast<const f32x4*>(P + off + (long long)k * N + j);
                hv = *reinterpret_cast<const f32x4*>(H + off + (long long)k * N + j);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { p[e] = pv[e]; h[e] = hv[e]; }
        } else {
            p[0] = in ? P[off + (long long)k * N + j] : 0.f;
            h[0] = in ? H[off + (long long)k * N + j] : 0.f;
        }
        const float x0 = k < N ? X[off + k] : 0.f;
        float rs = 0.f;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            rs += p[e] * y0[e];
            if (rule == PU_RULE_HEBB) {
                col[e] += p[e] * x0;
                es += (double)(p[e] * (x0 * y0[e] - h[e]));
            } else {
                const float hy = h[e] * y0[e];
                col[e] += p[e] * (x0 - 2.f * hy);
                es += (double)(p[e] * y0[e] * (x0 - hy));
            }
        }
        // every lane of the wave takes part (out-of-range lanes carry zeros); the xor distances
        // stay inside the 32-lane group
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) rs += __shfl_xor(rs, d);
        if (l == 0 && k < N) rowp[((long long)b * N + k) * nstrips + strip] = rs;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) cs[g][l * V + e] = col[e];
    es = block_tree256(es);           // its first barrier also publishes cs
    if (threadIdx.x < 32 * V) {
        const int jc = strip * 32 * V + threadIdx.x;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += cs[q][threadIdx.x];
        if (jc < N) colp[((long long)b * nchunks + chunk) * N + jc] = s;
    }
    if (threadIdx.x == 0) etap[((long long)b * nchunks + chunk) * nstrips + strip] = es;
}

// dx0[b][k] = eta sum_strip rowp, dy0[b][j] = eta sum_chunk colp (grid-stride over B N); block 0
// also sums the np fp64 deta partials in index order -> deta[0]
__global__ __launch_bounds__(256) void trace_bwd_finish_kernel(const float* __restrict__ rowp, const float* __restrict__ colp,
                                                               const double* __restrict__ etap, const float* __restrict__ eta_p,
                                                               int B, int N, int nstrips, int nchunks, int np,
                                                               float* __restrict__ dx0, float* __restrict__ dy0,
                                                               float* __restrict__ deta) {
#pragma clang fp contract(off)
    const float eta = eta_p[0];
    const long long total = (long long)B * N;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / N), c = (int)(i - (long long)b * N);
        float sr = 0.f, sc = 0.f;
        for (int s = 0; s < nstrips; ++s) sr += rowp[i * nstrips + s];
        for (int q = 0; q < nchunks; ++q) sc += colp[((long long)b * nchunks + q) * N + c];
        dx0[i] = eta * sr;
        dy0[i] = eta * sc;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += etap[i];
    s = block_tree256(s);
    if (threadIdx.x == 0) deta[0] = (float)s;
}

// dH_b = dH_t + alpha (.) T_b, T_b = the per-slot product head_dw_kernel left in the workspace;
// dH_t = (1-eta) P (hebb) or P (1 - eta y0[j]^2) (oja), 0 without P.  One pass: 12 B in, 4 B out
// per element.  grid (ceil(N N / V / 256), B)
template <int V>
__global__ __launch_bounds__(256) void head_dh_kernel(const float* __restrict__ P, const float* __restrict__ Y,
                                                      const float* __restrict__ alpha, const float* __restrict__ partial,
                                                      const float* __restrict__ eta_p, int N, int rule,
                                                      float* __restrict__ dH) {
#pragma clang fp contract(off)
    const long long nn = (long long)N * N;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= nn) return;
    const int b = blockIdx.y;
    const long long off = (long long)b * nn;
    const float* Tb = partial + (long long)b * 2 * nn;
    const int j = (int)(idx % N);
    float p[V], t[V], a[V], o[V];
    if constexpr (V == 4) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(Tb + idx), av = *reinterpret_cast<const f32x4*>(alpha + idx);
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (P) pv = *reinterpret_cast<const f32x4*>(P + off + idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) { p[e] = pv[e]; t[e] = tv[e]; a[e] = av[e]; }
    } else {
        p[0] = P ? P[off + idx] : 0.f;
        t[0] = Tb[idx];
        a[0] = alpha[idx];
    }
    if (P) {
        const float eta = eta_p[0];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float f = 1.f - eta;
            if (rule != PU_RULE_HEBB) {
                const float y0 = Y[off + j + e];
                f = 1.f - eta * (y0 * y0);
            }
            o[e] = p[e] * f + a[e] * t[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = a[e] * t[e];
    }
    if constexpr (V == 4) {
        f32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = o[e];
        *reinterpret_cast<f32x4*>(dH + off + idx) = ov;
    } else {
        dH[off + idx] = o[0];
    }
}

}  // namespace pu
