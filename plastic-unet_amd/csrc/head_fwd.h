// Forward kernels of the plastic head (included by plastic.hip, whose entry points launch them):
// head_fwd_kernel (VALU GEMM, optional fused trace update), trace_kernel(_v4) (the stand-alone
// update), head_fused_fwd_kernel (outconv + head, phase-serial) and head_pipe_fwd_kernel (the same,
// pipelined, at N = 128).
#pragma once

#include "head_common.h"

namespace pu {

// Y[b][i][j] = sigmoid( sum_k X[b][i][k] * (w[k][j] + alpha[k][j]*H[b][k][j]) )     (unet_p.py:70-79)
// With Hn != nullptr the trace update is fused in: every block also accumulates row 0 of its
// column tile (y0 = Y[b][0][j0:j0+T], the same fmaf chain as the block that owns row 0, so the
// values are identical) and then writes H'[b][k][j] for its own T x T tile with k in the tile's
// row range: H is read from HBM once for Weff and re-read from L2 for the update; one launch.
// Hn must not alias H (other blocks still read H).  grid (N/T, N/T, B)
template <int T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ X, const float* __restrict__ H,
                                                       const float* __restrict__ w, const float* __restrict__ alpha,
                                                       float* __restrict__ Y, float* __restrict__ Hn,
                                                       const float* __restrict__ eta_p, int N, int rule) {
#pragma clang fp contract(off)
    constexpr int M = T / 16;          // micro-tile side
    __shared__ float xs[HK][T + 4];    // xs[k][i]
    __shared__ float ws[HK][T + 4];    // ws[k][j]
    __shared__ float x0s[HK];          // X[b][0][k]
    __shared__ float y0s[T];
    const int b = blockIdx.z;
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const float* Xb = X + (long long)b * N * N;
    const float* Hb = H + (long long)b * N * N;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const bool fuse = Hn != nullptr;
    float acc[M][M] = {};
    float acc0[M] = {};
    for (int k0 = 0; k0 < N; k0 += HK) {
        for (int e = threadIdx.x; e < HK * T; e += 256) {
            int kk = e % HK, ii = e / HK;               // X tile: row i x k, stored transposed
            int gi = i0 + ii, gk = k0 + kk;
            xs[kk][ii] = (gi < N && gk < N) ? Xb[(long long)gi * N + gk] : 0.f;
            int jj = e % T, kk2 = e / T;                // Weff tile: k x j
            int gj = j0 + jj, gk2 = k0 + kk2;
            float v = 0.f;
            if (gj < N && gk2 < N) {
                long long o = (long long)gk2 * N + gj;
                v = w[o] + alpha[o] * Hb[o];   // torch: w + mul(alpha, hebb) - two roundings
            }
            ws[kk2][jj] = v;
        }
        if (fuse && threadIdx.x < HK) x0s[threadIdx.x] = (k0 + threadIdx.x < N) ? Xb[k0 + threadIdx.x] : 0.f;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HK; ++kk) {
            float a[M], bb[M];
#pragma unroll
            for (int q = 0; q < M; ++q) { a[q] = xs[kk][ty * M + q]; bb[q] = ws[kk][tx * M + q]; }
            tile_fma<M>(acc, a, bb);
            if (fuse && ty == 0) {
                const float a0 = x0s[kk];
#pragma unroll
                for (int r = 0; r < M; ++r) acc0[r] = fmaf(a0, bb[r], acc0[r]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < M; ++q) {
        int gi = i0 + ty * M + q;
        if (gi >= N) continue;
#pragma unroll
        for (int r = 0; r < M; ++r) {
            int gj = j0 + tx * M + r;
            if (gj < N) Y[((long long)b * N + gi) * N + gj] = sigmoid(acc[q][r]);
        }
    }
    if (!fuse) return;
    if (ty == 0) {
#pragma unroll
        for (int r = 0; r < M; ++r) y0s[tx * M + r] = sigmoid(acc0[r]);
    }
    __syncthreads();
    const float eta = eta_p[0];
    const float one_m_eta = 1.f - eta;
    float* Hnb = Hn + (long long)b * N * N;
    // H' rows k = i0.. (the tile's row range), columns j0..: coalesced over j
    for (int e = threadIdx.x; e < T * T; e += 256) {
        const int kk = e / T, jj = e % T;
        const int gk = i0 + kk, gj = j0 + jj;
        if (gk < N && gj < N) {
            const long long o = (long long)gk * N + gj;
            Hnb[o] = trace_rule(Hb[o], Xb[gk], y0s[jj], eta, one_m_eta, rule);
        }
    }
}

// H'[b][k][j] from x0 = X[b][0][k] and y0 = Y[b][0][j]  (unet_p.py:81-86); the stand-alone update
// (pu_trace_update).  grid (ceil(N*N/4 / 256), B): one float4 per thread, 32-bit indexing
__global__ void trace_kernel(const float* __restrict__ H, const float* __restrict__ X, const float* __restrict__ Y,
                             const float* __restrict__ eta_p, float* __restrict__ Hn, int N, int rule) {
#pragma clang fp contract(off)
    const float eta = eta_p[0];
    const float one_m_eta = 1.f - eta;
    const long long off = (long long)blockIdx.y * N * N;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    const int k = idx / N, j = idx - k * N;
    Hn[off + idx] = trace_rule(H[off + idx], X[off + k], Y[off + j], eta, one_m_eta, rule);
}

__global__ void trace_kernel_v4(const float* __restrict__ H, const float* __restrict__ X, const float* __restrict__ Y,
                                const float* __restrict__ eta_p, float* __restrict__ Hn, int N, int rule) {
#pragma clang fp contract(off)
    const float eta = eta_p[0];
    const float one_m_eta = 1.f - eta;
    const int N4 = N >> 2;
    const long long off = (long long)blockIdx.y * N * N;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;    // float4 index within the slot
    if (idx >= N * N4) return;
    const int k = idx / N4, j4 = idx - k * N4;
    const f32x4 h = reinterpret_cast<const f32x4*>(H + off)[idx];
    const float x0 = X[off + k];
    const f32x4 y0 = *reinterpret_cast<const f32x4*>(Y + off + j4 * 4);
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = trace_rule(h[e], x0, y0[e], eta, one_m_eta, rule);
    reinterpret_cast<f32x4*>(Hn + off)[idx] = out;
}


// ------------------------------------------------------------------- fused head (outconv + head)
// One block (512 threads, two per CU at N = 128) = 16 rows i0..i0+15 of slot b, all N columns.  Phases:
//  1. outconv of the block's 16 rows and of row 0 (x0, needed by the trace update) into LDS:
//     L lanes per pixel (L = C/4 up to 16), float4 channel loads, U pixels per lane group in
//     flight, dot4_fma + lane_tree16 over the L lanes - the arithmetic of outconv_fwd_kernel (whose
//     idle lanes add zeros), so X is bit-identical to the two-launch path;
//  2. Weff_b = w + alpha (.) H_b in chunks of kc rows through LDS (all of it at N <= 128); Y = X Weff
//     on v_mfma_f32_16x16x4_f32 (column tile t -> wave t mod 8) and y0 = x0 Weff as a VALU fmaf
//     chain in the same k order (== the MFMA's, bitwise), so every block holds row 0's Y;
//  3. Y = sigmoid, X rows written out (the backward's input);
//  4. H'[k][j] for the block's rows k from H, x0[k], y0[j] (unet_p.py:81-86 operation order).
constexpr int FH_R = 16;      // rows per block (32 at nbf >= 256: see pu_plastic_head_fwd)
constexpr int FH_NT = 512;    // threads per block (2 blocks per CU at nbf 128: one block's feature
                               // loads overlap the other's GEMM / trace phases)
constexpr int FH_WAVES = FH_NT / 64;
constexpr int FH_LDS_W = 16384;   // floats of the Weff chunk (64 KB)

// Weff rows per LDS chunk: all N rows when N x N fits, else the largest multiple of 4 (the MFMA's
// k step) that divides N and fits (N % 16 == 0, so 16 always qualifies: N = 144 -> 72, 192 -> 64,
// 320 -> 40, 384 -> 32, 512 -> 32).  The chunk loop steps k0 by kc up to N, so kc must divide N.
inline int fused_head_chunk(int N) {
    if (N * N <= FH_LDS_W) return N;
    int best = 16;
    for (int d = 4; d * N <= FH_LDS_W && d <= N; d += 4)
        if (N % d == 0) best = d;
    return best;
}

template <typename T, int L, int TPW, int R = FH_R>
__global__ __launch_bounds__(FH_NT) void head_fused_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ wo,
                                                               const float* __restrict__ bo, int C,
                                                               const float* __restrict__ H, const float* __restrict__ w,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ eta_p, float* __restrict__ X,
                                                               float* __restrict__ Y, float* __restrict__ Hn, int N,
                                                               FastDiv dN, int kc, int rule) {
    constexpr int RT = (R + 15) / 16;         // 16-row MFMA tiles of the block's rows
    extern __shared__ float fh_lds[];
    float* xs = fh_lds;                       // [R + 1][N]: own rows, then row 0
    float* ws = xs + (R + 1) * N;             // [kc][N]
    float* y0s = ws + kc * N;                 // [N]
    const int b = blockIdx.y;
    const int i0 = blockIdx.x * R;
    const int tid = threadIdx.x;
    const bool fuse = Hn != nullptr;
    const long long nn = (long long)N * N;
    const T* fb = feat + (long long)b * nn * C;
    const float* Hb = H + (long long)b * nn;

    // ---- 1. outconv
    {
        constexpr int U = L >= 8 ? 8 : 4;       // pixels per lane group in flight
        const float bias = bo ? bo[0] : 0.f;
        const int lane = tid % L;
        constexpr int PPP = FH_NT / L;          // pixels per pass
        const int npix = (fuse ? R + 1 : R) * N;
        auto reduce_store = [&](int q0, float (&s)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float t = lane_tree16<L>(s[u]);
                const int q = q0 + u * PPP;
                if (lane == 0 && q < npix) xs[q] = t + bias;
            }
        };
        auto pixel = [&](int q) -> const T* {
            q = min(q, npix - 1);
            const int r = (int)fdiv((unsigned)q, dN), k = q - r * N;
            return fb + ((long long)(r < R ? i0 + r : 0) * N + k) * C;
        };
        for (int q0 = tid / L; q0 < npix; q0 += U * PPP) {
            const T* px[U];
#pragma unroll
            for (int u = 0; u < U; ++u) px[u] = pixel(q0 + u * PPP);
            float sacc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) sacc[u] = 0.f;
            for (int c = lane * 4; c < C; c += 4 * L) {
                const f32x4 ww = *reinterpret_cast<const f32x4*>(wo + c);
                f32x4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = ld4(px[u] + c);
#pragma unroll
                for (int u = 0; u < U; ++u) sacc[u] += dot4_fma(v[u], ww);
            }
            reduce_store(q0, sacc);
        }
    }
    __syncthreads();
    // X rows of this block -> global (coalesced)
    for (int e = tid; e < R * N; e += FH_NT) X[(long long)b * nn + (long long)i0 * N + e] = xs[e];

    // the trace update's first float4 of H (rows i0.., L2-resident after the Weff build), in
    // flight during the GEMM
    f32x4 hpre = f32x4{0.f, 0.f, 0.f, 0.f};
    if (fuse && tid < R * N / 4) hpre = reinterpret_cast<const f32x4*>(Hb + (long long)i0 * N)[tid];

    // ---- 2. GEMM
    const int wave = tid >> 6, l = tid & 63;
    const int tiles = N / 16;
    f32x4 acc[TPW][RT];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[t][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float acc0 = 0.f;                                  // y0 chain of column tid (tid < N)
    for (int k0 = 0; k0 < N; k0 += kc) {
        {
#pragma clang fp contract(off)
            // float4 pieces, 8 per array and thread in flight at once (N = 128: the whole chunk in
            // one round trip; the scalar form took four, 4.4 us of the kernel by ablation)
            const int ne4 = kc * N / 4;
            const f32x4* w4 = reinterpret_cast<const f32x4*>(w + (long long)k0 * N);
            const f32x4* a4 = reinterpret_cast<const f32x4*>(alpha + (long long)k0 * N);
            const f32x4* h4 = reinterpret_cast<const f32x4*>(Hb + (long long)k0 * N);
            for (int e0 = tid; e0 < ne4; e0 += 8 * FH_NT) {
                f32x4 wv[8], av[8], hv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int o = min(e0 + FH_NT * u, ne4 - 1);
                    wv[u] = w4[o]; av[u] = a4[o]; hv[u] = h4[o];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (e0 + FH_NT * u < ne4) {
                        f32x4 o;
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] = wv[u][c] + av[u][c] * hv[u][c];   // torch: w + mul(alpha, hebb)
                        reinterpret_cast<f32x4*>(ws)[e0 + FH_NT * u] = o;
                    }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int tile = wave + FH_WAVES * t;
            if (tile < tiles) {
                const float* wcol = ws + (l >> 4) * N + tile * 16 + (l & 15);
                const float* xrow = xs + (l & 15) * N + k0 + (l >> 4);   // row tile rt: + 16 rt N
                // operands of 4 k-steps read before their MFMAs (kc % 16 == 0 or kc = 4 .. 12: see
                // fused_head_chunk - the tail loop takes the rest); each W fragment feeds RT tiles
                int kk = 0;
                for (; kk + 16 <= kc; kk += 16) {
                    float xa[RT][4], wb[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        wb[j] = wcol[(kk + 4 * j) * N];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) xa[rt][j] = xrow[16 * rt * N + kk + 4 * j];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            acc[t][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt][j], wb[j], acc[t][rt], 0, 0, 0);
                }
                for (; kk < kc; kk += 4)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[t][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xrow[16 * rt * N + kk], wcol[kk * N], acc[t][rt], 0, 0, 0);
            }
        }
        if (fuse && tid < N) {
            // the same k-ordered fmaf chain; 8 k's operands read ahead of their fmas
            float s0 = acc0;
            int kk = 0;
            for (; kk + 8 <= kc; kk += 8) {
                float xa[8], wb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { xa[j] = xs[R * N + k0 + kk + j]; wb[j] = ws[(kk + j) * N + tid]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) s0 = fmaf(xa[j], wb[j], s0);
            }
            for (; kk < kc; ++kk) s0 = fmaf(xs[R * N + k0 + kk], ws[kk * N + tid], s0);
            acc0 = s0;
        }
        __syncthreads();
    }

    // ---- 3. sigmoid + store (C layout of 16x16: column l & 15, rows 4 (l >> 4) + reg)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = wave + FH_WAVES * t;
        if (tile < tiles) {
            const int j = tile * 16 + (l & 15);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                if (16 * rt + 4 * (l >> 4) < R) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int gi = i0 + 16 * rt + 4 * (l >> 4) + r;
                        Y[((long long)b * N + gi) * N + j] = sigmoid(acc[t][rt][r]);
                    }
                }
            }
        }
    }
    if (!fuse) return;
    if (tid < N) y0s[tid] = sigmoid(acc0);
    __syncthreads();

    // ---- 4. trace update of rows k = i0 .. i0+15
    const float eta = eta_p[0];
    const float one_m_eta = 1.f - eta;
    // rows i0 .. i0+R-1 of H / H' are contiguous: float4 over the block's R * N elements
    const f32x4* Hr = reinterpret_cast<const f32x4*>(Hb + (long long)i0 * N);
    f32x4* Hnr = reinterpret_cast<f32x4*>(Hn + (long long)b * nn + (long long)i0 * N);
    for (int e4 = tid; e4 < R * N / 4; e4 += FH_NT) {
        const f32x4 h = e4 == tid ? hpre : Hr[e4];
        const int kk = (int)fdiv((unsigned)(4 * e4), dN), j = 4 * e4 - kk * N;
        const float x0 = xs[R * N + i0 + kk];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = trace_rule(h[e], x0, y0s[j + e], eta, one_m_eta, rule);
        Hnr[e4] = o;
    }
}

// ------------------------------------------------------- fused head, pipelined (N = 128, L = 16)
// head_fused_fwd_kernel runs its phases one after the other on all 8 waves: the feature stream
// (outconv, 26.5 us of its 35.7 at bs 32 x 128^2 x 64 channels), then Weff / GEMM / y0 / the
// trace update (9 us of latency chains) - with one block per CU nothing overlaps that tail.  Here
// 12 waves split the roles:
//   waves 0..7 (streamers, the serial kernel's outconv configuration and per-CU stream rate): one
//     continuous stream over the 17 rows in the order row 0, i0 .. i0+15, 256 pixels per pass with
//     the next pass's loads issued before the current pass is reduced - so the block barriers
//     between phases (every 2 passes = 2 rows at U = 4) do not drain the memory pipeline;
//   waves 8..11 (workers): phase 0 builds Weff = w + alpha (.) H_b in LDS; after every phase they
//     form Y = X Weff for the rows just streamed (thread = (column j, row), one k-ordered
//     fmaf chain per row - the MFMA's chain, bit-identical), sigmoid, store; the phase after row 0's
//     y0 runs the block's trace update.
// What is left after the stream is one row's GEMM.  Arithmetic identical to head_fused_fwd_kernel
// (the same outconv lane tree, k order, sigmoid and trace expressions).
constexpr int HP_SW = 8 * 64;        // streamer threads (8 waves)
constexpr int HP_NT = HP_SW + 256;   // ... and 4 worker waves
constexpr int HP_U = 4;              // pixels in flight per streamer lane group and pass (4: one row per pass)
constexpr int HP_N = 128;
template <typename T>
__global__ __launch_bounds__(HP_NT) void head_pipe_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ wo,
                                                              const float* __restrict__ bo, int C,
                                                              const float* __restrict__ H, const float* __restrict__ w,
                                                              const float* __restrict__ alpha,
                                                              const float* __restrict__ eta_p, float* __restrict__ X,
                                                              float* __restrict__ Y, float* __restrict__ Hn, int rule) {
#pragma clang fp contract(off)
    constexpr int N = HP_N, L = 16, R = 16;
    constexpr int PPP = HP_SW / L;            // pixels per lane-group round
    constexpr int PPI = HP_U * PPP;           // pixels per pass
    constexpr int NPIX = (R + 1) * N;         // the stream: row 0, then rows i0 .. i0+15
    constexpr int NPASS = (NPIX + PPI - 1) / PPI;
    constexpr int NPH = (NPASS + 1) / 2;      // phases (2 passes each)
    constexpr int RPP = 2 * PPI / N;          // stream rows per phase (2 with 8 streamer waves at U = 4)
    constexpr int RPT = RPP / 2;              // rows per worker thread and phase
    static_assert(PPI % N == 0 && RPT <= 3, "a pass is whole rows");
    static_assert(N / R == 8, "the XCD block order below assumes 8 row blocks per slot");
    __shared__ __attribute__((aligned(16))) float xs[(R + 1) * N];   // stream order: row 0, then own rows
    __shared__ __attribute__((aligned(16))) float ws[N * N];
    __shared__ float y0s[N];
    // XCD-aware block order: blocks are dealt round-robin over the 8 XCDs by linear id, so the
    // plain (row block, slot) grid put row block x of EVERY slot on XCD x and each XCD's L2 fetched
    // every slot's H_b (W_eff) and row-0 features - 8x per slot.  Unit u = xcd * B + (lin / 8)
    // gives each XCD a contiguous run of units: the 8 row blocks of a slot share one XCD (B % 8 ==
    // 0; otherwise at most one slot straddles two).  A bijection on [0, 8B): speed only, the
    // per-block arithmetic does not depend on the placement.
    const int nslot = gridDim.y;
    const int lin = blockIdx.x + (N / R) * blockIdx.y;
    const int unit = (lin & 7) * nslot + (lin >> 3);
    const int b = unit / (N / R);
    const int rb = unit % (N / R);
    const int i0 = rb * R;
    const int tid = threadIdx.x;
    const bool streamer = tid < HP_SW;        // wave-uniform
    const long long nn = (long long)N * N;
    const T* fb = feat + (long long)b * nn * C;
    const float* Hb = H + (long long)b * nn;

    if (streamer) {
        const float bias = bo ? bo[0] : 0.f;
        const int lane = tid % L;
        f32x4 buf[2][HP_U];
        // pixels of pass k (stream order q -> image row: q / N == 0 ? 0 : i0 + q / N - 1)
        auto load = [&](int k, f32x4 (&v)[HP_U]) {
#pragma unroll
            for (int u = 0; u < HP_U; ++u) {
                const int q = min(k * PPI + tid / L + u * PPP, NPIX - 1);
                const int r = q / N, col = q & (N - 1);
                const T* px = fb + ((long long)(r == 0 ? 0 : i0 + r - 1) * N + col) * C;
                v[u] = ld4(px + lane * 4);
            }
        };
        const f32x4 ww = *reinterpret_cast<const f32x4*>(wo + lane * 4);
        // reduce pass k from registers v (the next pass's loads already in flight)
        auto reduce = [&](int k, const f32x4 (&v)[HP_U]) {
#pragma unroll
            for (int u = 0; u < HP_U; ++u) {
                const int q = k * PPI + tid / L + u * PPP;
                float sacc = 0.f;
                sacc += dot4_fma(v[u], ww);
                if (C > 4 * L) {                  // channels beyond the first 64 (not prefetched)
                    const int qc = min(q, NPIX - 1);
                    const int r = qc / N, col = qc & (N - 1);
                    const T* px = fb + ((long long)(r == 0 ? 0 : i0 + r - 1) * N + col) * C;
                    for (int c = lane * 4 + 4 * L; c < C; c += 4 * L)
                        sacc += dot4_fma(ld4(px + c), *reinterpret_cast<const f32x4*>(wo + c));
                }
                const float t = lane_tree16<L>(sacc);
                if (lane == 0 && q < NPIX) xs[q] = t + bias;
            }
        };
        // passes in pairs (static buffer roles): a phase = 2 passes = 2 rows, then the barrier
        load(0, buf[0]);
#pragma unroll 1
        for (int k = 0; k < NPASS; k += 2) {
            if (k + 1 < NPASS) load(k + 1, buf[1]);
            reduce(k, buf[0]);
            if (k + 1 < NPASS) {
                if (k + 2 < NPASS) load(k + 2, buf[0]);
                reduce(k + 1, buf[1]);
            }
            __syncthreads();                  // this phase's rows are in xs
        }
        // X rows out (stream rows 1 .. 16 = image rows i0 .. i0+15)
        for (int e = tid; e < R * N; e += HP_SW) X[(long long)b * nn + (long long)i0 * N + e] = xs[N + e];
    } else {
        const int tw = tid - HP_SW;           // 0 .. 255
        const int j = tw & (N - 1), rh = tw >> 7;
        // phase 0: Weff (head_fused_fwd_kernel's fill without its clamp and guard.  The two stay apart,
        // and so do the trace updates below: as shared functions they changed the instruction
        // selection or the GEMM's schedule of these two kernels - DESIGN.md)
        {
            const f32x4* w4 = reinterpret_cast<const f32x4*>(w);
            const f32x4* a4 = reinterpret_cast<const f32x4*>(alpha);
            const f32x4* h4 = reinterpret_cast<const f32x4*>(Hb);
            for (int e0 = tw; e0 < N * N / 4; e0 += 8 * 256) {
                f32x4 wv[8], av[8], hv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int o = e0 + 256 * u;
                    wv[u] = w4[o]; av[u] = a4[o]; hv[u] = h4[o];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    f32x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = wv[u][c] + av[u][c] * hv[u][c];   // torch: w + mul(alpha, hebb)
                    reinterpret_cast<f32x4*>(ws)[e0 + 256 * u] = o;
                }
            }
        }
        for (int ph = 0; ph < NPH; ++ph) {
            __syncthreads();                  // phase ph's stream rows are in xs
            // Y of stream rows RPP ph + RPT rh .. (stream row 0 = image row 0 -> y0 only)
            const int s0 = RPP * ph + RPT * rh;
            const int nrow = max(0, min(RPT, R + 1 - s0));
            if (nrow > 0) {
                float acc[RPT];
#pragma unroll
                for (int r = 0; r < RPT; ++r) acc[r] = 0.f;
                for (int k = 0; k < N; k += 4) {
                    float wk[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) wk[e] = ws[(k + e) * N + j];
#pragma unroll
                    for (int r = 0; r < RPT; ++r)
                        if (r < nrow) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[r] = fmaf(xs[(s0 + r) * N + k + e], wk[e], acc[r]);
                        }
                }
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    if (r < nrow) {
                        const float y = sigmoid(acc[r]);
                        if (s0 + r == 0) y0s[j] = y;
                        else Y[((long long)b * N + i0 + s0 + r - 1) * N + j] = y;
                    }
            }
            if (ph == 1) {                    // (RPP >= 2: y0 was formed in phase 0)
                // trace update of rows i0 .. i0+15 (y0 formed in phase 0's GEMM - complete at this
                // phase's barrier -, x0 = stream row 0)
                const float eta = eta_p[0];
                const float one_m_eta = 1.f - eta;
                const f32x4* Hr = reinterpret_cast<const f32x4*>(Hb + (long long)i0 * N);
                f32x4* Hnr = reinterpret_cast<f32x4*>(Hn + (long long)b * nn + (long long)i0 * N);
                for (int e4 = tw; e4 < R * N / 4; e4 += 256) {
                    const f32x4 h = Hr[e4];
                    const int kk = (4 * e4) / N, jj = 4 * e4 - kk * N;
                    const float x0 = xs[i0 + kk];
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = trace_rule(h[e], x0, y0s[jj + e], eta, one_m_eta, rule);
                    Hnr[e4] = o;
                }
            }
        }
    }
}

}  // namespace pu
