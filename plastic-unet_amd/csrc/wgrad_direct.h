// Weight gradients on the VALU: the single-channel stem, pointwise and small-channel kernels.
// Part of wgrad.hip, which includes it once, after its parameter block and shared helpers.
#pragma once

namespace pu {

// ------------------------------------------------------- single-channel stem weight gradient
// dW[n][tap] = sum_m dZ[m][n] x[m + tap] and db[n] = sum_m dZ[m][n] for the 1 -> N stem conv
// (inc.c0): the layer is the read of dZ (N channels per pixel).  Blocks sweep 16 x 64 pixel tiles
// (grid-stride) with the 1-channel halo staged in LDS; lanes in groups of N/4 per pixel, each lane
// 4 output channels x (9 taps + bias) accumulators over its pixels (dZ float4 loads: a
// wave-instruction reads 4 pixels x N channels contiguously); the block's groups are summed in
// fixed order through LDS into slab row [block][n][0..9] and the fixed-order split reduction
// finishes - deterministic like every other weight gradient.
constexpr int SWS_TH = 16, SWS_TW = 64;

// BF16ROWS (pu_wgrad_args.math == 2): dZ is a bf16 NHWC tensor, widened exactly on load (the bf16
// trunk's stem: no fp32 copy of dZ), otherwise the same fmaf chains
template <int N, bool BF16ROWS = false>
__global__ __launch_bounds__(256) void wgrad_stem_kernel(const WgradParams p) {
    constexpr int L = N / 4, PG = 256 / L;
    constexpr int HH = SWS_TH + 2, HW = SWS_TW + 2;
    constexpr int RED = PG * 10 * N;
    __shared__ __attribute__((aligned(16))) float smem[RED > HH * HW ? RED : HH * HW];
    const int tid = threadIdx.x;
    const int lane_c = tid % L, grp = tid / L;
    float acc[10][4];
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
    const int ntiles = p.batch * p.tiles_h * p.tiles_w;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int txi = t % p.tiles_w;
        const int tyi = (t / p.tiles_w) % p.tiles_h;
        const int b = t / (p.tiles_w * p.tiles_h);
        const int y0 = tyi * SWS_TH - 1, x0 = txi * SWS_TW - 1;
        const long long img = (long long)b * p.Hi * p.Wi;
        __syncthreads();                       // the previous tile's readers are done
        for (int e = tid; e < HH * HW; e += 256) {
            const int hy = e / HW, hx = e - hy * HW;
            const int gy = y0 + hy, gx = x0 + hx;
            smem[e] = ((unsigned)gy < (unsigned)p.Hi && (unsigned)gx < (unsigned)p.Wi)
                          ? p.src0[img + (long long)gy * p.Wi + gx] : 0.f;
        }
        __syncthreads();
        // 4 pixels per pass, their dZ loads issued together (unconditional: a pixel past the image
        // edge loads pixel 0 and adds nothing), so the loop waits once per 4 loads
        static_assert((SWS_TH * SWS_TW) % (4 * PG) == 0, "stem wgrad pass");
        for (int q0 = grp; q0 < SWS_TH * SWS_TW; q0 += 4 * PG) {
            f32x4 dzs[4];
            bool ok[4];
            int hb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * PG;
                const int row = q / SWS_TW, col = q - row * SWS_TW;
                const int oy = tyi * SWS_TH + row, ox = txi * SWS_TW + col;
                ok[u] = oy < p.Ho && ox < p.Wo;
                hb[u] = row * HW + col;
                const long long m = ok[u] ? ((long long)b * p.Ho + oy) * p.Wo + ox : 0;
                if constexpr (BF16ROWS) {
                    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
                    const bf16x4_t zb = *reinterpret_cast<const bf16x4_t*>(reinterpret_cast<const __bf16*>(p.P) + m * N + 4 * lane_c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dzs[u][e] = (float)zb[e];
                } else {
                    dzs[u] = *reinterpret_cast<const f32x4*>(p.P + m * N + 4 * lane_c);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                const f32x4 dz = dzs[u];
#pragma unroll
                for (int t9 = 0; t9 < 9; ++t9) {
                    const float a = smem[hb[u] + (t9 / 3) * HW + t9 % 3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t9][e] = fmaf(a, dz[e], acc[t9][e]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[9][e] += dz[e];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) smem[(grp * 10 + k) * N + 4 * lane_c + e] = acc[k][e];
    __syncthreads();
    float* slab = p.slab + (long long)blockIdx.x * p.Nr * p.Kcp;
    for (int idx = tid; idx < 10 * N; idx += 256) {
        const int k = idx / N, n = idx - k * N;
        float v = 0.f;
        for (int g = 0; g < PG; ++g) v += smem[(g * 10 + k) * N + n];
        slab[(long long)n * p.Kcp + k] = v;   // k = tap (C = 1); k = 9 = K: the bias column
    }
}

// ------------------------------------------------------- pointwise (1x1) small weight gradient
// dW[n][c] = sum_m dZ[m][n] X[m][c] and db[n] = sum_m dZ[m][n] for a 1x1 / s1 / p0 conv with a
// handful of channels (config C4's CoordConv 1x1: 4 -> 8 channels at 256^2, 2.1 M pixels).  As a
// GEMM it is K = 4: the tiled kernel spent 85 latency-bound 16-row stages per block on it (155 us
// for 100 MB); here a thread streams whole pixels (C + N floats, consecutive pixels on consecutive
// lanes) and keeps all N x (C + 1) sums in registers, fmaf chains in pixel order.  The block's 256
// chains reduce in a fixed butterfly (xor 32 .. 1) then wave order, one slab row per block; the
// fixed-order split reduction finishes it - deterministic.
template <int C, int N>
__global__ __launch_bounds__(256) void wgrad_pw_kernel(const WgradParams p) {
    constexpr int V = N * (C + 1);                // C weights + the bias per output channel
    __shared__ float part[4][V];
    const int tid = threadIdx.x;
    float acc[N][C + 1];
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int c = 0; c <= C; ++c) acc[n][c] = 0.f;
    const long long m0 = (long long)blockIdx.x * p.mps;
    const long long m1 = min((long long)p.M, m0 + p.mps);
    for (long long m = m0 + tid; m < m1; m += 256) {
        float x[C], g[N];
        if constexpr (C % 4 == 0) {
#pragma unroll
            for (int q = 0; q < C / 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(p.src0 + m * C + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[4 * q + e] = v[e];
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = p.src0[m * C + c];
        }
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p.P + m * N + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[4 * q + e] = v[e];
        }
#pragma unroll
        for (int n = 0; n < N; ++n) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[n][c] = fmaf(g[n], x[c], acc[n][c]);
            acc[n][C] += g[n];
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int c = 0; c <= C; ++c) {
            float v = acc[n][c];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) part[wave][n * (C + 1) + c] = v;
        }
    __syncthreads();
    float* slab = p.slab + (long long)blockIdx.x * p.Nr * p.Kcp;
    for (int i = tid; i < V; i += 256) {
        const float v = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
        const int n = i / (C + 1), c = i - n * (C + 1);
        if (c < C) slab[(long long)n * p.Kcp + c] = v;
        else if (p.bias_mode == 1) slab[(long long)n * p.Kcp + p.K] = v;
    }
}

// ------------------------------------------------------------- small-channel weight gradient
// 3x3/s1/p1 with C <= 16 input and N <= 16 output channels (configs C4/C5's 8/16-channel levels):
// a GEMM with N, K this small wastes most of an MFMA tile, so each block sweeps 16 x 32 pixel
// tiles (grid-stride), stages the input halo and the gradient tile in LDS, and accumulates
// dW[n][tap][c] on the VALU: thread items = (tap, 4 output x 4 input channels) plus bias items
// (4 output channels), replicated over pixel groups when the items do not fill the block.  The
// block's partial goes to slab row [block][n][tap*C + c] (bias at column K) and the fixed-order
// fp64 split reduction below finishes it - deterministic like the GEMM path.
constexpr int SW_TH = 16, SW_TW = 32;

// 4x4 outer-product accumulate of 4 output channels g (x) 4 input channels x: channel pairs on
// v_pk_fma_f32 (one rounding per element, as fmaf)
__device__ __forceinline__ void sw_fma44(f32x2 (&a)[4][2], const f32x4& g, const f32x4& x) {
    const f32x2 xa = {x[0], x[1]}, xb = {x[2], x[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 gg = {g[i], g[i]};
        a[i][0] = __builtin_elementwise_fma(gg, xa, a[i][0]);
        a[i][1] = __builtin_elementwise_fma(gg, xb, a[i][1]);
    }
}

template <int C, int N>
__global__ __launch_bounds__(256) void wgrad_small_kernel(const WgradParams p) {
    constexpr int HH = SW_TH + 2, HWD = SW_TW + 2;
    constexpr int CP = (C + 3) & ~3, C4 = CP / 4, N4 = N / 4;
    // weight items: (tap row r, 4 output x 4 input channels) with the 3 taps of the row, plus
    // bias items (4 output channels)
    constexpr int RT = 3;                                 // taps per item
    constexpr int WITEMS = 3 * N4 * C4;
    constexpr int ITEMS = WITEMS + N4;
    // LDS bank conflicts (64 banks: a ds_read_b128 serves 16 lanes per cycle): a group's items
    // padded to a multiple of 16 lanes keeps each 16-lane phase inside one pixel group, and a
    // halo row pitch of HWD + 1 pixels puts the 3 tap rows x input-channel quads on distinct banks
    // (C = 8: chunk offsets {0,1,6,7,12,13}; C = 16: {0..3, 12..15, 8..11})
    constexpr int ITEMS_P = ITEMS >= 12 ? (ITEMS + 15) / 16 * 16 : ITEMS;
    constexpr int HWP = HWD + 1;
    constexpr int GROUPS = 256 / ITEMS_P;
    static_assert(GROUPS >= 1, "items");
    constexpr int ACC = RT * 16;
    constexpr int HALO = HH * HWP * CP, GT = SW_TH * SW_TW * N;
    constexpr int SMEM = (HALO + GT) > (GROUPS * ITEMS * ACC) ? (HALO + GT) : (GROUPS * ITEMS * ACC);
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float* halo = smem;
    float* gt = smem + HALO;

    const int tid = threadIdx.x;
    const int item = tid % ITEMS_P, grp = tid / ITEMS_P;
    const bool active = grp < GROUPS && item < ITEMS;
    const bool wi = item < WITEMS;
    int tr = 0, co4 = 0, ci4 = 0;                          // tr: tap row
    if (wi) {
        tr = item / (N4 * C4);
        const int rem = item - tr * (N4 * C4);
        co4 = rem / C4;
        ci4 = rem - co4 * C4;
    } else {
        co4 = item - WITEMS;
    }
    f32x2 acc[RT][4][2];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i][0] = acc[t][i][1] = f32x2{0.f, 0.f};

    const int ntiles = p.batch * p.tiles_h * p.tiles_w;
    // the tile's halo and gradient rows are loaded into registers one tile ahead (all loads of a
    // tile in flight at once), stored to LDS between two barriers, and the next tile's loads then
    // fly under this tile's accumulation
    constexpr int NH = HH * HWD * C4, NG = SW_TH * SW_TW * N4;
    constexpr int PH = (NH + 255) / 256, PG2 = (NG + 255) / 256;
    f32x4 rh[PH], rg[PG2];
    auto load_tile = [&](int t) {
        const int txi = t % p.tiles_w;
        const int tyi = (t / p.tiles_w) % p.tiles_h;
        const int b = t / (p.tiles_w * p.tiles_h);
        const int y0 = tyi * SW_TH, x0 = txi * SW_TW;
        const long long img = (long long)b * p.Hi * p.Wi;
#pragma unroll
        for (int it = 0; it < PH; ++it) {
            const int e = it * 256 + tid;
            const int q = e % C4, pix = e / C4;
            const int hx = pix % HWD, hy = pix / HWD;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < NH && (unsigned)gy < (unsigned)p.Hi && (unsigned)gx < (unsigned)p.Wi) {
                const long long px = img + (long long)gy * p.Wi + gx;
                if (C % 4 == 0 && p.c0 % 4 == 0) {
                    const int c = 4 * q;
                    v = c < p.c0 ? *reinterpret_cast<const f32x4*>(p.src0 + px * p.c0 + c)
                                 : *reinterpret_cast<const f32x4*>(p.src1 + px * p.c1 + (c - p.c0));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = 4 * q + k;
                        if (c < C) v[k] = c < p.c0 ? p.src0[px * p.c0 + c] : p.src1[px * p.c1 + (c - p.c0)];
                    }
                }
            }
            rh[it] = v;
        }
#pragma unroll
        for (int it = 0; it < PG2; ++it) {
            const int e = it * 256 + tid;
            const int q = e % N4, pix = e / N4;
            const int oy = y0 + pix / SW_TW, ox = x0 + pix % SW_TW;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < NG && oy < p.Ho && ox < p.Wo)
                v = *reinterpret_cast<const f32x4*>(p.P + ((long long)(b * p.Ho + oy) * p.Wo + ox) * N + 4 * q);
            rg[it] = v;
        }
    };
    if ((int)blockIdx.x < ntiles) load_tile(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();                       // previous tile's readers are done
#pragma unroll
        for (int it = 0; it < PH; ++it) {
            const int e = it * 256 + tid;
            if (e < NH) {
                const int pix = e / C4, hy = pix / HWD, hx = pix - hy * HWD;
                *reinterpret_cast<f32x4*>(halo + (hy * HWP + hx) * CP + 4 * (e % C4)) = rh[it];
            }
        }
#pragma unroll
        for (int it = 0; it < PG2; ++it) {
            const int e = it * 256 + tid;
            if (e < NG) *reinterpret_cast<f32x4*>(gt + (e / N4) * N + 4 * (e % N4)) = rg[it];
        }
        if (t + (int)gridDim.x < ntiles) load_tile(t + gridDim.x);
        __syncthreads();
        if (active) {
            // 4 consecutive output pixels x the row's 3 taps: 4 gradient + 6 halo reads per
            // 192 fmas (the per-tap form: 2 reads per 16)
            constexpr int QW = SW_TW / 4;
            for (int pq = grp; pq < SW_TH * QW; pq += GROUPS) {
                const int row = pq / QW, col0 = (pq - row * QW) * 4;
                f32x4 g[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    g[u] = *reinterpret_cast<const f32x4*>(gt + (row * SW_TW + col0 + u) * N + 4 * co4);
                if (wi) {
                    f32x4 x[6];
#pragma unroll
                    for (int v = 0; v < 6; ++v)
                        x[v] = *reinterpret_cast<const f32x4*>(halo + ((row + tr) * HWP + col0 + v) * CP + 4 * ci4);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int s3 = 0; s3 < RT; ++s3) sw_fma44(acc[s3], g[u], x[u + s3]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[0][0][0] += f32x2{g[u][0], g[u][1]};
                        acc[0][0][1] += f32x2{g[u][2], g[u][3]};
                    }
                }
            }
        }
    }
    // fixed-order reduction over the pixel groups, then this block's slab rows
    __syncthreads();
    if (active) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    smem[(grp * ITEMS + item) * ACC + t * 16 + i * 4 + 2 * h] = acc[t][i][h][0];
                    smem[(grp * ITEMS + item) * ACC + t * 16 + i * 4 + 2 * h + 1] = acc[t][i][h][1];
                }
    }
    __syncthreads();
    if (tid < ITEMS) {
        float* slab = p.slab + (long long)blockIdx.x * p.Nr * p.Kcp;
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = 0.f;
            for (int g = 0; g < GROUPS; ++g)
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] += smem[(g * ITEMS + tid) * ACC + t * 16 + e];
            if (tid < WITEMS) {
                const int tap = 3 * tr + t;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 4 * ci4 + j;
                        if (c < C) slab[(long long)(4 * co4 + i) * p.Kcp + tap * C + c] = v[i * 4 + j];
                    }
            } else if (t == 0 && p.bias_mode == 1) {   // column K exists only with a bias (Kc = K + 1)
#pragma unroll
                for (int i = 0; i < 4; ++i) slab[(long long)(4 * co4 + i) * p.Kcp + p.K] = v[i];
            }
        }
    }
}

}  // namespace pu
