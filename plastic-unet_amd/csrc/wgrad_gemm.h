// Weight gradients as tiled GEMMs: the register-staged, direct-to-LDS (DMA) and bf16 tile kernels.
// Part of wgrad.hip, which includes it once, after its parameter block and shared helpers.
#pragma once

namespace pu {

template <int BN, int BK, int WN, int WK, bool QVEC>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
    constexpr int FN = BN / WN / 32;
    constexpr int FK = BK / WK / 32;
    constexpr int P_PER_ROW = BN / 4;               // float4 per P row
    constexpr int P_LD = (WG_BM * P_PER_ROW) / 256;  // float4 loads per thread
    constexpr int Q_PER_ROW = BK / 4;
    constexpr int Q_LD = (WG_BM * Q_PER_ROW) / 256;
    static_assert(WN * WK == 4, "4 waves");
    static_assert(P_LD >= 1 && Q_LD >= 1, "tile too small for 256 threads");

    __shared__ __attribute__((aligned(16))) float lds[2 * WG_BM * (BN + BK)];
    float* Ps = lds;
    float* Qs = lds + 2 * WG_BM * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> scalar math
    const int wn = wave % WN, wk = wave / WN;
    const int lr = lane & 31, lh = lane >> 5;
    // wgrad_block written out: through the helper the 64 x 64 tile takes two more SGPRs
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = tile % p.gx;
    const int tyz = tile / p.gx;
    const int ty = tyz % p.gy;
    const int tz = tyz / p.gy;
    const int n_blk = ty * BN;
    const int k_blk = tx * BK;
    const int m_begin = tz * p.mps;
    const int m_end = min(p.M, m_begin + p.mps);

    // ---- fixed per-thread P columns
    const int p_col = (tid % P_PER_ROW) * 4;
    const int p_row = tid / P_PER_ROW;               // + i * (256 / P_PER_ROW)
    const int pn = n_blk + p_col;
    // ---- fixed per-thread Q columns: tap offsets and channel
    const int q_col = (tid % Q_PER_ROW) * 4;
    const int q_row = tid / Q_PER_ROW;               // + i * (256 / Q_PER_ROW)
    int q_r[4], q_s[4], q_c[4];
    bool q_ok[4], q_one[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // QVEC: the four columns share one tap (C % 4 == 0), so only element 0 is decoded
        const int k = k_blk + q_col + e;
        q_ok[e] = k < p.K;
        q_one[e] = (p.bias_mode == 1) && k == p.K;
        const int kk = q_ok[e] ? k : 0;
        const int tap = fdiv(kk, p.dC);
        q_c[e] = kk - tap * p.C;
        q_r[e] = fdiv(tap, p.dKw);
        q_s[e] = tap - q_r[e] * p.kw;
        if (QVEC) break;
    }

    f32x4 rp[P_LD], rq[Q_LD];
    auto load_stage = [&](int m0) {
#pragma unroll
        for (int i = 0; i < P_LD; ++i) {
            int m = m0 + p_row + i * (256 / P_PER_ROW);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                if (pn + 3 < p.N) {
                    v = *reinterpret_cast<const f32x4*>(p.P + (long long)m * p.N + pn);
                } else if (p.bias_mode == 2 && pn == p.N) {
                    v[0] = 1.f;
                }
            }
            rp[i] = v;
        }
        // Q rows: the wave's first row is uniform (decomposed on the scalar unit); lanes add a
        // small row delta (0 .. 64/Q_PER_ROW - 1) with carry into ho / b.
        constexpr int QR_PER_WAVE = 64 / Q_PER_ROW;
        const int q_delta = lane / Q_PER_ROW;
#pragma unroll
        for (int i = 0; i < Q_LD; ++i) {
            const int mu = m0 + wave * QR_PER_WAVE + i * (256 / Q_PER_ROW);
            const int tu = fdiv(mu, p.dWo);
            const int wou = mu - tu * p.Wo;
            const int bu = fdiv(tu, p.dHo);
            const int hou = tu - bu * p.Ho;
            const int m = mu + q_delta;
            int wo = wou + q_delta, ho = hou, b = bu;
            while (wo >= p.Wo) {
                wo -= p.Wo;
                if (++ho >= p.Ho) { ho = 0; ++b; }
            }
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                long long pb = (long long)b * p.Hi * p.Wi;
                int hb = ho * p.stride - p.pad, wb = wo * p.stride - p.pad;
                if (QVEC) {
                    if (q_ok[0]) {
                        int hi = hb + q_r[0], wi = wb + q_s[0];
                        if ((unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) {
                            long long pix = pb + hi * p.Wi + wi;
                            int c = q_c[0];
                            const float* src = c < p.c0 ? p.src0 + pix * p.c0 + c : p.src1 + pix * p.c1 + (c - p.c0);
                            v = *reinterpret_cast<const f32x4*>(src);
                        }
                    } else if (q_one[0]) {
                        v[0] = 1.f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (q_ok[e]) {
                            int hi = hb + q_r[e], wi = wb + q_s[e];
                            if ((unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) {
                                long long pix = pb + hi * p.Wi + wi;
                                int c = q_c[e];
                                v[e] = c < p.c0 ? p.src0[pix * p.c0 + c] : p.src1[pix * p.c1 + (c - p.c0)];
                            }
                        } else if (q_one[e]) {
                            v[e] = 1.f;
                        }
                    }
                }
            }
            rq[i] = v;
        }
    };
    auto store_stage = [&](int buf) {
        float* ps = Ps + buf * WG_BM * BN;
        float* qs = Qs + buf * WG_BM * BK;
#pragma unroll
        for (int i = 0; i < P_LD; ++i)
            *reinterpret_cast<f32x4*>(ps + (p_row + i * (256 / P_PER_ROW)) * BN + p_col) = rp[i];
#pragma unroll
        for (int i = 0; i < Q_LD; ++i)
            *reinterpret_cast<f32x4*>(qs + (q_row + i * (256 / Q_PER_ROW)) * BK + q_col) = rq[i];
    };

    f32x16 acc[FN][FK];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FK; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int a_col0 = wn * (BN / WN) + lr;
    const int b_col0 = wk * (BK / WK) + lr;

    if (m_begin < m_end) {
        load_stage(m_begin);
        store_stage(0);
    }
    __syncthreads();
    int buf = 0;
    for (int m0 = m_begin; m0 < m_end; m0 += WG_BM) {
        const bool more = m0 + WG_BM < m_end;
        if (more) load_stage(m0 + WG_BM);
        const float* ps = Ps + buf * WG_BM * BN;
        const float* qs = Qs + buf * WG_BM * BK;
#pragma unroll
        for (int ks = 0; ks < WG_BM / 2; ++ks) {
            float fa[FN], fb[FK];
            const int row = ks * 2 + lh;
#pragma unroll
            for (int i = 0; i < FN; ++i) fa[i] = ps[row * BN + a_col0 + i * 32];
#pragma unroll
            for (int j = 0; j < FK; ++j) fb[j] = qs[row * BK + b_col0 + j * 32];
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int j = 0; j < FK; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // ---- partial tile -> slab[z][n][k]
    float* slab = p.slab + (long long)tz * p.Nr * p.Kcp;
#pragma unroll
    for (int i = 0; i < FN; ++i) {
#pragma unroll
        for (int j = 0; j < FK; ++j) {
            const int k = k_blk + b_col0 + j * 32;
            if (k >= p.Kc) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n_blk + wn * (BN / WN) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (n < p.Nr) slab[(long long)n * p.Kcp + k] = acc[i][j][r];
            }
        }
    }
}

// ------------------------------------------------------------------------ direct-to-LDS variant
// C % 4 == 0: P and Q tiles are fetched with global_load_lds_dwordx4 into row-major LDS images
// ([16 rows][BN] and [16 rows][BK]); the MFMA operands are ds_read_b32 of 32 consecutive floats
// per half-wave (conflict-free).  Padding / out-of-image taps read a zero page.  Roles are
// transposed (Q as the A operand) so each lane owns 4 consecutive k of one n and the partial tile
// is stored as float4 into a Kcp-strided slab.  The bias is not an extra GEMM column/row (that
// costs a whole extra tile whenever K or N is a multiple of the tile): the k-tile-0 blocks
// (mode 1) or n-tile-0 blocks (mode 2) column-sum the staged P / Q image out of LDS on the VALU
// and write the partial into slab column K / row N.

// 8 fp32 values -> their exact 3-term bf16 split.  split3_pairs' operations in the same order, but
// with the residuals as scalar subtractions: written with the packed subtraction of split3_pair,
// the X6 DMA tiles below compile to a different mix of v_add_f32 and v_pk_add_f32, so their copy
// stays in the form they were tuned with.
__device__ __forceinline__ void wg_split3(const float (&x)[8], bf16x8_t& h, bf16x8_t& m, bf16x8_t& l) {
#pragma clang fp contract(off)
    u32x4_t hv, mv, lv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float x0 = x[2 * q], x1 = x[2 * q + 1];
        const unsigned a = pk_bf16(f32x2{x0, x1});
        const float r0 = x0 - __builtin_bit_cast(float, a << 16);
        const float r1 = x1 - __builtin_bit_cast(float, a & 0xffff0000u);
        const unsigned b = pk_bf16(f32x2{r0, r1});
        const float l0 = r0 - __builtin_bit_cast(float, b << 16);
        const float l1 = r1 - __builtin_bit_cast(float, b & 0xffff0000u);
        hv[q] = a;
        mv[q] = b;
        lv[q] = pk_bf16(f32x2{l0, l1});
    }
    h = __builtin_bit_cast(bf16x8_t, hv);
    m = __builtin_bit_cast(bf16x8_t, mv);
    l = __builtin_bit_cast(bf16x8_t, lv);
}

// X6: the 16 staged pixel rows are one k-step of v_mfma_f32_32x32x16_bf16 and each fp32 product
// is 6 exact bf16 products (hi/mid/lo split, fp32 accumulation) - 6 x 32 cycles against the
// 8 x 64 of v_mfma_f32_32x32x2_f32; lane (i, h) reads rows 8h..8h+7 of its column.
// NW waves (WN x WK): 6 waves give the 64 x 576 tile of the 64-channel layers (K = 9 x 64 or
// 9 x 128 with no padding, 64 x 96 per wave: 5 operand splits per 36 MFMAs); the P pieces that do
// not divide among the waves are issued by every wave anyway (the counted wait stays uniform),
// the surplus ones reading the zero page into a 1 KB sink.
// FQ: stride 1, same-size input (Hi == Ho, Wi == Wo >= 4) - a Q lane's source row is its output
// pixel m shifted by the tap, so the per-stage address is one scalar product plus per-lane
// constants, and the lane's (ho, wo) advance by compare-and-wrap (row delta < 4 < Wo) instead of
// the per-lane divisions of the general path.
template <int BN, int BK, int WN, int WK, int NBUF, bool X6, int NW = 4, bool FQ = false>
__global__ __launch_bounds__(NW * 64) void wgrad_dma_kernel(const WgradParams p) {
    constexpr int FN = BN / WN / 32;
    constexpr int FK = BK / WK / 32;
    constexpr int P_ROWS = 256 / BN;              // rows per 1 KB glds instruction
    constexpr int P_TOT = WG_BM / P_ROWS;         // P glds per stage
    constexpr int P_LD = (P_TOT + NW - 1) / NW;   // per wave (surplus -> sink)
    constexpr int Q_LD = WG_BM * BK / 256 / NW;   // Q instructions may straddle rows (BK = 192)
    constexpr int G = P_LD + Q_LD;
    constexpr int STAGE = WG_BM * (BN + BK);
    constexpr int SINK = (P_TOT % NW) ? 256 : 0;
    static_assert(WN * WK == NW && P_LD >= 1 && Q_LD >= 1 && 256 % BN == 0 && (WG_BM * BK) % (256 * NW) == 0, "tile");

    __shared__ __attribute__((aligned(16))) float lds[NBUF * STAGE + SINK];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WN, wk = wave / WN;
    const int lr = lane & 31, lh = lane >> 5;
    const WgradBlock blk = wgrad_block(p);
    const int tx = blk.tx, ty = blk.ty, tz = blk.tz, m_begin = blk.m_begin, m_end = blk.m_end;
    const int n_blk = ty * BN;
    const int k_blk = tx * BK;

    // P lane geometry: column n (fixed), row delta within the instruction
    const int p_col = (lane % (BN / 4)) * 4;
    const int p_dr = lane / (BN / 4);
    const int pn = n_blk + p_col;
    const bool p_in = pn < p.N;
    // Q lane geometry per instruction j: image float offset (wave*Q_LD + j)*256 + 4*lane ->
    // (uniform first row q_row0, lane row delta, column k -> tap offsets and channel)
    int q_row0[Q_LD], q_dr[Q_LD], q_r[Q_LD], q_s[Q_LD], q_cs[Q_LD];
    const float* q_ptr[Q_LD];
#pragma unroll
    for (int j = 0; j < Q_LD; ++j) {
        const int base = (wave * Q_LD + j) * 256;
        const int off = base + 4 * lane;
        q_row0[j] = base / BK;
        q_dr[j] = off / BK - q_row0[j];
        const int qk = k_blk + off % BK;
        q_r[j] = 0; q_s[j] = 0; q_cs[j] = 0; q_ptr[j] = nullptr;
        if (qk < p.K) {
            const int tap = fdiv(qk, p.dC);
            const int c = qk - tap * p.C;
            q_r[j] = fdiv(tap, p.dKw);
            q_s[j] = tap - q_r[j] * p.kw;
            const bool first = c < p.c0;
            q_ptr[j] = first ? p.src0 + c : p.src1 + (c - p.c0);
            q_cs[j] = first ? p.c0 : p.c1;
        }
    }
    // FQ lane constants: source = q_ptr + (m + dr + (r - pad) * Wi + (s - pad)) * cs
    const float* q_fb[FQ ? Q_LD : 1];
    bool q_first[FQ ? Q_LD : 1];
    if constexpr (FQ) {
#pragma unroll
        for (int j = 0; j < Q_LD; ++j) {
            q_first[j] = q_cs[j] == p.c0;
            q_fb[j] = q_ptr[j] ? q_ptr[j] + (long long)(q_dr[j] + (q_r[j] - p.pad) * p.Wi + (q_s[j] - p.pad)) * q_cs[j]
                               : g_wg_zero16;
            q_r[j] -= p.pad;
            q_s[j] -= p.pad;
        }
    }
    const float* p_lane = p.P + (long long)p_dr * p.N + pn;

    auto issue = [&](int m0, int slot) {
        float* ps = lds + slot * STAGE;
        float* qs = ps + WG_BM * BN;
#pragma unroll
        for (int j = 0; j < P_LD; ++j) {
            const int I = (P_TOT % NW) ? wave + NW * j : wave * P_LD + j;
            const int row0 = I * P_ROWS;
            const int m = m0 + row0 + p_dr;
            const float* g = g_wg_zero16;
            float* dst = ps + row0 * BN;
            if (SINK && I >= P_TOT) dst = lds + NBUF * STAGE;
            else if (m < m_end && p_in) g = p_lane + (long long)(m0 + row0) * p.N;
            __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)dst, 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < Q_LD; ++j) {
            const int mu = m0 + q_row0[j];   // wave-uniform: decomposed on the scalar unit
            const int tu = fdiv(mu, p.dWo);
            const int wou = mu - tu * p.Wo;
            const int bu = fdiv(tu, p.dHo);
            const int hou = tu - bu * p.Ho;
            if constexpr (FQ) {
                int wo = wou + q_dr[j];
                const bool cw = wo >= p.Wo;
                wo = cw ? wo - p.Wo : wo;
                int ho = hou + (cw ? 1 : 0);
                ho = ho >= p.Ho ? ho - p.Ho : ho;
                const int hi = ho + q_r[j], wi = wo + q_s[j];
                const bool ok = mu + q_dr[j] < m_end && q_ptr[j] && (unsigned)hi < (unsigned)p.Hi &&
                                (unsigned)wi < (unsigned)p.Wi;
                const long long mo = q_first[j] ? (long long)mu * p.c0 : (long long)mu * p.c1;
                const float* g = ok ? q_fb[j] + mo : g_wg_zero16;
                __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(qs + (wave * Q_LD + j) * 256), 16, 0, 0);
                continue;
            }
            // lane delta with carry, branch-free (keeps the main loop one basic block)
            int wo = wou + q_dr[j];
            const int cw = fdiv(wo, p.dWo);
            wo -= cw * p.Wo;
            int ho = hou + cw;
            const int ch = fdiv(ho, p.dHo);
            ho -= ch * p.Ho;
            const int b = bu + ch;
            const float* g = g_wg_zero16;
            if (mu + q_dr[j] < m_end && q_ptr[j]) {
                const int hi = ho * p.stride - p.pad + q_r[j], wi = wo * p.stride - p.pad + q_s[j];
                if ((unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi)
                    g = q_ptr[j] + ((long long)b * p.Hi * p.Wi + (long long)hi * p.Wi + wi) * q_cs[j];
            }
            __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(qs + (wave * Q_LD + j) * 256), 16, 0, 0);
        }
    };

    f32x16 acc[FK][FN];
#pragma unroll
    for (int i = 0; i < FK; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int a_col0 = wn * (BN / WN) + lr;   // n columns this lane reads from P
    const int b_col0 = wk * (BK / WK) + lr;   // k columns this lane reads from Q
    const int T = (m_end > m_begin) ? (m_end - m_begin + WG_BM - 1) / WG_BM : 0;

    // bias column sums (block-uniform role): mode 1 sums P columns in k-tile 0, mode 2 Q columns in n-tile 0
    const int bias_w = (p.bias_mode == 1 && tx == 0) ? BN : (p.bias_mode == 2 && ty == 0) ? BK : 0;
    float bsum = 0.f;

    // every iteration issues one stage (past m_end: zero page), so the counted wait is constant
#pragma unroll
    for (int s0 = 0; s0 < NBUF - 1; ++s0) issue(m_begin + s0 * WG_BM, s0);

    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * G) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const float* ps = lds + (t % NBUF) * STAGE;
        const float* qs = ps + WG_BM * BN;
        if constexpr (X6) {
            float xa[FN][8], xb[FK][8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int row = 8 * lh + e;
#pragma unroll
                for (int j = 0; j < FN; ++j) xa[j][e] = ps[row * BN + a_col0 + j * 32];
#pragma unroll
                for (int i = 0; i < FK; ++i) xb[i][e] = qs[row * BK + b_col0 + i * 32];
            }
            bf16x8_t ph[FN], pm[FN], pl[FN];
#pragma unroll
            for (int j = 0; j < FN; ++j) wg_split3(xa[j], ph[j], pm[j], pl[j]);
#pragma unroll
            for (int i = 0; i < FK; ++i) {
                bf16x8_t qh, qm, ql;
                wg_split3(xb[i], qh, qm, ql);
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    acc[i][j] = mma6(qh, qm, ql, ph[j], pm[j], pl[j], acc[i][j]);
                }
                if (i == 0) issue(m_begin + (t + NBUF - 1) * WG_BM, (t + NBUF - 1) % NBUF);
            }
        } else {
        // the whole stage's operands up front ((FN+FK)*8 VGPRs): the reads of step ks+1.. land
        // under the MFMAs of step ks instead of a lgkmcnt(0) bubble before every step
        float fa[WG_BM / 2][FN], fb[WG_BM / 2][FK];
#pragma unroll
        for (int ks = 0; ks < WG_BM / 2; ++ks) {
            const int row = ks * 2 + lh;
#pragma unroll
            for (int j = 0; j < FN; ++j) fa[ks][j] = ps[row * BN + a_col0 + j * 32];
#pragma unroll
            for (int i = 0; i < FK; ++i) fb[ks][i] = qs[row * BK + b_col0 + i * 32];
        }
#pragma unroll
        for (int ks = 0; ks < WG_BM / 2; ++ks) {
#pragma unroll
            for (int i = 0; i < FK; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ks][i], fa[ks][j], acc[i][j], 0, 0, 0);
            // next stage's loads mid-stage: address arithmetic overlaps the MFMAs
            if (ks == 1) issue(m_begin + (t + NBUF - 1) * WG_BM, (t + NBUF - 1) % NBUF);
        }
        // pin the order the default scheduler undoes (it sinks each read next to its MFMA):
        // all operand reads of the stage, then the MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, (WG_BM / 2) * (FN + FK), 0);
        __builtin_amdgcn_sched_group_barrier(0x008, (WG_BM / 2) * FN * FK, 0);
        }
        // bias column sums after the MFMA block (a divergent branch here does not split it)
        if (tid < bias_w) {   // one column per thread, all rows of the stage
            const float* img = p.bias_mode == 1 ? ps : qs;
#pragma unroll
            for (int r = 0; r < WG_BM; ++r) bsum += img[r * bias_w + tid];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the past-the-end zero-page loads

    // partial tile -> slab[z][n][k] (row stride Kcp, float4 over 4 consecutive k); store_frag
    // written out: through the helper eight instantiations get other address instructions
    float* slab = p.slab + (long long)tz * p.Nr * p.Kcp;
    if (tid < bias_w) {
        if (p.bias_mode == 1) {
            const int n = n_blk + tid;
            if (n < p.N) slab[(long long)n * p.Kcp + p.K] = bsum;
        } else {
            const int k = k_blk + tid;
            if (k < p.K) slab[(long long)p.N * p.Kcp + k] = bsum;
        }
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n_blk + wn * (BN / WN) + j * 32 + lr;
        if (n >= p.N) continue;
#pragma unroll
        for (int i = 0; i < FK; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k_blk + wk * (BK / WK) + i * 32 + 8 * q + 4 * lh;
                if (k >= p.K) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                *reinterpret_cast<f32x4*>(slab + (long long)n * p.Kcp + k) = v;
            }
        }
    }
}

// swizzle of 16-byte chunks in 256-byte rows: conflict-free ds_read_b64_tr_b16
__device__ __forceinline__ int wb_sw(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// ------------------------------------------------------------------ bf16 weight gradient (C3)
// dW[n][k] = sum_m P[m][n] * Q[m][k] with bf16 P (dZ or ConvT input rows) and bf16 im2col Q,
// fp32 MFMA accumulation (v_mfma_f32_32x32x16_bf16), fp32 slab partials, the same fp64 split
// reduction.  The GEMM's k dimension is the pixel index m, so each MFMA operand lane needs 8
// consecutive pixel rows of one column: the stage images are row-major [32 pixel rows][128]
// bf16 (256-byte rows) read with ds_read_b64_tr_b16 (per 16-lane group: 4 rows x 16 columns,
// delivered column-major).  The 16-byte chunk ch of row r is stored at ch ^ sw(r),
// sw(r) = ((r&3)<<2) | ((r>>2)&3) (conflict-free transposed reads on 256-byte rows); glds cannot
// permute its LDS writes, so each lane fetches the global chunk that belongs at its position.

constexpr int WB_ROWS = 32;   // pixel rows per stage (2 MFMA k-steps)
constexpr int WB_W = 128;     // columns per image (BN = BK = 128)


__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const WgradBf16Params p) {
    constexpr int NBUF = 3;
    constexpr int LD = WB_ROWS * WB_W * 2 / 1024 / 4;   // glds per wave per image per stage (2)
    constexpr int G = 2 * LD;
    constexpr int IMG = WB_ROWS * WB_W;                 // bf16 elements per image
    constexpr int STAGE = 2 * IMG;
    __shared__ __attribute__((aligned(16))) __bf16 lds[NBUF * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wk = wave >> 1;            // 2 x 2 waves, 64 x 64 each
    const int lr = lane & 31, lh = lane >> 5;
    const WgradBlock blk = wgrad_block(p);
    const int tx = blk.tx, ty = blk.ty, tz = blk.tz, m_begin = blk.m_begin, m_end = blk.m_end;
    const int n_blk = ty * WB_W;
    const int k_blk = tx * WB_W;

    // loader geometry: instruction j (= wave*LD + jj) of an image covers rows 4j .. 4j+3; lane l
    // writes physical chunk l%16 of row 4j + l/16, i.e. logical chunk (l%16) ^ sw(row)
    const int lrow = lane >> 4;                          // row within the instruction
    int p_col[LD], q_r[LD], q_s[LD], q_cs[LD];
    const __bf16* q_ptr[LD];
    bool p_in[LD];
#pragma unroll
    for (int jj = 0; jj < LD; ++jj) {
        const int j = wave * LD + jj;
        const int ch = (lane & 15) ^ ((lrow << 2) | (j & 3));
        p_col[jj] = n_blk + 8 * ch;
        p_in[jj] = p_col[jj] < p.N;
        const int qk = k_blk + 8 * ch;
        q_r[jj] = 0; q_s[jj] = 0; q_cs[jj] = 0; q_ptr[jj] = nullptr;
        if (qk < p.K) {
            const int tap = fdiv(qk, p.dC);
            const int c = qk - tap * p.C;
            q_r[jj] = fdiv(tap, p.dKw);
            q_s[jj] = tap - q_r[jj] * p.kw;
            const bool first = c < p.c0;
            q_ptr[jj] = first ? p.src0 + c : p.src1 + (c - p.c0);
            q_cs[jj] = first ? p.c0 : p.c1;
        }
    }

    const __bf16* zero = reinterpret_cast<const __bf16*>(g_wg_zero16);
    auto issue = [&](int m0, int slot) {
        __bf16* ps = lds + slot * STAGE;
        __bf16* qs = ps + IMG;
#pragma unroll
        for (int jj = 0; jj < LD; ++jj) {
            const int j = wave * LD + jj;
            const int m = m0 + 4 * j + lrow;
            const __bf16* g = zero;
            if (m < m_end && p_in[jj]) g = p.P + (long long)m * p.N + p_col[jj];
            __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(ps + j * 512), 16, 0, 0);
        }
#pragma unroll
        for (int jj = 0; jj < LD; ++jj) {
            const int j = wave * LD + jj;
            const int mu = m0 + 4 * j;                   // wave-uniform
            const int tu = fdiv(mu, p.dWo);
            const int wou = mu - tu * p.Wo;
            const int bu = fdiv(tu, p.dHo);
            const int hou = tu - bu * p.Ho;
            int wo = wou + lrow;
            const int cw = fdiv(wo, p.dWo);
            wo -= cw * p.Wo;
            int ho = hou + cw;
            const int chh = fdiv(ho, p.dHo);
            ho -= chh * p.Ho;
            const int b = bu + chh;
            const __bf16* g = zero;
            if (mu + lrow < m_end && q_ptr[jj]) {
                const int hi = ho * p.stride - p.pad + q_r[jj], wi = wo * p.stride - p.pad + q_s[jj];
                if ((unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi)
                    g = q_ptr[jj] + ((long long)b * p.Hi * p.Wi + (long long)hi * p.Wi + wi) * q_cs[jj];
            }
            __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(qs + j * 512), 16, 0, 0);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addressing: 16-lane group g = lane>>4 covers columns 16*(g&1) + 0..15 and
    // rows 8*(g>>1) + (0..3 | 4..7) of a k-step; lane 4q+p of the group addresses row q, columns
    // 4p..4p+3 (logical chunk (p>>1), byte half (p&1))
    const int grp = lane >> 4, gq = (lane >> 2) & 3, gp = lane & 3;
    auto tr_addr = [&](int row, int col) {   // byte offset of (row, col) in a swizzled image
        return row * (WB_W * 2) + 16 * ((col >> 3) ^ wb_sw(row)) + 2 * (col & 7);
    };
    const int T = (m_end > m_begin) ? (m_end - m_begin + WB_ROWS - 1) / WB_ROWS : 0;
    const int bias_w = (p.bias_mode == 1 && tx == 0) ? 1 : (p.bias_mode == 2 && ty == 0) ? 2 : 0;
    float bsum = 0.f;

#pragma unroll
    for (int s0 = 0; s0 < NBUF - 1; ++s0) issue(m_begin + s0 * WB_ROWS, s0);

    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* pb = reinterpret_cast<const char*>(lds + (t % NBUF) * STAGE);
        const char* qb = pb + IMG * 2;
        bf16x8_t fa[2][2], fb[2][2];   // [kstep][frag]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int row0 = ks * 16 + 8 * (grp >> 1) + gq;
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const int ccol = 16 * (grp & 1) + 4 * gp;
                // A operand: Q^T rows = k columns of the Q image
                const int qc = wk * 64 + f * 32 + ccol;
                fa[ks][f] = tr_frag(qb, tr_addr(row0, qc), tr_addr(row0 + 4, qc));
                // B operand: P columns n
                const int pc = wn * 64 + f * 32 + ccol;
                fb[ks][f] = tr_frag(pb, tr_addr(row0, pc), tr_addr(row0 + 4, pc));
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i], fb[ks][j], acc[i][j], 0, 0, 0);
            if (ks == 0) issue(m_begin + (t + NBUF - 1) * WB_ROWS, (t + NBUF - 1) % NBUF);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        if (bias_w && tid < WB_W) {           // bias column sums: P columns (mode 1) / Q (mode 2)
            const char* img = bias_w == 1 ? pb : qb;
            for (int r = 0; r < WB_ROWS; ++r)
                bsum += (float)*reinterpret_cast<const __bf16*>(img + tr_addr(r, tid));
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    float* slab = p.slab + (long long)tz * p.Nr * p.Kcp;
    if (bias_w && tid < WB_W) {
        if (bias_w == 1) {
            const int n = n_blk + tid;
            if (n < p.N) slab[(long long)n * p.Kcp + p.K] = bsum;
        } else {
            const int k = k_blk + tid;
            if (k < p.K) slab[(long long)p.N * p.Kcp + k] = bsum;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n_blk + wn * 64 + j * 32 + lr;
        if (n >= p.N) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            store_frag<true>(slab + (long long)n * p.Kcp, acc[i][j], k_blk + wk * 64 + i * 32 + 4 * lh, p.K);
    }
}

}  // namespace pu
