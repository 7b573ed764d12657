// Weight gradients of 3x3 / s1 convolutions with halo reuse: the 6-product and the bf16 kernel.
// Part of wgrad.hip, which includes it once, after its parameter block and shared helpers.
#pragma once

namespace pu {

// ------------------------------------------ 6-product weight gradient with halo reuse (3x3/s1)
// dW[n][tap][c] = sum_m dZ[m][n] * X[m + tap][c].  A stage is 16 consecutive output pixels of one
// image row; the 9 taps read only the 3 x 18 halo pixels around them, so the block loads and
// splits that halo ONCE (54 pixel rows x 64 channels, instead of 9 x 16 im2col rows) together
// with the 16 dZ rows (64 channels), writes the hi / mid / lo bf16 planes into LDS (row-major,
// 128-byte rows, 16-byte chunk ch of row r at ch ^ 4*((r >> 1) & 1): conflict-free transposed
// reads), and every wave reads its MFMA operands with ds_read_b64_tr_b16: tap (r, s) is the
// 16-row window starting at halo row 18 r + s.  Block tile: 64 output channels x 64 input
// channels x all 9 taps, 4 waves = (channel half, output half), each 9 accumulators (one per
// tap).  Raw fp32 rows arrive in registers one stage ahead (global_load_dwordx4; halo pixels
// outside the image are zero); the planes are double buffered, one barrier per stage.
// Requires stride 1, pad 1, 3x3, Hi == Ho, Wi == Wo, Wo % 16 == 0, c0 % 64 == c1 % 64 == 0,
// N % 64 == 0, bias_mode != 2, every source under 2^31 elements.
constexpr int HX_ROWS = 54;                   // halo pixel rows (3 x 18)
__device__ __forceinline__ int hx_off(int row, int col) {   // byte offset in a 64-column plane
    return row * 128 + 16 * ((col >> 3) ^ (((row >> 1) & 1) << 2)) + 2 * (col & 7);
}

// NT = 64-channel output tiles per block: NT = 1 is 4 waves (two blocks per CU); NT = 2 is 8 waves
// (one block per CU) sharing each loaded and split X halo between 128 output channels - half the
// X reads and splits per MFMA, 12 instead of 20 raw-row registers per thread.
template <int NT>
__global__ __launch_bounds__(256 * NT) void wgrad_halo_x6_kernel(const WgradParams p) {
    constexpr int NTH = 256 * NT;
    constexpr int RS = NTH / 16;              // halo rows per X group (16 NT: keeps the row swizzle)
    constexpr int XG = (HX_ROWS + RS - 1) / RS;   // X float4 groups per thread (864 = 3 x 256 + 96 | 512 + 352)
    constexpr int IMG = (HX_ROWS + 16 * NT) * 128;  // one plane: 54 X rows, then NT x 16 dZ rows
    __shared__ __attribute__((aligned(16))) char lds[2 * 3 * IMG];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ci = wave & 1, nj = (wave >> 1) & 1, nt = wave >> 2;
    const WgradBlock blk = wgrad_block(p);   // tx: 64-channel input tile, ty: 64-channel output tile
    const int tx = blk.tx, ty = blk.ty, tz = blk.tz, m_begin = blk.m_begin, m_end = blk.m_end;
    const int T = m_end > m_begin ? (m_end - m_begin) / 16 : 0;

    // ---- thread roles in the loads: column quad cq (fixed), halo pixel rows hp_i = tid/16 + RS i
    const int cq = tid & 15;
    const int c_lo = tx * 64;                 // first input channel of the tile
    const bool first = c_lo < p.c0;
    const float* xsrc = first ? p.src0 + c_lo : p.src1 + (c_lo - p.c0);
    const int cs = first ? p.c0 : p.c1;
    const float* x_lane[XG];
    unsigned x_cls[XG];                       // edge classes: 1 top, 2 bottom, 4 left, 8 right, 16 past the halo, 32 all
#pragma unroll
    for (int i = 0; i < XG; ++i) {
        const int hp = (tid >> 4) + RS * i;
        const int rr = hp / 18, cc = hp - rr * 18;
        x_lane[i] = xsrc + (long long)((rr - 1) * p.Wi + (cc - 1)) * cs + cq * 4;
        if (hp >= HX_ROWS) x_lane[i] = g_wg_zero16;   // rows past the halo: class 16 -> zero page, never stored
        x_cls[i] = 32u | (hp >= HX_ROWS ? 16u
                                        : ((rr == 0 ? 1u : 0u) | (rr == 2 ? 2u : 0u) | (cc == 0 ? 4u : 0u) | (cc == 17 ? 8u : 0u)));
    }
    // dZ roles: row prow of the stage, channel quad pq of the block's 64 NT output channels
    const int pq = tid % (16 * NT), prow = tid / (16 * NT);
    const float* p_lane = p.P + (long long)prow * p.N + ty * 64 * NT + pq * 4;

    f32x4 rx[XG], rp;
    auto load = [&](int t) {                  // raw rows of stage t into registers (branch-free:
        const int m0 = m_begin + 16 * t;      // out-of-image halo pixels read the zero page)
        const int tu = fdiv(m0, p.dWo);
        const int wo0 = m0 - tu * p.Wo;
        const int bu = fdiv(tu, p.dHo);
        const int ho = tu - bu * p.Ho;
        const bool live = t < T;
        // a stage past the split's end (prefetch beyond T) reads the zero page in every lane
        const unsigned flags = live ? (16u | (ho == 0 ? 1u : 0u) | (ho == p.Ho - 1 ? 2u : 0u) | (wo0 == 0 ? 4u : 0u) |
                                       (wo0 + 16 == p.Wo ? 8u : 0u))
                                    : 0xffffffffu;
        const unsigned xo = __umul24((unsigned)m0, (unsigned)cs);
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const float* g = (x_cls[i] & flags) ? g_wg_zero16 : x_lane[i] + xo;
            rx[i] = *reinterpret_cast<const f32x4*>(g);
        }
        const float* gp = live ? p_lane + __umul24((unsigned)m0, (unsigned)p.N) : g_wg_zero16;
        rp = *reinterpret_cast<const f32x4*>(gp);
    };
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    const bool bias_blk = p.bias_mode == 1 && tx == 0;
    // plane writes: halo rows hp_i = hp_0 + RS i keep the swizzle of hp_0 (RS i = 0 mod 4), so
    // every write of a thread is one base address plus an immediate
    const int w_base = hx_off(tid >> 4, cq * 4);
    const int wp_base = hx_off(HX_ROWS + 16 * (pq >> 4) + prow, (pq & 15) * 4);
    auto split_store = [&](int buf) {         // registers -> bf16 planes of buffer buf
        char* pb = lds + buf * 3 * IMG;
        auto put = [&](char* dst, const f32x4 v) {
            unsigned h[2], m[2], l[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) split3_pair(f32x2{v[2 * q], v[2 * q + 1]}, h[q], m[q], l[q]);
            *reinterpret_cast<u32x2_t*>(dst) = u32x2_t{h[0], h[1]};
            *reinterpret_cast<u32x2_t*>(dst + IMG) = u32x2_t{m[0], m[1]};
            *reinterpret_cast<u32x2_t*>(dst + 2 * IMG) = u32x2_t{l[0], l[1]};
        };
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const int hp = (tid >> 4) + RS * i;
            if (i < XG - 1 || hp < HX_ROWS) put(pb + w_base + i * RS * 128, rx[i]);
        }
        put(pb + wp_base, rp);
        if (bias_blk) bsum += rp;
    };

    f32x16 acc[9];
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t9][r] = 0.f;

    // transposed reads: group grp = lane>>4 covers columns 16 (grp&1) + 0..15, rows 8 (grp>>1) +
    // gq (+4); lane 4 gq + gp addresses row gq, columns 4 gp .. 4 gp + 3
    const int grp = lane >> 4, gq = (lane >> 2) & 3, gp = lane & 3;
    const int rsub = 8 * (grp >> 1) + gq;
    const int ccol = 16 * (grp & 1) + 4 * gp;
    // tap (r, s) reads halo rows 18 r + s + rsub (+4): rows congruent mod 4 share the swizzle, so
    // the 9 taps need 3 base addresses (18 r + s mod 4 in {0, 1, 2, 3}) plus immediates
    int xb[4];
#pragma unroll
    for (int res = 0; res < 4; ++res) xb[res] = hx_off(res + rsub, ci * 32 + ccol);
    const int pbase = hx_off(HX_ROWS + 16 * nt + rsub, nj * 32 + ccol);
    auto mfma_stage = [&](auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        const char* pb = lds + buf * 3 * IMG;
        const bf16x8_t ph = tr_frag(pb + pbase, 0, 4 * 128), pm = tr_frag(pb + IMG + pbase, 0, 4 * 128),
                       pl = tr_frag(pb + 2 * IMG + pbase, 0, 4 * 128);
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) {
            const int row0 = (t9 / 3) * 18 + (t9 % 3);
            const char* xa = pb + xb[row0 & 3] + (row0 & ~3) * 128;
            const bf16x8_t qh = tr_frag(xa, 0, 4 * 128), qm = tr_frag(xa + IMG, 0, 4 * 128),
                           ql = tr_frag(xa + 2 * IMG, 0, 4 * 128);
            acc[t9] = mma6(qh, qm, ql, ph, pm, pl, acc[t9]);
        }
    };
    auto step = [&](int t, auto bufc) {       // MFMAs of stage t (buffer t & 1), split stage t+1
        constexpr int buf = decltype(bufc)::value;
        mfma_stage(bufc);
        if (t + 1 < T) {
            split_store(buf ^ 1);             // raw(t+1) has been in flight for a whole stage
            load(t + 2);
        }
        lds_barrier();
    };

    if (T > 0) {
        load(0);
        split_store(0);
        load(1);
        lds_barrier();
    }
    int t = 0;
    for (; t + 1 < T; t += 2) {
        step(t, std::integral_constant<int, 0>{});
        step(t + 1, std::integral_constant<int, 1>{});
    }
    if (t < T) step(t, std::integral_constant<int, 0>{});

    float* slab = p.slab + (long long)tz * p.Nr * p.Kcp;
    if (bias_blk) {                           // column sums of dZ: 16 rows of partials per column
        f32x4* red = reinterpret_cast<f32x4*>(lds);
        red[tid] = bsum;
        __syncthreads();
        if (tid < 16 * NT) {
            f32x4 v = red[tid];
            for (int r = 1; r < 16; ++r) v += red[r * 16 * NT + tid];
#pragma unroll
            for (int e = 0; e < 4; ++e) slab[(long long)(ty * 64 * NT + tid * 4 + e) * p.Kcp + p.K] = v[e];
        }
    }
    const int lr = lane & 31, lh = lane >> 5;
    const int n = ty * 64 * NT + nt * 64 + nj * 32 + lr;
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
        store_frag<false>(slab + (long long)n * p.Kcp, acc[t9], t9 * p.C + c_lo + ci * 32 + 4 * lh, 0);
}

// ------------------------------------------ bf16 weight gradient with halo reuse (3x3/s1, C3)
// The bf16 form of wgrad_halo_x6_kernel: the operands already are bf16, so a stage's 3 x 18 halo
// (54 pixel rows x 64 channels = 128 B per row) and its 16 dZ rows go to ONE LDS plane as they
// arrive, and each tap is one v_mfma_f32_32x32x16_bf16 per wave instead of an im2col image per
// tap (wgrad_bf16_kernel stages 9 shifted copies of every pixel).  Same swizzle (hx_off), same
// transposed reads, same 4-wave (channel half, output half) x 9-tap accumulator layout, same
// slab partials.  Two stages (32 output pixels) per barrier: the bf16 MFMA work of one stage
// (9 x 32 cycles per wave) is too short to hide a barrier.  Requirements as the x6 kernel.

template <int NT>                             // 64-channel output tiles per block (as the x6 kernel)
__global__ __launch_bounds__(256 * NT) void wgrad_halo_bf16_kernel(const WgradBf16Params p) {
    constexpr int RS = 16 * NT;               // halo rows per row group
    constexpr int XG = (HX_ROWS + RS - 1) / RS;   // halo row groups per thread (54 = 3 x 16 + 6 | 32 + 22)
    constexpr int SPB = 2;                    // stages per barrier
    constexpr int IMG = (HX_ROWS + 16 * NT) * 128;  // one stage's plane: 54 X rows, then NT x 16 dZ rows
    __shared__ __attribute__((aligned(16))) char lds[2 * SPB * IMG];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ci = wave & 1, nj = (wave >> 1) & 1, nt = wave >> 2;
    const WgradBlock blk = wgrad_block(p);   // tx: 64-channel input tile, ty: 64-channel output tile
    const int tx = blk.tx, ty = blk.ty, tz = blk.tz, m_begin = blk.m_begin, m_end = blk.m_end;
    const int T = m_end > m_begin ? (m_end - m_begin) / 16 : 0;

    const int cq = tid & 15;                  // 4-channel quad of the row this thread loads
    const int c_lo = tx * 64;
    const bool first = c_lo < p.c0;
    const __bf16* xsrc = first ? p.src0 + c_lo : p.src1 + (c_lo - p.c0);
    const int cs = first ? p.c0 : p.c1;
    const __bf16* zero = reinterpret_cast<const __bf16*>(g_wg_zero16);
    const __bf16* x_lane[XG];
    unsigned x_cls[XG];                       // edge classes: 1 top, 2 bottom, 4 left, 8 right, 16 past the halo, 32 all
#pragma unroll
    for (int i = 0; i < XG; ++i) {
        const int hp = (tid >> 4) + RS * i;
        const int rr = hp / 18, cc = hp - rr * 18;
        x_lane[i] = xsrc + (long long)((rr - 1) * p.Wi + (cc - 1)) * cs + cq * 4;
        if (hp >= HX_ROWS) x_lane[i] = zero;
        x_cls[i] = 32u | (hp >= HX_ROWS ? 16u
                                        : ((rr == 0 ? 1u : 0u) | (rr == 2 ? 2u : 0u) | (cc == 0 ? 4u : 0u) | (cc == 17 ? 8u : 0u)));
    }
    const int pq = tid % (16 * NT), prow = tid / (16 * NT);   // dZ row and channel quad
    const __bf16* p_lane = p.P + (long long)prow * p.N + ty * 64 * NT + pq * 4;

    u32x2_t rx[SPB][XG], rp[SPB];
    auto load = [&](int t, int j) {           // raw bf16 rows of stage t into register set j
        const int m0 = m_begin + 16 * t;
        const int tu = fdiv(m0, p.dWo);
        const int wo0 = m0 - tu * p.Wo;
        const int bu = fdiv(tu, p.dHo);
        const int ho = tu - bu * p.Ho;
        const bool live = t < T;
        const unsigned flags = live ? (16u | (ho == 0 ? 1u : 0u) | (ho == p.Ho - 1 ? 2u : 0u) | (wo0 == 0 ? 4u : 0u) |
                                       (wo0 + 16 == p.Wo ? 8u : 0u))
                                    : 0xffffffffu;
        const unsigned xo = __umul24((unsigned)m0, (unsigned)cs);
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const __bf16* g = (x_cls[i] & flags) ? zero : x_lane[i] + xo;
            rx[j][i] = *reinterpret_cast<const u32x2_t*>(g);
        }
        const __bf16* gp = live ? p_lane + __umul24((unsigned)m0, (unsigned)p.N) : zero;
        rp[j] = *reinterpret_cast<const u32x2_t*>(gp);
    };
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    const bool bias_blk = p.bias_mode == 1 && tx == 0;
    const int w_base = hx_off(tid >> 4, cq * 4);
    const int wp_base = hx_off(HX_ROWS + 16 * (pq >> 4) + prow, (pq & 15) * 4);
    auto store = [&](int buf, int j, bool live) {   // register set j -> plane j of buffer buf
        char* pb = lds + (buf * SPB + j) * IMG;
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const int hp = (tid >> 4) + RS * i;
            if (i < XG - 1 || hp < HX_ROWS) *reinterpret_cast<u32x2_t*>(pb + w_base + i * RS * 128) = rx[j][i];
        }
        *reinterpret_cast<u32x2_t*>(pb + wp_base) = rp[j];
        if (bias_blk && live) {
            bsum[0] += __builtin_bit_cast(float, rp[j][0] << 16);
            bsum[1] += __builtin_bit_cast(float, rp[j][0] & 0xffff0000u);
            bsum[2] += __builtin_bit_cast(float, rp[j][1] << 16);
            bsum[3] += __builtin_bit_cast(float, rp[j][1] & 0xffff0000u);
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t9][r] = 0.f;

    const int grp = lane >> 4, gq = (lane >> 2) & 3, gp = lane & 3;
    const int rsub = 8 * (grp >> 1) + gq;
    const int ccol = 16 * (grp & 1) + 4 * gp;
    int xb[4];
#pragma unroll
    for (int res = 0; res < 4; ++res) xb[res] = hx_off(res + rsub, ci * 32 + ccol);
    const int pbase = hx_off(HX_ROWS + 16 * nt + rsub, nj * 32 + ccol);
    auto mfma_plane = [&](const char* pb) {
        const bf16x8_t ph = tr_frag(pb + pbase, 0, 4 * 128);
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) {
            const int row0 = (t9 / 3) * 18 + (t9 % 3);
            const bf16x8_t qh = tr_frag(pb + xb[row0 & 3] + (row0 & ~3) * 128, 0, 4 * 128);
            acc[t9] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qh, ph, acc[t9], 0, 0, 0);
        }
    };
    // group g = stages SPB g .. SPB g + SPB - 1 in buffer g & 1; the loads of group g + 1 are in
    // flight while group g's MFMAs run
    const int NG = (T + SPB - 1) / SPB;
    auto group = [&](int g, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
#pragma unroll
        for (int j = 0; j < SPB; ++j) mfma_plane(lds + (buf * SPB + j) * IMG);
        if (g + 1 < NG) {
#pragma unroll
            for (int j = 0; j < SPB; ++j) store(buf ^ 1, j, SPB * (g + 1) + j < T);
#pragma unroll
            for (int j = 0; j < SPB; ++j) load(SPB * (g + 2) + j, j);
        }
        lds_barrier();
    };

    if (NG > 0) {
#pragma unroll
        for (int j = 0; j < SPB; ++j) load(j, j);
#pragma unroll
        for (int j = 0; j < SPB; ++j) store(0, j, j < T);
#pragma unroll
        for (int j = 0; j < SPB; ++j) load(SPB + j, j);
        lds_barrier();
    }
    int g = 0;
    for (; g + 1 < NG; g += 2) {
        group(g, std::integral_constant<int, 0>{});
        group(g + 1, std::integral_constant<int, 1>{});
    }
    if (g < NG) group(g, std::integral_constant<int, 0>{});

    float* slab = p.slab + (long long)tz * p.Nr * p.Kcp;
    if (bias_blk) {
        f32x4* red = reinterpret_cast<f32x4*>(lds);
        red[tid] = bsum;
        __syncthreads();
        if (tid < 16 * NT) {
            f32x4 v = red[tid];
            for (int r = 1; r < 16; ++r) v += red[r * 16 * NT + tid];
#pragma unroll
            for (int e = 0; e < 4; ++e) slab[(long long)(ty * 64 * NT + tid * 4 + e) * p.Kcp + p.K] = v[e];
        }
    }
    const int lr = lane & 31, lh = lane >> 5;
    const int n = ty * 64 * NT + nt * 64 + nj * 32 + lr;
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
        store_frag<false>(slab + (long long)n * p.Kcp, acc[t9], t9 * p.C + c_lo + ci * 32 + 4 * lh, 0);
}

}  // namespace pu
