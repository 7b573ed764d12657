// Winograd-domain 3x3 weight gradients: 64 x 64 channel blocks, and 128 x 128 blocks of one position column.
// After wgrad_halo.h (hx_off, the 128-byte plane swizzle) and wgrad_gemm.h (wb_sw, the 256-byte one).
// Part of wgrad.hip, which includes it once, after its parameter block and shared helpers.
#pragma once

namespace pu {

// ------------------------------------------ Winograd-domain 3x3 weight gradient (F(2x2, 3x3))
// The forward of F(2x2,3x3) is y = A^T [ (G g G^T) (.) (B^T d B) ] A (winograd.hip); its
// derivative w.r.t. the kernel g, summed over the 2x2 output tiles (d = the tile's 4x4 input
// window, e = its 2x2 output gradient), is
//     dW = G^T M G,   M_xi[n][c] = sum_tiles Ehat_xi[tile][n] Dhat_xi[tile][c]  (xi = 16 positions)
// with Ehat = A e A^T and Dhat = B^T d B - both formed with +-1 adds only, so every operand is an
// fp32 value that splits exactly into hi/mid/lo bf16 and the products are the same 6-term fp32
// arithmetic as every other weight gradient here, accumulated in fp32.  16 products per tile and
// (n, c) instead of the direct 36 (9 taps x 4 pixels): 2.25x fewer MFMAs.  G^T M G (factors 1/2,
// exact scalings) runs once per block on its fp32 partial M, so the slab keeps the direct
// kernels' [split][n][tap * C + c] layout (+ the bias column) and the same fixed-order fp64
// reduction finishes it - deterministic.
//
// Block: 64 output x 64 input channels x all 16 positions over a contiguous range of tiles (one
// split), 8 waves; wave (wc, wn, wj) accumulates 32 input x 32 output channels for the 8 positions
// (i, 2 wj + jj): 128 accumulators.  A stage is 16 tiles = one k-step of v_mfma_f32_32x32x16_bf16,
// split into 4 sub-stages, one per row i of the positions (as winograd.hip).  Thread (tile pt,
// channel pair cp) keeps its tile's 4x4 window (2 input channels) and 2x2 gradient tile (2 output
// channels) in registers and forms row i of Dhat and Ehat for the next sub-stage while the MFMAs
// of the current one run; the planes go to LDS as [tile row][64 channels] bf16 images (128-byte
// rows, the halo kernel's swizzle) read back with ds_read_b64_tr_b16 (k = tile).  Each window row
// is reloaded for the next stage as soon as its last transform is formed (>= 2 sub-stages of
// cover).  Ehat is formed with the sign-normalised A' = [1 0; 1 1; 1 -1; 0 1] (A's row 3 is
// [0 -1]): M_xi = s_i s_j M'_xi, s = (1, 1, 1, -1), applied in the output transform.
constexpr int WW_IMG = 16 * 128;           // one (position, plane) image: 16 tile rows x 64 channels
constexpr int WW_SLOT = 4 * 3 * WW_IMG;    // one operand, one sub-stage: 4 positions x 3 planes

struct WinoWgradParams {
    WgradParams p;
    int tiles, tps;            // tiles (batch x Ho/2 x Wo/2); tiles per split (multiple of 16)
    FastDiv dTw, dTh;          // tile index -> (image, tile row, tile column)
    unsigned x0_bytes, x1_bytes, p_bytes;   // buffer ranges (sources shifted back by Wi + 1 pixels)
};

// tile m of the grid of 2 x 2 output tiles -> image b, tile row ty, tile column tx
struct WinoTile {
    int b, ty, tx;
};
__device__ __forceinline__ WinoTile wino_tile(const WinoWgradParams& w, int m) {
    WinoTile t;
    const int t2 = fdiv(m, w.dTw);
    t.tx = m - t2 * (w.p.Wo >> 1);
    t.b = fdiv(t2, w.dTh);
    t.ty = t2 - t.b * (w.p.Ho >> 1);
    return t;
}

__global__ __launch_bounds__(512) void wgrad_wino_x6_kernel(const WinoWgradParams w) {
#pragma clang fp contract(off)
    const WgradParams& p = w.p;
    // two sub-stage slots per operand, as separate arrays: the compiler then knows that the
    // plane stores of the next sub-stage (other slot) do not alias this sub-stage's operand reads
    // and can interleave them; after the loop lx0 / lx1 carry the output-transform exchange
    __shared__ __attribute__((aligned(16))) char lx0[WW_SLOT];
    __shared__ __attribute__((aligned(16))) char lx1[WW_SLOT];
    __shared__ __attribute__((aligned(16))) char lg0[WW_SLOT];
    __shared__ __attribute__((aligned(16))) char lg1[WW_SLOT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave & 1, wn = (wave >> 1) & 1, wj = wave >> 2;
    // logical block (split z, output block ny, input block cx), cx fastest: the blocks an XCD runs
    // together read the same tiles
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int cx = blk % p.gx;
    const int rest = blk / p.gx;
    const int ny = rest % p.gy;
    const int z = rest / p.gy;
    const int t_begin = z * w.tps;
    const int t_end = min(w.tiles, t_begin + w.tps);
    const int S = (t_end - t_begin + 15) >> 4;

    // ---- producer role: tile pt of a stage, channel pair cp of the 64 input / 64 output channels
    const int pt = tid >> 5, cp = tid & 31;
    const int c_lo = cx * 64;
    const bool first = c_lo < p.c0;
    const int cs = first ? p.c0 : p.c1;       // pixel stride of the input block's source
    const int shift = p.Wi + 1;               // window corner (2ty-1, 2tx-1) >= (-1, -1)
    const __amdgpu_buffer_rsrc_t xr = uniform_rsrc((first ? p.src0 : p.src1) - (long long)shift * cs,
                                              first ? w.x0_bytes : w.x1_bytes);
    const __amdgpu_buffer_rsrc_t gr = uniform_rsrc(p.P, w.p_bytes);
    const unsigned pixb = (unsigned)cs * 4u;
    const unsigned xco = (unsigned)((first ? c_lo : c_lo - p.c0) + 2 * cp) * 4u;
    const unsigned gco = (unsigned)(ny * 64 + 2 * cp) * 4u;
    const unsigned gpix = (unsigned)p.N * 4u;
    const int st_off = hx_off(pt, 2 * cp);    // the thread's 4-byte slot in every image

    // window rows of a stage as the loader sees them (byte offsets; LEAN_OOB: zeros)
    unsigned xv[4];
    bool xc0 = false, xc3 = false;
    auto decode_x = [&](int k) {
        const int m = t_begin + 16 * k + pt;
        const bool mv = m < t_end;
        WinoTile t = {0, 0, 0};
        if (mv) t = wino_tile(w, m);
        const int ty = t.ty, tx = t.tx, b = t.b;
        const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
        const unsigned base = (unsigned)(((b * p.Hi + y0) * p.Wi + x0 + shift) * cs) * 4u + xco;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            xv[r] = mv && (unsigned)(y0 + r) < (unsigned)p.Hi ? base + (unsigned)(r * p.Wi) * pixb : LEAN_OOB;
        xc0 = x0 >= 0;
        xc3 = x0 + 3 < p.Wi;
    };
    unsigned gv[2];
    auto decode_g = [&](int k) {
        const int m = t_begin + 16 * k + pt;
        if (m < t_end) {
            const WinoTile t = wino_tile(w, m);
            const int ty = t.ty, tx = t.tx, b = t.b;
            const unsigned base = (unsigned)((b * p.Ho + 2 * ty) * p.Wo + 2 * tx) * gpix + gco;
            gv[0] = base;
            gv[1] = base + (unsigned)p.Wo * gpix;
        } else {
            gv[0] = gv[1] = LEAN_OOB;
        }
    };
    f32x2 d[4][4], e[2][2];
    auto load_x = [&](int r) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            unsigned vo = xv[r];
            if (s == 0) vo = xc0 ? vo : LEAN_OOB;
            if (s == 3) vo = xc3 ? vo : LEAN_OOB;
            d[r][s] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(
                                                       xr, vo, __builtin_amdgcn_readfirstlane(s * pixb), 0));
        }
    };
    auto load_g = [&](int a) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
            e[a][s] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(
                                                       gr, gv[a], __builtin_amdgcn_readfirstlane(s * gpix), 0));
    };
    // row i of Dhat (B^T d B) and Ehat (A' e A'^T) for this thread's pairs -> bf16 planes in the
    // sub-stage slots sx / sg: image (j, plane) at (3 j + plane) * WW_IMG
    auto form = [&](auto i_c, char* sx, char* sg) {
        constexpr int i = decltype(i_c)::value;
        f32x2 t[4], u[2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (i == 0) t[s] = d[0][s] - d[2][s];
            else if constexpr (i == 1) t[s] = d[1][s] + d[2][s];
            else if constexpr (i == 2) t[s] = d[2][s] - d[1][s];
            else t[s] = d[1][s] - d[3][s];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (i == 0) u[s] = e[0][s];
            else if constexpr (i == 1) u[s] = e[0][s] + e[1][s];
            else if constexpr (i == 2) u[s] = e[0][s] - e[1][s];
            else u[s] = e[1][s];
        }
        const f32x2 dv[4] = {t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]};
        const f32x2 ev[4] = {u[0], u[0] + u[1], u[0] - u[1], u[1]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned h, m, l;
            split3_pair(dv[j], h, m, l);
            char* b = sx + 3 * j * WW_IMG + st_off;
            *reinterpret_cast<unsigned*>(b) = h;
            *reinterpret_cast<unsigned*>(b + WW_IMG) = m;
            *reinterpret_cast<unsigned*>(b + 2 * WW_IMG) = l;
            split3_pair(ev[j], h, m, l);
            b = sg + 3 * j * WW_IMG + st_off;
            *reinterpret_cast<unsigned*>(b) = h;
            *reinterpret_cast<unsigned*>(b + WW_IMG) = m;
            *reinterpret_cast<unsigned*>(b + 2 * WW_IMG) = l;
        }
    };

    // ---- MFMA role: transposed fragment reads as in wgrad_halo_x6_kernel (k = tile row)
    const int grp = lane >> 4, gq = (lane >> 2) & 3, gp = lane & 3;
    const int rsub = 8 * (grp >> 1) + gq;
    const int ccol = 16 * (grp & 1) + 4 * gp;
    const int xa = hx_off(rsub, wc * 32 + ccol) + 2 * wj * 3 * WW_IMG;
    const int ga = hx_off(rsub, wn * 32 + ccol) + 2 * wj * 3 * WW_IMG;
    f32x16 acc[8];                            // [i][jj]: position (i, 2 wj + jj)
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
    auto mma = [&](auto x_c, const char* sx, const char* sg, int jj) {
        constexpr int x = decltype(x_c)::value;
        const char* xb = sx + xa + jj * 3 * WW_IMG;
        const char* gb = sg + ga + jj * 3 * WW_IMG;
        const bf16x8_t qh = tr_frag(xb, 0, 4 * 128), qm = tr_frag(xb + WW_IMG, 0, 4 * 128),
                       ql = tr_frag(xb + 2 * WW_IMG, 0, 4 * 128);
        const bf16x8_t ph = tr_frag(gb, 0, 4 * 128), pm = tr_frag(gb + WW_IMG, 0, 4 * 128),
                       pl = tr_frag(gb + 2 * WW_IMG, 0, 4 * 128);
        acc[x] = mma6(qh, qm, ql, ph, pm, pl, acc[x]);
    };
    f32x2 bsum = {0.f, 0.f};               // dbias partial of the thread's output pair

    // sub-stage (k, i): MFMAs of row i from slot i & 1, row i + 1 (or the next stage's row 0)
    // formed into the other slot, then the window / gradient rows whose last use that was are
    // reloaded for the next stage (x row 0 two stages ahead: its stage-k + 1 copy was formed in
    // the sub-stage before)
    auto sub = [&](int k, auto i_c) {
        constexpr int i = decltype(i_c)::value;
        char* sx = (i & 1) ? lx1 : lx0;
        char* sg = (i & 1) ? lg1 : lg0;
        char* nx = (i & 1) ? lx0 : lx1;
        char* ng = (i & 1) ? lg0 : lg1;
        mma(std::integral_constant<int, 2 * i>{}, sx, sg, 0);
        // (past the last stage this forms zeros into a slot no MFMA reads: the sub-stage stays
        // one basic block for the interleave below)
        form(std::integral_constant<int, (i + 1) & 3>{}, nx, ng);
        if constexpr (i == 1) {               // d row 2 and e row 0 are dead: next stage's
            load_x(2);
            bsum += e[0][0] + e[0][1];
            decode_g(k + 1);
            load_g(0);
        } else if constexpr (i == 2) {        // d rows 1, 3 and e row 1 are dead
            load_x(1);
            load_x(3);
            bsum += e[1][0] + e[1][1];
            load_g(1);
        } else if constexpr (i == 3) {        // d row 0 of stage k + 1 was used: stage k + 2's
            decode_x(k + 2);
            load_x(0);
        }
        mma(std::integral_constant<int, 2 * i + 1>{}, sx, sg, 1);
        // Interleave: the wave's 12 MFMAs spread over the forming work (~110 VALU + 24 LDS
        // stores) instead of 6 before and 6 after it - the two waves of a SIMD run the same phase
        // between barriers, so MFMAs bunched at the ends leave the matrix pipe idle during the VALU
#if !PU_NO_ILV
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);       // position 0 operands
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 9, 0);     // ~1/12 of the VALU
            __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);     // ~1/12 of the plane stores
            if (q == 2) __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);   // position 1 operands
        }
#endif
        lds_barrier();
    };

    // prologue: stage 0 whole, sub-stage (0, 0) formed, stage 1's row 0 in flight
    decode_x(0);
    load_x(0);
    load_x(1);
    load_x(2);
    load_x(3);
    decode_g(0);
    load_g(0);
    load_g(1);
    form(std::integral_constant<int, 0>{}, lx0, lg0);
    decode_x(1);
    load_x(0);
    lds_barrier();
    for (int k = 0; k < S; ++k) {
        sub(k, std::integral_constant<int, 0>{});
        sub(k, std::integral_constant<int, 1>{});
        sub(k, std::integral_constant<int, 2>{});
        sub(k, std::integral_constant<int, 3>{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // trailing (empty-range) loads

    float* slab = p.slab + (long long)z * p.Nr * p.Kcp;
    // ---- bias: column sums of dZ over the split, fixed order (thread stages, then the 16 tiles)
    if (p.bias_mode == 1 && cx == 0) {
        f32x2* red = reinterpret_cast<f32x2*>(lg0);
        red[tid] = bsum;
        __syncthreads();
        if (tid < 32) {
            f32x2 v = red[tid];
            for (int r = 1; r < 16; ++r) v += red[r * 32 + tid];
            slab[(long long)(ny * 64 + 2 * tid) * p.Kcp + p.K] = v[0];
            slab[(long long)(ny * 64 + 2 * tid + 1) * p.Kcp + p.K] = v[1];
        }
        __syncthreads();
    }

    // ---- output transform dW = G^T M G (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]).  Over the rows
    // first (the wave holds all 4 rows of its 2 columns j): R[r][j] = sum_a G[a][r] M[a][j]; then
    // dW[r][s] = sum_j R[r][j] G[j][s] = P0[r][s] + P1[r][s], P0 from j = 0, 1 (wj = 0), P1 from
    // j = 2, 3 (wj = 1).  The two waves of a (wc, wn) pair swap halves through LDS: wave wj
    // finishes the channel groups q = 2 wj, 2 wj + 1 of its accumulators.  Signs: M = s_i s_j M'.
    const float sj1 = wj ? -1.f : 1.f;        // s_j of column jj = 1 (j = 3 for wj = 1)
    // 6 KB per wave: the wc = 0 pairs in lx0, the wc = 1 pairs in lx1
    float* xs = reinterpret_cast<float*>(wc ? lx1 : lx0) + (wn * 2 + wj) * 24 * 64;
    const float* xrd = reinterpret_cast<const float*>(wc ? lx1 : lx0) + (wn * 2 + (1 - wj)) * 24 * 64;
    const int lr = lane & 31, lh = lane >> 5;
    const int n = ny * 64 + wn * 32 + lr;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float mine[2][3][4], other[2][3][4];  // [q half][s][e]
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ee = 0; ee < 4; ++ee) {
                const int idx = 4 * q + ee;
                float R[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    // M[a][j] = s_a s_j M'[a][j]: s_3 = -1 on row a = 3 and on column j = 3
                    const float m0 = acc[0 * 2 + jj][idx], m1 = acc[1 * 2 + jj][idx];
                    const float m2 = acc[2 * 2 + jj][idx], m3 = -acc[3 * 2 + jj][idx];
                    float v = r == 0 ? m0 + 0.5f * (m1 + m2) : r == 1 ? 0.5f * (m1 - m2) : 0.5f * (m1 + m2) + m3;
                    R[jj] = jj == 1 ? sj1 * v : v;
                }
                // this wave's share of dW[r][s] for s = 0..2
                float P[3];
                if (wj == 0) {            // j = 0, 1: R0 G[0] + R1 G[1]
                    P[0] = R[0] + 0.5f * R[1];
                    P[1] = 0.5f * R[1];
                    P[2] = 0.5f * R[1];
                } else {                  // j = 2, 3: R2 G[2] + R3 G[3]
                    P[0] = 0.5f * R[0];
                    P[1] = -0.5f * R[0];
                    P[2] = 0.5f * R[0] + R[1];
                }
                const bool keep = (q >> 1) == wj;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (keep) mine[q & 1][s][ee] = P[s];
                    else other[q & 1][s][ee] = P[s];
                }
            }
        // send the partner's half: [qh][s][e] -> 24 floats per lane
#pragma unroll
        for (int qh = 0; qh < 2; ++qh)
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) xs[((qh * 3 + s) * 4 + ee) * 64 + lane] = other[qh][s][ee];
        __syncthreads();
#pragma unroll
        for (int qh = 0; qh < 2; ++qh)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                f32x4 v;
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) {
                    const float o = xrd[((qh * 3 + s) * 4 + ee) * 64 + lane];
                    // P0 + P1 in that order on both waves of the pair
                    v[ee] = wj == 0 ? mine[qh][s][ee] + o : o + mine[qh][s][ee];
                }
                const int q = 2 * wj + qh;
                const int k = (3 * r + s) * p.C + c_lo + wc * 32 + 8 * q + 4 * lh;
                *reinterpret_cast<f32x4*>(slab + (long long)n * p.Kcp + k) = v;
            }
        __syncthreads();
    }
}

// ---------------------------------- Winograd-domain weight gradient, one position column per block
// wgrad_wino_x6_kernel forms dW = G^T M G rows first: R[r][j] = sum_a G[a][r] M[a][j] is local to
// the wave that holds column j's four positions, and only the second half, dW[r][s] = sum_j R[r][j]
// G[j][s], crosses waves.  So a block may own ONE column j of the 4 x 4 positions and hand phase 2
// the three numbers R[0..2][j] per (n, c): with the same 65 536 accumulators it then covers 128 input
// x 128 output channels and forms 4 x (128 + 128) values per tile for 4 x 128 x 128 products - 64
// products per formed value against 32.  The slab page of (split z, column j) is virtual split
// 4 z + j: [Nr][Kcp] with Kc = 3 C (+ 1 bias column) and column r C + c; wgrad_finish_cols_kernel
// finishes the transform per split in fp32 and sums the splits.  Every value is formed by the
// operations of wgrad_wino_x6_kernel in its order (transforms, split, products, accumulation per
// split over the same tile ranges, R, then P0 + P1, then the fp64 sums), so dweight and dbias are
// bit-identical to that kernel's.
//
// 512 threads, 8 waves (wc of 2, wn of 4): a wave accumulates 64 input x 32 output channels for
// the column's 4 positions (8 accumulator blocks).  A stage is 16 tiles = one k-step, in two
// sub-stages of two positions (i = 2 h, 2 h + 1), so the LDS footprint is that of the 64 x 64
// kernel: per operand and slot 2 positions x 3 planes x [16 tile rows][128 channels] bf16 (256-byte
// rows, wgrad_bf16_kernel's swizzle).  Thread (tile pt, channel quad cq) holds the two window
// columns (4 rows each) that column j of B^T d B reads and the one or two dZ columns that column j
// of A' e A'^T reads.  The column is a block-uniform run-time value (all four columns of a
// (cx, ny, z) sit next to each other in ONE grid and share their windows in L2); each window
// column gets the row transform t_i first, as in the 64 x 64 kernel, then the two columns combine
// in a packed fma with a +-1 operand - exactly the rounded sum or difference:
//     j = 0: t[0] - t[2]   j = 1: t[1] + t[2]   j = 2: t[2] - t[1]   j = 3: t[1] - t[3]
//     j = 0: u[0]          j = 1: u[0] + u[1]   j = 2: u[0] - u[1]   j = 3: u[1] (= -A row 3)
// (j = 2 loads its columns as (2, 1): forming t[1] - t[2] and negating M afterwards is NOT
// bit-identical - the MFMA accumulation is not symmetric under a sign flip of an operand.)
// Sub-stage (k, 1) forms all four positions' values of stage k + 1 (positions 2, 3 are held in
// registers for sub-stage (k + 1, 0)), after which the raw columns are dead and stage k + 2's are
// loaded: two sub-stages of cover, as in the 64 x 64 kernel.
// Requires wino_wgrad_ok and c0 % 128 == c1 % 128 == N % 128 == 0.
constexpr int WWR_IMG = 16 * 256;            // one (position, plane) image: 16 tile rows x 128 channels
constexpr int WWR_SLOT = 2 * 3 * WWR_IMG;    // one operand, one sub-stage: 2 positions x 3 planes
__device__ __forceinline__ int wwr_off(int row, int col) {   // byte offset in a 128-column plane
    return row * 256 + 16 * ((col >> 3) ^ wb_sw(row)) + 2 * (col & 7);
}

__global__ __launch_bounds__(512) void wgrad_wino_cols_x6_kernel(const WinoWgradParams w) {
#pragma clang fp contract(off)
    const WgradParams& p = w.p;
    // two sub-stage slots per operand as separate arrays (see wgrad_wino_x6_kernel)
    __shared__ __attribute__((aligned(16))) char lx0[WWR_SLOT];
    __shared__ __attribute__((aligned(16))) char lx1[WWR_SLOT];
    __shared__ __attribute__((aligned(16))) char lg0[WWR_SLOT];
    __shared__ __attribute__((aligned(16))) char lg1[WWR_SLOT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave & 1, wn = wave >> 1;
    // logical block (split z, output block ny, input block cx, column J), J fastest: the four columns
    // of a channel block and tile range run on one XCD and read the same windows and dZ tiles
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int J = blk & 3;
    const int cx = (blk >> 2) % p.gx;
    const int rest = (blk >> 2) / p.gx;
    const int ny = rest % p.gy;
    const int z = rest / p.gy;
    const int t_begin = z * w.tps;
    const int t_end = min(w.tiles, t_begin + w.tps);
    const int S = (t_end - t_begin + 15) >> 4;
    const int xca = J == 0 ? 0 : J == 2 ? 2 : 1, xcb = J == 3 ? 3 : J == 2 ? 1 : 2;   // window columns a, b: dv = t_a + sx t_b
    const float sxf = J == 1 ? 1.f : -1.f;
    const int gca = J == 3 ? 1 : 0;                           // dZ columns: ev = u_a + sg u_b, b = column 1
    const bool gtwo = J == 1 || J == 2;                       // (columns 0 and 3 read one dZ column)
    const float sgf = J == 2 ? -1.f : 1.f;
    const f32x2 sx2 = {sxf, sxf}, sg2 = {sgf, sgf};

    // ---- producer role: tile pt of a stage, channel quad cq of the 128 input / output channels
    const int pt = tid >> 5, cq = tid & 31;
    const int c_lo = cx * 128;
    const bool first = c_lo < p.c0;
    const int cs = first ? p.c0 : p.c1;       // pixel stride of the input block's source
    const int shift = p.Wi + 1;               // window corner (2ty-1, 2tx-1) >= (-1, -1)
    const __amdgpu_buffer_rsrc_t xr = uniform_rsrc((first ? p.src0 : p.src1) - (long long)shift * cs,
                                              first ? w.x0_bytes : w.x1_bytes);
    const __amdgpu_buffer_rsrc_t gr = uniform_rsrc(p.P, w.p_bytes);
    const unsigned pixb = (unsigned)cs * 4u;
    const unsigned xco = (unsigned)((first ? c_lo : c_lo - p.c0) + 4 * cq) * 4u;
    const unsigned gco = (unsigned)(ny * 128 + 4 * cq) * 4u;
    const unsigned gpix = (unsigned)p.N * 4u;
    const int st_off = wwr_off(pt, 4 * cq);   // the thread's 8-byte slot in every image

    f32x2 da[4][2], db[4][2], ea[2][2], eb[2][2];   // raw columns a, b: [window / dZ row][channel pair]
    // decode tile pt of stage k and load its columns (out-of-range tiles, rows and columns: zeros)
    auto load_stage = [&](int k) {
        const int m = t_begin + 16 * k + pt;
        const bool mv = m < t_end;
        WinoTile t = {0, 0, 0};
        if (mv) t = wino_tile(w, m);
        const int ty = t.ty, tx = t.tx, b = t.b;
        const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
        const unsigned base = (unsigned)(((b * p.Hi + y0) * p.Wi + x0 + shift) * cs) * 4u + xco;
        // columns 1 and 2 are always inside the (even-width) image
        const bool cva = mv && (xca != 0 || x0 >= 0), cvb = mv && (xcb != 3 || x0 + 3 < p.Wi);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool rv = (unsigned)(y0 + r) < (unsigned)p.Hi;
            const unsigned oa = cva && rv ? base + (unsigned)xca * pixb : LEAN_OOB;
            const unsigned ob = cvb && rv ? base + (unsigned)xcb * pixb : LEAN_OOB;
            const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)(r * p.Wi) * pixb);
            const f32x4 a4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, oa, so, 0));
            const f32x4 b4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, ob, so, 0));
            da[r][0] = f32x2{a4[0], a4[1]}; da[r][1] = f32x2{a4[2], a4[3]};
            db[r][0] = f32x2{b4[0], b4[1]}; db[r][1] = f32x2{b4[2], b4[3]};
        }
        const unsigned gbase = (unsigned)((b * p.Ho + 2 * ty) * p.Wo + 2 * tx) * gpix + gco;
        const unsigned ga_ = mv ? gbase + (unsigned)gca * gpix : LEAN_OOB;
        const unsigned gb_ = mv && gtwo ? gbase + gpix : LEAN_OOB;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)(a * p.Wo) * gpix);
            const f32x4 a4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(gr, ga_, so, 0));
            const f32x4 b4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(gr, gb_, so, 0));
            ea[a][0] = f32x2{a4[0], a4[1]}; ea[a][1] = f32x2{a4[2], a4[3]};
            eb[a][0] = f32x2{b4[0], b4[1]}; eb[a][1] = f32x2{b4[2], b4[3]};
        }
    };
    // one position's 4 channels of both operands -> hi / mid / lo plane words of slot position jj
    auto put = [&](const f32x2 (&v)[2], char* b) {
        unsigned h0, m0, l0, h1, m1, l1;
        split3_pair(v[0], h0, m0, l0);
        split3_pair(v[1], h1, m1, l1);
        *reinterpret_cast<u32x2_t*>(b) = u32x2_t{h0, h1};
        *reinterpret_cast<u32x2_t*>(b + WWR_IMG) = u32x2_t{m0, m1};
        *reinterpret_cast<u32x2_t*>(b + 2 * WWR_IMG) = u32x2_t{l0, l1};
    };
    f32x2 hd[2][2], he[2][2];              // positions 2, 3 of the stage formed last
    f32x2 bsum[2] = {{0.f, 0.f}, {0.f, 0.f}};   // dbias partial of the thread's output quad
    // column J of Dhat and Ehat from the raw columns, in the 64 x 64 kernel's order (the row
    // transform of each column first, then the two columns combined): positions (0, J), (1, J) to
    // the slot, (2, J), (3, J) held
    auto form_a = [&](char* sx, char* sg) {
        f32x2 dv0[2], dv1[2], ev0[2], ev1[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const f32x2 ta[4] = {da[0][hf] - da[2][hf], da[1][hf] + da[2][hf], da[2][hf] - da[1][hf], da[1][hf] - da[3][hf]};
            const f32x2 tb[4] = {db[0][hf] - db[2][hf], db[1][hf] + db[2][hf], db[2][hf] - db[1][hf], db[1][hf] - db[3][hf]};
            const f32x2 ua[4] = {ea[0][hf], ea[0][hf] + ea[1][hf], ea[0][hf] - ea[1][hf], ea[1][hf]};
            const f32x2 ub[4] = {eb[0][hf], eb[0][hf] + eb[1][hf], eb[0][hf] - eb[1][hf], eb[1][hf]};
            dv0[hf] = __builtin_elementwise_fma(tb[0], sx2, ta[0]);
            dv1[hf] = __builtin_elementwise_fma(tb[1], sx2, ta[1]);
            hd[0][hf] = __builtin_elementwise_fma(tb[2], sx2, ta[2]);
            hd[1][hf] = __builtin_elementwise_fma(tb[3], sx2, ta[3]);
            ev0[hf] = __builtin_elementwise_fma(ub[0], sg2, ua[0]);
            ev1[hf] = __builtin_elementwise_fma(ub[1], sg2, ua[1]);
            he[0][hf] = __builtin_elementwise_fma(ub[2], sg2, ua[2]);
            he[1][hf] = __builtin_elementwise_fma(ub[3], sg2, ua[3]);
            bsum[hf] += ea[0][hf] + eb[0][hf];    // dZ rows 0, 1 in the 64 x 64 kernel's order (J = 1)
            bsum[hf] += ea[1][hf] + eb[1][hf];
        }
        put(dv0, sx + st_off);
        put(ev0, sg + st_off);
        put(dv1, sx + 3 * WWR_IMG + st_off);
        put(ev1, sg + 3 * WWR_IMG + st_off);
    };
    auto form_b = [&](char* sx, char* sg) {
        put(hd[0], sx + st_off);
        put(he[0], sg + st_off);
        put(hd[1], sx + 3 * WWR_IMG + st_off);
        put(he[1], sg + 3 * WWR_IMG + st_off);
    };

    // ---- MFMA role: transposed fragment reads (k = tile row); rows +0 / +4 of a fragment sit in
    // differently swizzled rows, so each has its own offset
    const int grp = lane >> 4, gq = (lane >> 2) & 3, gp = lane & 3;
    const int rsub = 8 * (grp >> 1) + gq;
    const int ccol = 16 * (grp & 1) + 4 * gp;
    int xo[2][2], go[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        xo[0][hh] = wwr_off(rsub + 4 * hh, wc * 64 + ccol);
        xo[1][hh] = wwr_off(rsub + 4 * hh, wc * 64 + 32 + ccol);
        go[hh] = wwr_off(rsub + 4 * hh, wn * 32 + ccol);
    }
    f32x16 acc[8];                            // [f][i]: input channels 32 f .., position (i, J)
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
    // slot position jj = position j of the row: 3 dZ fragments, then 6 products for each channel half
    auto mma = [&](auto j_c, const char* sx, const char* sg, int jj) {
        constexpr int j = decltype(j_c)::value;
        const char* gb = sg + jj * 3 * WWR_IMG;
        const bf16x8_t ph = tr_frag(gb, go[0], go[1]), pm = tr_frag(gb + WWR_IMG, go[0], go[1]),
                        pl = tr_frag(gb + 2 * WWR_IMG, go[0], go[1]);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const char* xb = sx + jj * 3 * WWR_IMG;
            const bf16x8_t qh = tr_frag(xb, xo[f][0], xo[f][1]), qm = tr_frag(xb + WWR_IMG, xo[f][0], xo[f][1]),
                            ql = tr_frag(xb + 2 * WWR_IMG, xo[f][0], xo[f][1]);
            acc[4 * f + j] = mma6(qh, qm, ql, ph, pm, pl, acc[4 * f + j]);
        }
    };

    // sub-stage (k, h): the 24 MFMAs of positions 2 h, 2 h + 1 from slot h while the other slot is
    // formed - h = 0: the held positions 2, 3 of stage k; h = 1: stage k + 1 from the raw rows,
    // then stage k + 2's rows are loaded (past the last stage: zeros into a slot no MFMA reads)
    auto sub = [&](int k, auto h_c) {
        constexpr int h = decltype(h_c)::value;
        char* sx = h ? lx1 : lx0;
        char* sg = h ? lg1 : lg0;
        char* nx = h ? lx0 : lx1;
        char* ng = h ? lg0 : lg1;
        mma(std::integral_constant<int, 2 * h>{}, sx, sg, 0);
        if constexpr (h == 0) {
            form_b(nx, ng);
        } else {
            form_a(nx, ng);
            load_stage(k + 2);
        }
        mma(std::integral_constant<int, 2 * h + 1>{}, sx, sg, 1);
        // the wave's 24 MFMAs spread over the forming work, operands fetched a channel half ahead
#if !PU_NO_ILV
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);       // position 0: dZ and half 0
#pragma unroll
        for (int q = 0; q < 24; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA
            if (q == 0 || q == 12) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);   // half 1
            if (q == 6) __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);             // position 1
            __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);     // ~1/24 of the VALU
            if (q & 1) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // 12 plane stores
        }
#endif
        lds_barrier();
    };

    // prologue: stage 0 formed (positions 0, 1 in slot 0), stage 1's rows in flight
    load_stage(0);
    form_a(lx0, lg0);
    load_stage(1);
    lds_barrier();
    for (int k = 0; k < S; ++k) {
        sub(k, std::integral_constant<int, 0>{});
        sub(k, std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // trailing (empty-range) loads

    float* slab = p.slab + (long long)(4 * z + J) * p.Nr * p.Kcp;
    // ---- bias: column sums of dZ over the split, fixed order (thread stages, then the 16 tiles);
    // column 1's blocks read all four dZ pixels.  p.K is this slab's bias column, 3 C.
    if (p.bias_mode == 1 && cx == 0 && J == 1) {
        f32x2* red = reinterpret_cast<f32x2*>(lg0);
        red[2 * tid] = bsum[0];
        red[2 * tid + 1] = bsum[1];
        __syncthreads();
        if (tid < 64) {                       // channel pair tid of the 128
            f32x2 v = red[tid];
            for (int r = 1; r < 16; ++r) v += red[r * 64 + tid];
            slab[(long long)(ny * 128 + 2 * tid) * p.Kcp + p.K] = v[0];
            slab[(long long)(ny * 128 + 2 * tid + 1) * p.Kcp + p.K] = v[1];
        }
        __syncthreads();                      // lg0 is reused below
    }

    // ---- first half of the output transform, lane local: R[r] = sum_a G[a][r] M[a][J] with
    // M[a][J] = s_a s_J M'[a][J], the 64 x 64 kernel's expression; column r C + c of the page.
    // An accumulator lane holds 4 channels of one output row n, so direct stores would be 32-byte
    // pieces of 32 slab rows; each wave turns its [32 n][64 c] tile of one r through a private LDS
    // tile (rows skewed by 16 B) and stores 4 rows x 256 contiguous bytes per instruction.
    constexpr int TP = 68;                    // floats per staging row
    const float kap = J == 3 ? -1.f : 1.f;
    float* wt = reinterpret_cast<float*>((wave >> 1) == 0 ? lx0 : (wave >> 1) == 1 ? lx1 : (wave >> 1) == 2 ? lg0 : lg1) +
                (wave & 1) * (32 * TP);
    const int ln = lane & 31, lh = lane >> 5;
    const int rr = lane >> 4, rc = (lane & 15) * 4;
    float* obase = slab + (long long)(ny * 128 + wn * 32 + rr) * p.Kcp + c_lo + wc * 64 + rc;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 t;
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) {
                    const int idx = 4 * q + ee;
                    const float m0 = acc[4 * f][idx], m1 = acc[4 * f + 1][idx];
                    const float m2 = acc[4 * f + 2][idx], m3 = -acc[4 * f + 3][idx];
                    const float hs = 0.5f * (m1 + m2);
                    t[ee] = kap * (r == 0 ? m0 + hs : r == 1 ? 0.5f * (m1 - m2) : hs + m3);
                }
                *reinterpret_cast<f32x4*>(wt + ln * TP + 32 * f + 8 * q + 4 * lh) = t;
            }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wt + (rr + 4 * it) * TP + rc);
            *reinterpret_cast<f32x4*>(obase + (long long)(4 * it) * p.Kcp + r * p.C) = v;
        }
    }
}

}  // namespace pu
