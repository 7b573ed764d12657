// Weight (and bias) gradients of the convolutions as split-K fp32 MFMA GEMMs.
//
// Replaces the autograd weight/bias backward of nn.Conv2d (src/unet/unet_p.py:184-201) and
// nn.ConvTranspose2d (unet_p.py:238) that loss.backward() (src/train.py:110) runs on the CPU.
//
//   out[n][k] = sum_m P[m][n] * Q[m][k]      m = pixel rows (B*H*W), split over grid.z
//   P = rows operand (conv: dZ; ConvT: its low-res input), Q = im2col of src0|src1 at tap(k)
//   bias_mode 1 adds a ones COLUMN (k == K)  -> dbias[n]  = sum_m P[m][n]
//   bias_mode 2 adds a ones ROW    (n == N)  -> dbias[c] = sum_taps sum_m Q[m][(tap,c)]
// MFMA mapping (32x32x2): lane (i, h) supplies A[i][h] = P[m0+h][n_i] and B[h][j] = Q[m0+h][k_j],
// both read from LDS with ds_read_b32 (32 consecutive floats per half-wave: conflict-free).
// Partial tiles go to a per-split slab; wgrad_reduce sums the splits in a fixed order
// (deterministic) and writes PyTorch's [n][c][kh][kw] layout.
//
// This file holds the parameter block, what the kernels share, the plan, the launchers and the
// entries; the kernels are in wgrad_gemm.h, wgrad_halo.h, wgrad_wino.h, wgrad_direct.h and
// wgrad_reduce.h, by family.
#include "mfma_common.h"
#include <type_traits>

#ifndef PU_NO_ILV
#define PU_NO_ILV 0   // 1: leave MFMA / VALU placement to the scheduler (A/B builds)
#endif

namespace pu {


constexpr int WG_BM = 16;  // pixel rows per LDS stage

// The launch parameters over the operand element type T (float | __bf16); the slab is fp32 on both
// paths.  One layout, in the order the fp32 kernels were compiled with: regrouping the fields to
// set the fp32-only ones (Kc, batch, tiles_w, tiles_h) apart changed the scalar loads of every
// fp32 kernel, so the bf16 kernels carry four integers they do not read.
template <typename T>
struct WgradParamsT {
    int M, N, Nr, K, Kc, C, c0, c1;   // Kc: slab columns in use, K (+ 1 bias column)
    int Hi, Wi, Ho, Wo, kw, stride, pad;
    const T* P;
    const T* src0;
    const T* src1;
    int bias_mode;
    float* slab;
    int mps;  // pixel rows per split (multiple of the stage's rows)
    int gx, gy;  // k-tiles, n-tiles
    int Kcp;     // slab row stride (Kc rounded up to 4)
    int batch, tiles_w, tiles_h;   // direct kernels: pixel tiles of an image
    FastDiv dWo, dHo, dC, dKw;
};
struct WgradParams : WgradParamsT<float> {};
struct WgradBf16Params : WgradParamsT<__bf16> {};

// The block's place in the grid.  XCD-aware order: logical tile = (split z, n-tile y, k-tile x), x
// fastest; each XCD walks a contiguous range, so the k-tiles that re-read the same pixel rows share
// its L2.  Split z covers pixel rows [m_begin, m_end).
struct WgradBlock {
    int tx, ty, tz, m_begin, m_end;
};
template <typename P>
__device__ __forceinline__ WgradBlock wgrad_block(const P& p) {
    WgradBlock b;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    b.tx = tile % p.gx;
    const int tyz = tile / p.gx;
    b.ty = tyz % p.gy;
    b.tz = tyz / p.gy;
    b.m_begin = b.tz * p.mps;
    b.m_end = min(p.M, b.m_begin + p.mps);
    return b;
}

// One 32 x 32 accumulator fragment's values of this lane - 4 consecutive k at columns k + 8 q,
// q = 0..3, of one n - into the lane's slab row as float4; CHECK: columns from K on are dropped
template <bool CHECK>
__device__ __forceinline__ void store_frag(float* row, const f32x16& acc, int k, int K) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (CHECK && k + 8 * q >= K) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[4 * q + e];
        *reinterpret_cast<f32x4*>(row + (k + 8 * q)) = v;
    }
}

// the zero page of every kernel: padding, out-of-image taps and stages past a split's end read
// these 16 bytes (4 fp32 or 8 bf16)
__device__ __attribute__((aligned(16))) float g_wg_zero16[4] = {0.f, 0.f, 0.f, 0.f};

}  // namespace pu

// the kernels by family, each file once and in this order; one translation unit
#include "wgrad_gemm.h"
#include "wgrad_halo.h"
#include "wgrad_wino.h"
#include "wgrad_direct.h"
#include "wgrad_reduce.h"

namespace pu {

// ------------------------------------------------------------------ host: plan, launch, reduce
// One plan per call, fp32 and bf16 entries alike: which phase-1 kernel runs (kind), how its grid
// and slab are shaped, and which phase-2 reduction finishes it (reducer).
enum WgradKind {
    WK_STEM,        // wgrad_stem_kernel: the single-channel 3x3 stem, fp32 or bf16 rows
    WK_PW,          // wgrad_pw_kernel: 1x1 on 3 or 4 input channels
    WK_SMALL,       // wgrad_small_kernel: 3x3 on up to 16 x 16 channels
    WK_WINO,        // wgrad_wino_x6_kernel: Winograd domain, 64 x 64 channel blocks
    WK_WINO_COLS,   // wgrad_wino_cols_x6_kernel: 128 x 128 blocks, one position column each
    WK_HALO,        // wgrad_halo_x6_kernel
    WK_DMA,         // wgrad_dma_kernel: GEMM tile, float4 sources straight to LDS
    WK_REG,         // wgrad_kernel: GEMM tile, register-staged scalar loader
    WK_BF16,        // wgrad_bf16_kernel: 128 x 128 GEMM tile
    WK_BF16_HALO,   // wgrad_halo_bf16_kernel
};

enum WgradReducer {
    RD_COLS,        // wgrad_finish_cols_kernel: combines the column plan's pages
    RD_WIDE,        // wgrad_reduce_wide_kernel: one launch
    RD_SPLITS,      // a finisher over the fp32 splits
    RD_GROUPS,      // wgrad_sum_splits4_kernel into G fp64 partials, then a finisher over those
};

struct WgradPlan {
    WgradKind kind;
    WgradReducer reducer;
    bool fq = false;            // WK_DMA: the tile's FQ form
    bool transposed = false;    // RD_SPLITS / RD_GROUPS: the transposed finisher, not the quad one
    bool dw_vec = false;        // RD_COLS: float4 stores (dweight 16-byte aligned)
    int M, K, C, Nr, Kc, Kcp;   // the GEMM and its [Nr][Kcp] result (plan_dims)
    int BN, BK, gx, gy, splits, mps;
    int G;                      // reduction groups whose fp64 partials lie in the workspace
    // the slab is splits x pages pages of [Nr][pKcp] floats with the bias at column pK: one page
    // of the whole result per split, but the column plan's 4 position columns write [Nr][3 C (+ 1)]
    int pages, pK, pKc, pKcp;
    int fin_groups = 1;         // RD_COLS: the groups its finisher sums the splits in
    int tiles = 0, tps = 0;     // Winograd kinds: 2 x 2 output tiles, tiles per split
    int nt = 1;                 // halo kinds: 64-channel output tiles per block
    int tiles_w = 0, tiles_h = 0;   // direct kinds: pixel tiles of an image
    size_t slab_bytes() const { return (size_t)splits * pages * Nr * pKcp * sizeof(float); }
    size_t part_bytes() const { return G > 1 ? (size_t)G * Nr * Kcp * sizeof(double) : 0; }
    size_t ws_bytes() const { return ((slab_bytes() + 255) / 256) * 256 + part_bytes(); }
};

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool same_3x3(const pu_wgrad_args* a) {
    return a->kh == 3 && a->kw == 3 && a->stride == 1 && a->pad == 1 && a->in_h == a->out_h && a->in_w == a->out_w;
}

static bool stem_wgrad_ok(const pu_wgrad_args* a) {
    return a->c0 == 1 && a->c1 == 0 && (a->n == 8 || a->n == 16 || a->n == 32 || a->n == 64) && same_3x3(a) &&
           a->bias_mode == 1 && aligned16(a->rows);
}

// 1x1 / s1 / p0 same-size conv, one source, (C, N) an instantiated wgrad_pw_kernel pair
static bool pw_wgrad_ok(const pu_wgrad_args* a) {
    const int C = a->c0, N = a->n;
    return a->c1 == 0 && a->kh == 1 && a->kw == 1 && a->stride == 1 && a->pad == 0 && a->in_h == a->out_h &&
           a->in_w == a->out_w && a->bias_mode != 2 && (C == 3 || C == 4) && (N == 4 || N == 8 || N == 16) &&
           aligned16(a->rows) && (C % 4 || aligned16(a->src0));
}

static bool small_wgrad_ok(const pu_wgrad_args* a) {
    const int C = a->c0 + a->c1;
    return (C == 1 || C == 4 || C == 8 || C == 12 || C == 16) && (a->n == 4 || a->n == 8 || a->n == 16) &&
           same_3x3(a) && a->bias_mode != 2 && (C == 1 || (a->c0 % 4 == 0 && a->c1 % 4 == 0));
}

// the halo kernels: 3x3 / s1 / p1 same-size, 16-pixel stages within a row, 64-channel blocks
static bool halo_wgrad_ok(const pu_wgrad_args* a, const WgradPlan* pl) {
    return same_3x3(a) && a->out_w % 16 == 0 && a->c0 % 64 == 0 && a->c1 % 64 == 0 && a->n % 64 == 0 &&
           a->bias_mode != 2 && (long long)pl->M * pl->C < (1LL << 31);
}

// the Winograd-domain kernels: 3x3 / s1 / p1 on an even same-size grid, 64-channel input blocks
// from one source each, 64-channel output blocks, the 6-product arithmetic, byte offsets of the
// (shifted) sources and of dZ under 2^31
static bool wino_wgrad_ok(const pu_wgrad_args* a) {
    if (a->math != 1 || !same_3x3(a) || (a->out_h & 1) || (a->out_w & 1)) return false;
    if (a->c0 % 64 || a->c1 % 64 || a->n % 64 || a->bias_mode == 2) return false;
    const long long px = (long long)a->batch * a->in_h * a->in_w + a->in_w + 1;
    if (px * (a->c0 > a->c1 ? a->c0 : a->c1) * 4 >= (1LL << 31)) return false;
    if ((long long)a->batch * a->out_h * a->out_w * a->n * 4 >= (1LL << 31)) return false;
    return (((uintptr_t)a->rows | (uintptr_t)a->src0 | (uintptr_t)a->src1) & 7) == 0;
}

// Fewest tiles at which the column plan (wgrad_wino_cols_x6_kernel) is taken: C2's smallest qualifying
// layers (the 8 x 8 level at batch 32) have 512; the measured gate is in DESIGN.md section 2.
constexpr int WWR_MIN_TILES = 512;

// reduction groups: one pass (1 group, each thread sums every split of its entry) when the result
// has enough entries to fill the chip; otherwise groups of >= 8 splits each, then as many partials
static int reduce_groups(long long total, int splits) {
    int G = (int)ceil_div(262144LL, total);
    const int by_len = ceil_div(splits, 8);
    if (G > by_len) G = by_len;
    if (G > 16) G = 16;
    return G < 1 ? 1 : G;
}

// the GEMM's dimensions and the slab's shape, fp32 and bf16 alike: M pixel rows, K = taps x C,
// Nr x Kc slab entries with the bias as row N (mode 2) or column K (mode 1).  Kcp, the slab's row
// stride, is Kc rounded up to 4 floats: phase 2 reads and sums every slab as 16-byte quads.
static int plan_dims(const pu_wgrad_args* a, WgradPlan* pl, const char* who) {
    const long long M = (long long)a->batch * a->out_h * a->out_w;
    PU_REQUIRE(M < (1LL << 31), "%s: too many pixels", who);
    pl->M = (int)M;
    pl->C = a->c0 + a->c1;
    pl->K = a->kh * a->kw * pl->C;
    pl->Nr = a->n + (a->bias_mode == 2 ? 1 : 0);
    pl->Kc = pl->K + (a->bias_mode == 1 ? 1 : 0);
    pl->Kcp = (pl->Kc + 3) / 4 * 4;
    pl->pages = 1;
    pl->pK = pl->K;
    pl->pKc = pl->Kc;
    pl->pKcp = pl->Kcp;
    return PU_OK;
}

// the halo kernels (wgrad_halo_x6_kernel, wgrad_halo_bf16_kernel): 64 NT x 64 x 9-tap tiles,
// 16-pixel stages split so that one round of blocks fills the chip
static void plan_halo(const pu_wgrad_args* a, WgradKind kind, WgradPlan* pl) {
    pl->kind = kind;
    pl->nt = a->n % 128 == 0 ? 2 : 1;    // 128 output channels per block when they divide
    pl->BN = 64 * pl->nt;
    pl->BK = 9 * 64;
    pl->gx = pl->C / 64;
    pl->gy = a->n / pl->BN;
    int splits = (pl->nt == 2 ? 256 : 512) / (pl->gx * pl->gy);   // one 8-wave / two 4-wave blocks per CU
    const int stages = pl->M / 16;
    if (splits > stages) splits = stages;
    if (splits < 1) splits = 1;
    pl->mps = ceil_div(stages, splits) * 16;
    pl->splits = ceil_div(pl->M, pl->mps);
}

// the Winograd-domain kernels, one 512-thread block per CU: (C / cb) x (N / cb) channel blocks x
// tile splits of whole 16-tile stages, with cb = 64, or with cb = 128 x 4 position columns when the
// channels divide and there are tiles enough.  A column writes its own page of [Nr][3 C (+ 1 bias
// column)] entries, and the finisher sums the splits in the groups the whole result would get.
static void plan_wino(const pu_wgrad_args* a, WgradPlan* pl) {
    pl->tiles = a->batch * (a->out_h / 2) * (a->out_w / 2);
    const bool cols = a->c0 % 128 == 0 && a->c1 % 128 == 0 && a->n % 128 == 0 && pl->tiles >= WWR_MIN_TILES;
    const int cb = cols ? 128 : 64;
    pl->kind = cols ? WK_WINO_COLS : WK_WINO;
    pl->BN = cb;
    pl->BK = cols ? 3 * 128 : 9 * 64;
    pl->gx = pl->C / cb;
    pl->gy = a->n / cb;
    const int stages = ceil_div(pl->tiles, 16);
    int splits = 256 / ((cols ? 4 : 1) * pl->gx * pl->gy);
    if (splits > stages) splits = stages;
    if (splits < 1) splits = 1;
    pl->tps = ceil_div(stages, splits) * 16;
    pl->splits = ceil_div(pl->tiles, pl->tps);
    pl->mps = pl->tps * 4;
    if (cols) {
        pl->pages = 4;
        pl->pK = 3 * pl->C;
        pl->pKc = pl->pK + (a->bias_mode == 1 ? 1 : 0);
        pl->pKcp = (pl->pKc + 3) / 4 * 4;
    }
}

// Measured alternatives: capping the GEMM-path split count at 2 / 4 (round 3: C2 4060 -> 2262 /
// 2968 img/s - the deep layers' slab traffic is cheaper than idle CUs); round 1: 64 x 576 6-wave tiles for the 64-channel layers (-6 %), a
// 3-wave 64 x 192 tile (-8 %), a split-once-planes kernel that still staged fp32 through LDS
// (-10...-25 %); the halo kernel replaced all of them on 3x3/s1 layers.
static void plan_f32(const pu_wgrad_args* a, WgradPlan* pl) {
    const long long M = pl->M;
    if (pw_wgrad_ok(a)) {              // pointwise: contiguous pixel ranges, one slab row block each
        pl->kind = WK_PW;
        pl->splits = (int)(M / 256 < 1024 ? (M + 255) / 256 : 1024);
        pl->mps = (int)ceil_div(M, (long long)pl->splits);
        pl->splits = (int)ceil_div(M, (long long)pl->mps);
        pl->BN = a->n; pl->BK = pl->K; pl->gx = pl->gy = 1;
        return;
    }
    if (stem_wgrad_ok(a) || small_wgrad_ok(a)) {   // direct kernels: one slab row block per block
        const bool stem = stem_wgrad_ok(a);
        pl->kind = stem ? WK_STEM : WK_SMALL;
        pl->tiles_w = ceil_div(a->out_w, stem ? SWS_TW : SW_TW);
        pl->tiles_h = ceil_div(a->out_h, stem ? SWS_TH : SW_TH);
        const long long ntiles = (long long)a->batch * pl->tiles_w * pl->tiles_h;
        pl->splits = (int)(ntiles < 1024 ? ntiles : 1024);
        pl->BN = a->n; pl->BK = pl->K; pl->gx = pl->gy = 1; pl->mps = 0;
        return;
    }
    if (wino_wgrad_ok(a)) return plan_wino(a, pl);
    if (a->math == 1 && halo_wgrad_ok(a, pl)) return plan_halo(a, WK_HALO, pl);
    // the direct-to-LDS kernel (float4 sources) tiles only the N x K GEMM (bias via LDS column
    // sums); the register-staged kernel carries the bias as an extra ones column / row
    const bool dma = a->c0 % 4 == 0 && a->c1 % 4 == 0;
    pl->kind = dma ? WK_DMA : WK_REG;
    pl->fq = dma && a->math == 1 && a->stride == 1 && a->in_h == a->out_h && a->in_w == a->out_w && a->out_w >= 4;
    const int ext_n = dma ? a->n : pl->Nr;
    const int ext_k = dma ? pl->K : pl->Kc;
    int occ;  // resident blocks per CU (LDS / VGPR limited, from the resource-usage report)
    if (ext_k <= 64) { pl->BN = 64; pl->BK = 64; occ = dma ? 6 : 7; }
    else if (ext_n <= 64 && !dma) { pl->BN = 64; pl->BK = 256; occ = 3; }
    else if (ext_n <= 32 && a->math == 1) { pl->BN = 32; pl->BK = 128; occ = 4; }   // 32-channel layers (C4/C5)
    else if (ext_n <= 64) {
        // BK 128 (4 resident blocks) unless 192 (3 resident) pads k less - e.g. K = 9 taps x 64
        const bool b192 = ceil_div(ext_k, 192) * 192 < ceil_div(ext_k, 128) * 128;
        pl->BN = 64; pl->BK = b192 ? 192 : 128; occ = b192 ? 3 : 4;
    }
    else { pl->BN = 128; pl->BK = 128; occ = dma ? 3 : 4; }
    // 6-product path: a 128 x 256 tile (2x2 waves of 64 x 128) splits 6 operand fragments per 48
    // MFMAs instead of 4 per 24, when K pads no worse than with 128
    if (a->math == 1 && dma && pl->BN == 128 && ceil_div(ext_k, 256) * 256 <= ceil_div(ext_k, 128) * 128) {
        pl->BK = 256;
        occ = 2;
    }
    pl->gx = ceil_div(ext_k, pl->BK);
    pl->gy = ceil_div(ext_n, pl->BN);
    // one full round of resident blocks: a grid a few blocks past a multiple of the resident
    // slots costs a whole extra round
    int splits = 256 * occ / (pl->gx * pl->gy);
    const int max_splits = ceil_div(M, 256);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    pl->mps = ceil_div(ceil_div(M, splits), WG_BM) * WG_BM;
    pl->splits = ceil_div(M, pl->mps);
}

// bf16: the halo kernel, or 128 x 128 tiles of the N x K GEMM (bias via LDS column sums), pixel rows
// split so that one round of resident blocks (3 per CU: 48 KB ring) fills the chip
static void plan_bf16(const pu_wgrad_args* a, WgradPlan* pl) {
    if (halo_wgrad_ok(a, pl)) return plan_halo(a, WK_BF16_HALO, pl);
    pl->kind = WK_BF16;
    pl->BN = WB_W; pl->BK = WB_W;
    pl->gx = ceil_div(pl->K, WB_W);
    pl->gy = ceil_div(a->n, WB_W);
    int splits = 768 / (pl->gx * pl->gy);
    const int max_splits = ceil_div(pl->M, 512);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    pl->mps = ceil_div(ceil_div(pl->M, splits), WB_ROWS) * WB_ROWS;
    pl->splits = ceil_div(pl->M, pl->mps);
}

// Phase 2 of every weight-gradient path is a fixed-order fp64 reduction of the split partials and
// the store into PyTorch's [n][c][kh][kw] (+ bias).
// The one-launch wide reduction takes the direct small-channel / stem / pointwise plans (up to
// 1024 splits of a few-thousand-entry slab) and the other non-Winograd plans whose slabs are short
// (Nr x Kcp <= WR_WIDE_MAX entries: C4 / C5's 32-channel weight gradients, 9216 entries over
// hundreds of splits), where the grouped form is two latency-bound launches: C5 +0.8 %, C4 +0.7 %
// (`r06_experiments/wgrad_reduce_wide_ab.txt`).  Long slabs (C2 / C3, >= 32K entries) keep the
// grouped form: the wide one took C3's bf16 reductions from 0.36 to 1.39 ms per step, and the
// Winograd-domain kernel's 64-256 splits from 0.32 to 0.37 ms per C2 step.
// The split partials are summed in fp64 either way, in a different fixed order.
constexpr long long WR_WIDE_MAX = 16384;

static void plan_reducer(const pu_wgrad_args* a, WgradPlan* pl) {
    const long long total = (long long)pl->Nr * pl->Kcp;
    const int groups = reduce_groups(total, pl->splits);
    const bool direct = pl->kind == WK_STEM || pl->kind == WK_PW || pl->kind == WK_SMALL;
    pl->dw_vec = aligned16(a->dweight);
    pl->transposed = a->bias_mode != 2 && a->kh * a->kw <= 9 && pl->C % 4 == 0 && pl->dw_vec;
    pl->G = groups;
    if (pl->kind == WK_WINO_COLS) {
        pl->reducer = RD_COLS;
        pl->fin_groups = groups;
        pl->G = 1;                            // its partials stay in LDS: none in the workspace
    } else if ((direct || (pl->kind != WK_WINO && total <= WR_WIDE_MAX)) && a->bias_mode != 2) {
        pl->reducer = RD_WIDE;
    } else {
        pl->reducer = groups > 1 ? RD_GROUPS : RD_SPLITS;
    }
}

// The two entries differ in what their kernels ask of n, c0 and c1, in the math argument (fp32
// only) and in the tile choice.
static int plan_wgrad(const pu_wgrad_args* a, bool bf16, WgradPlan* pl) {
    const char* who = bf16 ? "pu_wgrad_bf16" : "pu_wgrad";
    PU_REQUIRE(a && a->batch > 0 && a->out_h > 0 && a->out_w > 0 && a->in_h > 0 && a->in_w > 0, "%s: bad grid", who);
    PU_REQUIRE(a->kh > 0 && a->kw > 0 && a->stride > 0 && a->pad >= 0, "%s: bad taps", who);
    PU_REQUIRE(a->rows && a->n > 0 && a->src0 && a->c0 > 0 && (a->c1 == 0 || a->src1), "%s: operands", who);
    if (bf16)
        PU_REQUIRE(a->n % 8 == 0 && a->c0 % 8 == 0 && a->c1 % 8 == 0,
                   "%s: n (%d) and channel counts (%d, %d) must be multiples of 8", who, a->n, a->c0, a->c1);
    else
        PU_REQUIRE(a->n % 4 == 0, "%s: n (%d) must be a multiple of 4", who, a->n);
    PU_REQUIRE(a->bias_mode >= 0 && a->bias_mode <= 2, "%s: bias_mode", who);
    PU_REQUIRE(a->bias_mode == 0 || a->dbias, "%s: dbias missing", who);
    PU_REQUIRE(a->dweight, "%s: dweight missing", who);
    if (!bf16) {
        PU_REQUIRE(a->math >= 0 && a->math <= 2, "%s: math %d", who, a->math);
        PU_REQUIRE(a->math != 2 || stem_wgrad_ok(a), "%s: math 2 (bf16 rows) is the single-channel stem only", who);
    }
    if (int st = plan_dims(a, pl, who)) return st;
    if (bf16 || (a->c0 % 4 == 0 && a->c1 % 4 == 0))   // sources read as 16-byte quads
        PU_REQUIRE(aligned16(a->src0) && aligned16(a->src1), "%s: sources must be 16-byte aligned", who);
    PU_REQUIRE(aligned16(a->rows), "%s: rows must be 16-byte aligned", who);
    if (bf16) plan_bf16(a, pl);
    else plan_f32(a, pl);
    plan_reducer(a, pl);
    return PU_OK;
}

template <typename T>
static void fill_params(const WgradPlan& pl, const pu_wgrad_args* a, void* workspace, WgradParamsT<T>* p) {
    p->M = pl.M; p->N = a->n; p->Nr = pl.Nr; p->K = pl.pK; p->Kc = pl.pKc; p->Kcp = pl.pKcp;
    p->C = pl.C; p->c0 = a->c0; p->c1 = a->c1;
    p->Hi = a->in_h; p->Wi = a->in_w; p->Ho = a->out_h; p->Wo = a->out_w;
    p->kw = a->kw; p->stride = a->stride; p->pad = a->pad;
    p->P = (const T*)a->rows; p->src0 = (const T*)a->src0; p->src1 = (const T*)a->src1;
    p->bias_mode = a->bias_mode;
    p->slab = (float*)workspace; p->mps = pl.mps; p->gx = pl.gx; p->gy = pl.gy;
    p->batch = a->batch; p->tiles_w = pl.tiles_w; p->tiles_h = pl.tiles_h;
    p->dWo = make_fastdiv(a->out_w); p->dHo = make_fastdiv(a->out_h);
    p->dC = make_fastdiv(pl.C); p->dKw = make_fastdiv(a->kw);
}

template <int N>
static void launch_stem(bool bf16_rows, dim3 grid, hipStream_t s, const WgradParams& p) {
    if (bf16_rows) hipLaunchKernelGGL((wgrad_stem_kernel<N, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wgrad_stem_kernel<N, false>), grid, dim3(256), 0, s, p);
}

// a DMA tile in the form the plan names: FQ, 6-product, or (PLAIN: where it is built) 3-product
template <int BN, int BK, int WN, int WK, bool PLAIN = true>
static void launch_dma(const WgradPlan& pl, bool x6, dim3 grid, hipStream_t s, const WgradParams& p) {
    if (pl.fq) hipLaunchKernelGGL((wgrad_dma_kernel<BN, BK, WN, WK, 3, true, 4, true>), grid, dim3(256), 0, s, p);
    else if (x6 || !PLAIN) hipLaunchKernelGGL((wgrad_dma_kernel<BN, BK, WN, WK, 3, true>), grid, dim3(256), 0, s, p);
    else if constexpr (PLAIN) hipLaunchKernelGGL((wgrad_dma_kernel<BN, BK, WN, WK, 3, false>), grid, dim3(256), 0, s, p);
}

// phase 1: the plan's kernel writes the split partials into the slab
static int wgrad_launch(const WgradPlan& pl, const pu_wgrad_args* a, void* workspace, hipStream_t s) {
    const dim3 grid(pl.gx * pl.gy * pl.splits * pl.pages);
    const int C = pl.C, N = a->n;
    const char* what = "pu_wgrad (gemm)";
    WgradParams p;             // the fp32 kinds'
    WgradBf16Params b;         // the bf16 kinds'
    if (pl.kind == WK_BF16 || pl.kind == WK_BF16_HALO) fill_params(pl, a, workspace, &b);
    else fill_params(pl, a, workspace, &p);
    switch (pl.kind) {
    case WK_STEM:
        what = "pu_wgrad (stem)";
        if (N == 64) launch_stem<64>(a->math == 2, grid, s, p);
        else if (N == 32) launch_stem<32>(a->math == 2, grid, s, p);
        else if (N == 16) launch_stem<16>(a->math == 2, grid, s, p);
        else launch_stem<8>(a->math == 2, grid, s, p);
        break;
    case WK_PW:
        what = "pu_wgrad (pointwise)";
#define PU_PW(C_, N_) if (C == C_ && N == N_) hipLaunchKernelGGL((wgrad_pw_kernel<C_, N_>), grid, dim3(256), 0, s, p)
        PU_PW(3, 4); else PU_PW(3, 8); else PU_PW(3, 16); else PU_PW(4, 4); else PU_PW(4, 8); else PU_PW(4, 16);
#undef PU_PW
        break;
    case WK_SMALL:
        what = "pu_wgrad (small-channel)";
#define PU_SW(C_, N_) if (C == C_ && N == N_) hipLaunchKernelGGL((wgrad_small_kernel<C_, N_>), grid, dim3(256), 0, s, p)
        PU_SW(1, 4); else PU_SW(1, 8); else PU_SW(1, 16); else PU_SW(4, 4); else PU_SW(4, 8); else PU_SW(4, 16);
        else PU_SW(8, 4); else PU_SW(8, 8); else PU_SW(8, 16); else PU_SW(12, 4); else PU_SW(12, 8);
        else PU_SW(12, 16); else PU_SW(16, 4); else PU_SW(16, 8); else PU_SW(16, 16);
#undef PU_SW
        break;
    case WK_WINO:
    case WK_WINO_COLS: {
        WinoWgradParams ww;
        ww.p = p;
        ww.tiles = pl.tiles;
        ww.tps = pl.tps;
        ww.dTw = make_fastdiv(a->out_w / 2);
        ww.dTh = make_fastdiv(a->out_h / 2);
        const long long px = (long long)a->batch * a->in_h * a->in_w + a->in_w + 1;
        ww.x0_bytes = (unsigned)(px * a->c0 * 4);
        ww.x1_bytes = (unsigned)(px * a->c1 * 4);
        ww.p_bytes = (unsigned)((long long)pl.M * a->n * 4);
        if (pl.kind == WK_WINO_COLS) hipLaunchKernelGGL(wgrad_wino_cols_x6_kernel, grid, dim3(512), 0, s, ww);
        else hipLaunchKernelGGL(wgrad_wino_x6_kernel, grid, dim3(512), 0, s, ww);
        break;
    }
    case WK_HALO:
        if (pl.nt == 2) hipLaunchKernelGGL(wgrad_halo_x6_kernel<2>, grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL(wgrad_halo_x6_kernel<1>, grid, dim3(256), 0, s, p);
        break;
    case WK_DMA:
        if (pl.BK == 64) launch_dma<64, 64, 2, 2>(pl, a->math == 1, grid, s, p);
        else if (pl.BN == 64 && pl.BK == 128) launch_dma<64, 128, 2, 2>(pl, a->math == 1, grid, s, p);
        else if (pl.BN == 32) launch_dma<32, 128, 1, 4, false>(pl, true, grid, s, p);      // planned under math 1 only
        else if (pl.BK == 192) launch_dma<64, 192, 2, 2>(pl, a->math == 1, grid, s, p);
        else if (pl.BK == 256) launch_dma<128, 256, 2, 2, false>(pl, true, grid, s, p);    // likewise
        else launch_dma<128, 128, 2, 2>(pl, a->math == 1, grid, s, p);
        break;
    case WK_REG:
#define PU_WG_REG(BN_, BK_, WN_, WK_) hipLaunchKernelGGL((wgrad_kernel<BN_, BK_, WN_, WK_, false>), grid, dim3(256), 0, s, p)
        if (pl.BK == 64) PU_WG_REG(64, 64, 2, 2);
        else if (pl.BK == 256) PU_WG_REG(64, 256, 1, 4);
        else PU_WG_REG(128, 128, 2, 2);
#undef PU_WG_REG
        break;
    case WK_BF16:
        what = "pu_wgrad_bf16 (gemm)";
        hipLaunchKernelGGL(wgrad_bf16_kernel, grid, dim3(256), 0, s, b);
        break;
    case WK_BF16_HALO:
        what = "pu_wgrad_bf16 (gemm)";
        if (pl.nt == 2) hipLaunchKernelGGL(wgrad_halo_bf16_kernel<2>, grid, dim3(512), 0, s, b);
        else hipLaunchKernelGGL(wgrad_halo_bf16_kernel<1>, grid, dim3(256), 0, s, b);
        break;
    }
    return check_launch(what);
}

// the transposed (coalesced float4 stores) or the quad (scattered stores) finisher over `count`
// partials: the fp32 slab's splits, or the fp64 partials of wgrad_sum_splits4_kernel
template <typename T>
static void launch_finisher(const T* part, int count, const WgradPlan& pl, const pu_wgrad_args* a, hipStream_t s) {
    const int taps = a->kh * a->kw;
    if (pl.transposed) {
        hipLaunchKernelGGL(wgrad_finish_t_kernel<T>, dim3((unsigned)ceil_div(pl.C, 256), (unsigned)a->n),
                           dim3((unsigned)(64 * taps)), 0, s, part, count, pl.Nr, pl.Kcp, pl.K, pl.C, taps, a->bias_mode,
                           a->dweight, a->dbias, a->accumulate);
        return;
    }
    const long long threads = (long long)pl.Nr * pl.Kcp / 4 + (a->bias_mode == 2 ? pl.C : 0);
    hipLaunchKernelGGL(wgrad_finish4_kernel<T>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, part, count,
                       pl.Nr, pl.Kcp, a->n, pl.K, pl.C, a->kh, a->kw, a->bias_mode, a->dweight, a->dbias, a->accumulate);
}

// phase 2: the plan's reduction of the slab into dweight (+ dbias)
static int wgrad_reduce(const WgradPlan& pl, const pu_wgrad_args* a, void* workspace, hipStream_t s) {
    const long long total = (long long)pl.Nr * pl.Kcp;
    const float* slab = (const float*)workspace;
    switch (pl.reducer) {
    case RD_COLS:
        hipLaunchKernelGGL(wgrad_finish_cols_kernel, dim3((unsigned)ceil_div(pl.C, 256), (unsigned)a->n),
                           dim3(192 * pl.fin_groups), 0, s, slab, pl.splits, pl.fin_groups, pl.Nr, pl.pKcp, pl.C,
                           a->bias_mode, a->dweight, a->dbias, a->accumulate, (int)pl.dw_vec);
        break;
    case RD_WIDE:
        hipLaunchKernelGGL(wgrad_reduce_wide_kernel, dim3((unsigned)ceil_div(total, (long long)WR_E)), dim3(256), 0, s,
                           slab, pl.splits, total, a->n, pl.Kcp, pl.K, pl.C, a->kh, a->kw, a->bias_mode, a->dweight,
                           a->dbias, a->accumulate);
        break;
    case RD_SPLITS:
        launch_finisher(slab, pl.splits, pl, a, s);
        break;
    case RD_GROUPS: {
        double* part = (double*)((char*)workspace + ((pl.slab_bytes() + 255) / 256) * 256);
        hipLaunchKernelGGL(wgrad_sum_splits4_kernel, dim3((unsigned)((total / 4 + 255) / 256), pl.G), dim3(256), 0, s,
                           slab, pl.splits, total, pl.G, part);
        launch_finisher((const double*)part, pl.G, pl, a, s);
        break;
    }
    }
    return check_launch("pu_wgrad (reduce)");
}

static int run_wgrad(const pu_wgrad_args* a, bool bf16, void* workspace, size_t ws_bytes, int phase, void* stream) {
    const char* who = bf16 ? "pu_wgrad_bf16" : "pu_wgrad";
    PU_REQUIRE(phase >= 1 && phase <= 3, "%s_phase: phase %d", who, phase);
    WgradPlan pl;
    if (int st = plan_wgrad(a, bf16, &pl)) return st;
    const size_t need = pl.ws_bytes();
    if (!workspace || ws_bytes < need) return fail(PU_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    hipStream_t s = as_stream(stream);
    if (phase & 1)
        if (int st = wgrad_launch(pl, a, workspace, s)) return st;
    return (phase & 2) ? wgrad_reduce(pl, a, workspace, s) : PU_OK;
}

static size_t wgrad_workspace_bytes(const pu_wgrad_args* a, bool bf16) {
    WgradPlan pl;
    return plan_wgrad(a, bf16, &pl) == PU_OK ? pl.ws_bytes() : 0;
}

// the tile queries' third value: which kind of kernel the plan names (plastic_unet.h)
static int tile_code(WgradKind kind) {
    switch (kind) {
    case WK_REG: return 0;
    case WK_DMA: return 1;
    case WK_SMALL: return 2;
    case WK_HALO: return 3;
    case WK_STEM: return 4;
    case WK_WINO:
    case WK_WINO_COLS: return 5;
    case WK_PW: return 6;
    case WK_BF16: return 0;
    case WK_BF16_HALO: return 1;
    }
    return -1;
}

static int wgrad_tile(const pu_wgrad_args* a, bool bf16, int* bn, int* bk, int* code, int* splits) {
    WgradPlan pl;
    if (int st = plan_wgrad(a, bf16, &pl)) return st;
    if (bn) *bn = pl.BN;
    if (bk) *bk = pl.BK;
    if (code) *code = tile_code(pl.kind);
    if (splits) *splits = pl.splits * pl.pages;
    return PU_OK;
}

}  // namespace pu

using namespace pu;

extern "C" size_t pu_wgrad_workspace_bytes(const pu_wgrad_args* a) { return wgrad_workspace_bytes(a, false); }

extern "C" int pu_wgrad_tile(const pu_wgrad_args* a, int* bn, int* bk, int* qvec, int* splits) {
    return wgrad_tile(a, false, bn, bk, qvec, splits);
}

extern "C" int pu_wgrad(const pu_wgrad_args* a, void* workspace, size_t ws_bytes, void* stream) {
    return run_wgrad(a, false, workspace, ws_bytes, 3, stream);
}

extern "C" int pu_wgrad_phase(const pu_wgrad_args* a, void* workspace, size_t ws_bytes, int phase, void* stream) {
    return run_wgrad(a, false, workspace, ws_bytes, phase, stream);
}

extern "C" size_t pu_wgrad_bf16_workspace_bytes(const pu_wgrad_args* a) { return wgrad_workspace_bytes(a, true); }

extern "C" int pu_wgrad_bf16_tile(const pu_wgrad_args* a, int* bn, int* bk, int* halo, int* splits) {
    return wgrad_tile(a, true, bn, bk, halo, splits);
}

extern "C" int pu_wgrad_bf16(const pu_wgrad_args* a, void* workspace, size_t ws_bytes, void* stream) {
    return run_wgrad(a, true, workspace, ws_bytes, 3, stream);
}

extern "C" int pu_wgrad_bf16_phase(const pu_wgrad_args* a, void* workspace, size_t ws_bytes, int phase, void* stream) {
    return run_wgrad(a, true, workspace, ws_bytes, phase, stream);
}
