// What the implicit-GEMM convolutions share: igemm.hip and igemm_bf16.hip with everything here,
// winograd.hip and smallconv.hip with the fp32 parameter block and the per-quad epilogue.
//   * ConvParams<T>, the launch parameters over the activation element type T (float | __bf16):
//     IgemmParams adds the fields only the fp32 entry has, IgemmBf16Params adds nothing;
//   * the output epilogue, templated on the parameter type: epi_row / shuf_off / epi_store4 (one
//     4-channel quad: bias, residual, ReLU, mask, channel scale, accumulate, in that order, and for
//     bf16 one rounding at the store) and the batched forms of a grid of 32 x 32 accumulator
//     fragments (epilogue_batched<MASK>, epilogue_batched_shuf).  Which batched form a launch takes
//     is decided where the kernels are: igemm.hip's epilogue<> and igemm_bf16.hip's epi_batch_b_ok /
//     epi_shuf_b_ok state the same conditions in the two shapes their kernels were compiled with
//     (merged into one function, either shape moved register counts of the kernels using it);
//   * the split-K partial-tile store and the split-K finish;
//   * the host side of both entry points: ConvPlan, the argument rules they share
//     (conv_check_args) and the parameter fill (conv_fill_params);
//   * through mfma_common.h: the vector types, the exact 3-term bf16 split of fp32 operands
//     (pairs form), the six-product sequence and the LDS barrier.
#pragma once
#include "mfma_common.h"

namespace pu {

// The fields both paths use.  T: the element type of activations, weights, masks and the residual
// in HBM (the bias and the split-K partials are fp32 on both paths).
template <typename T>
struct ConvParams {
    typedef T elem_t;
    int M, N, K, k_pad;
    int Hi, Wi, Ho, Wo, kh, kw, stride, pad;
    int C, c0, c1;
    const T* src0;
    const T* src1;
    const T* wt;
    const float* bias;
    T* dst0;
    T* dst1;
    const T* mask0;
    const T* mask1;
    int n0, flags;
    int cgroup, taps, gn;   // K order (0 tap-major, 16/32 channel-group-major), kh*kw, n-blocks
    int ksplit, t_per;      // split-K: blocks per tile and K stages per split
    float* part;            // split-K partial tiles [ksplit][M][N]
    const T* resid;         // RESID: NHWC tensor shaped like dst0, added before ReLU / mask
    int shuf_h, shuf_w, shuf_off;   // SHUFFLE2 output grid and crop offset
    FastDiv dWo, dHo, dC, dKw, dCo, dTaps;
    int in_pix;             // batch * Hi * Wi (the lean kernels' buffer extent)
};

// kF32Epi: the epilogue can have a channel scale and can be non-vector.  The shared epilogue reads
// the fp32-only fields under `if constexpr (P::kF32Epi)` alone, so a bf16 kernel tests none of them.
struct IgemmParams : ConvParams<float> {
    static constexpr bool kF32Epi = true;
    const float* cscale;    // per-(image, channel) factors [batch][cs_ld] or null (chan_scale)
    int cs_ld;
    FastDiv dHW;            // Ho * Wo: the image of GEMM row m
    int vec_epi;            // float4 epilogue (channel counts % 4 == 0, 16-byte aligned buffers)
};
struct IgemmBf16Params : ConvParams<__bf16> {
    static constexpr bool kF32Epi = false;
};

// Output position of GEMM row m: the pixel itself, or (SHUFFLE2) the batch row base b*shuf_h and
// the top-left corner (2ho - off, 2wo - off) of its 2x2 output block; b = the image (formed only
// when a channel scale needs it).
struct EpiRow {
    long long pix;
    int oh0, ow0;
    int b;
};

template <typename P>
__device__ __forceinline__ EpiRow epi_row(const P& p, int m) {
    if (!(p.flags & PU_EPI_SHUFFLE2)) {
        if constexpr (P::kF32Epi) return {m, 0, 0, p.cscale ? (int)fdiv(m, p.dHW) : 0};
        else return {m, 0, 0, 0};
    }
    const int t2 = fdiv(m, p.dWo);
    const int wo = m - t2 * p.Wo;
    const int bb = fdiv(t2, p.dHo);
    const int ho = t2 - bb * p.Ho;
    return {(long long)bb * p.shuf_h, 2 * ho - p.shuf_off, 2 * wo - p.shuf_off, bb};
}

// SHUFFLE2 destination element offset of channel n of row r; false if cropped away
template <typename P>
__device__ __forceinline__ bool shuf_off(const P& p, const EpiRow& r, int n, long long* off, int* c) {
    const int co = p.N >> 2;
    const int ij = fdiv(n, p.dCo);
    *c = n - ij * co;
    const int oh = r.oh0 + (ij >> 1), ow = r.ow0 + (ij & 1);
    if ((unsigned)oh >= (unsigned)p.shuf_h || (unsigned)ow >= (unsigned)p.shuf_w) return false;
    *off = ((r.pix + oh) * p.shuf_w + ow) * co + *c;
    return true;
}

// epilogue of channels n..n+3 of row r (n % 4 == 0, N % 4 == 0, n0 % 4 == 0; fp32: vec_epi)
template <typename P>
__device__ __forceinline__ void epi_store4(const P& p, const EpiRow& r, int n, f32x4 v) {
    typedef typename P::elem_t T;
    T* dst;
    const T* msk;
    long long off;
    int nb;   // bias index of the first channel
    const long long pix = r.pix;
    if (p.flags & PU_EPI_SHUFFLE2) {
        if (!shuf_off(p, r, n, &off, &nb)) return;
        dst = p.dst0; msk = p.mask0;
    } else if (n < p.n0) {
        off = pix * p.n0 + n;
        dst = p.dst0; msk = p.mask0; nb = n;
    } else {
        off = pix * (p.N - p.n0) + (n - p.n0);
        dst = p.dst1; msk = p.mask1; nb = n;
    }
    if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + nb);
    if (p.resid) v += ld4(p.resid + off);
    if (p.flags & PU_EPI_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (msk) {
        const f32x4 mv = ld4(msk + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) if (!(mv[e] > 0.f)) v[e] = 0.f;
    }
    if constexpr (P::kF32Epi) {
        if (p.cscale) v *= *reinterpret_cast<const f32x4*>(p.cscale + (long long)r.b * p.cs_ld + nb);
    }
    if (p.flags & PU_EPI_ACCUM) v += ld4(dst + off);
    st4(dst + off, v);
}

// ------------------------------------------------------------------------ batched epilogue forms
// The epilogue's common forms - bias (+ReLU), the forward; masks (+ReLU), the data gradient, into
// one or two NHWC destinations; and the ConvTranspose2d forward's bias under SHUFFLE2 - for an
// [FM][FN] grid of 32 x 32 accumulator fragments, with every operand load issued before the first
// store.  gfx9's vmcnt counts stores as well as loads, and epi_store4 loads each output's operand
// right before its store: the wait for that load then also waited out the round trip of every
// store before it, one store latency per output.  Operands and stores go through buffer
// descriptors with 32-bit offsets (a 32-column fragment lies in one destination: n0 % 32 == 0,
// so the descriptor is wave-uniform per fragment); lanes past M / N load zeros and drop their
// stores (out-of-range offsets), so no per-lane branch splits the batch.  Same operations, order
// and rounding as epi_store4.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t epi_rsrc(const void* base, bool on) {
    const unsigned long long b = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    void* ub = (void*)(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(ub, 0, on ? 0x7fffffff : 0, 0x00020000);
}

// one quad (4 elements of T) per buffer access: 16 bytes of fp32, 8 of bf16
__device__ __forceinline__ f32x4 buf_ld4(const float*, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ u32x2_t buf_ld4(const __bf16*, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
}
__device__ __forceinline__ f32x4 quad_f32(f32x4 q) { return q; }
__device__ __forceinline__ f32x4 quad_f32(u32x2_t q) {
    const bf16x4_t v = __builtin_bit_cast(bf16x4_t, q);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void buf_st4(const float*, f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_st4(const __bf16*, f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    bf16x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, o), r, voff, soff, 0);
}

// the bias of the 4 quads (channels 8q + 4lh ..) of the fragment whose first channel is c; on: the
// fragment lies inside N
__device__ __forceinline__ void epi_bias_frag(const __amdgpu_buffer_rsrc_t r, bool on, int c, f32x4 (&bv)[4]) {
    const unsigned nb = on ? (unsigned)c * 4u : LEAN_OOB;
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, nb, 32 * q, 0));
}

template <bool MASK, int FM, int FN, typename P>
__device__ __forceinline__ void epilogue_batched(const P& p, f32x16 (&acc)[FM][FN], int m0, int nc0, int lr, int lh) {
    typedef typename P::elem_t T;
    constexpr unsigned EB = sizeof(T);     // bytes per element; a quad every 8 channels: 8 * EB apart
    const bool relu = p.flags & PU_EPI_RELU;
    const int n1 = p.N - p.n0;
    unsigned orow[FM][FN];             // byte offset of (row m, fragment column 0), LEAN_OOB past M / N
    bool first[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) first[j] = nc0 + j * 32 < p.n0;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int m = m0 + i * 32 + lr;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int c = nc0 + j * 32 + 4 * lh - (first[j] ? 0 : p.n0);
            orow[i][j] = m < p.M && nc0 + j * 32 < p.N ? (unsigned)(m * (first[j] ? p.n0 : n1) + c) * EB : LEAN_OOB;
        }
    }
    decltype(buf_ld4(p.mask0, epi_rsrc(nullptr, false), 0u, 0)) mv[MASK ? FM : 1][FN][4];   // MASK: each output's mask
    f32x4 bv[FN][4];                                                                        // else its channels' bias
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        if constexpr (MASK) {
            const T* mk = first[j] ? p.mask0 : p.mask1;
            const __amdgpu_buffer_rsrc_t r = epi_rsrc(mk, mk != nullptr);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) mv[i][j][q] = buf_ld4(mk, r, orow[i][j], 8 * EB * q);
        } else {
            epi_bias_frag(epi_rsrc(p.bias, true), nc0 + j * 32 < p.N, nc0 + j * 32 + 4 * lh, bv[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const __amdgpu_buffer_rsrc_t rd = epi_rsrc(first[j] ? p.dst0 : p.dst1, true);
        const bool has_mk = (first[j] ? p.mask0 : p.mask1) != nullptr;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                if constexpr (!MASK) v += bv[j][q];
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if constexpr (MASK) {
                    if (has_mk) {
                        const f32x4 mf = quad_f32(mv[i][j][q]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (!(mf[e] > 0.f)) v[e] = 0.f;
                    }
                }
                buf_st4(p.dst0, v, rd, orow[i][j], 8 * EB * q);
            }
    }
}

// The ConvTranspose2d 2x2 / s2 forward's epilogue (SHUFFLE2 without a crop: column n = ij * co + c
// goes to pixel (2ho + i, 2wo + j) of the 2H x 2W grid, + bias[c]) in the same batched form: every
// bias load before the first store.  co % 32 == 0, so a 32-column fragment lies in one (i, j).
template <int FM, int FN, typename P>
__device__ __forceinline__ void epilogue_batched_shuf(const P& p, f32x16 (&acc)[FM][FN], int m0, int nc0, int lr, int lh) {
    constexpr unsigned EB = sizeof(typename P::elem_t);
    const bool relu = p.flags & PU_EPI_RELU;
    const int co = p.N >> 2;
    unsigned orow[FM][FN];
    int cj[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int nj = nc0 + j * 32;
        const int ij = nj < p.N ? nj / co : 0;
        cj[j] = nj - ij * co + 4 * lh;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int m = m0 + i * 32 + lr;
            unsigned o = LEAN_OOB;
            if (m < p.M && nj < p.N) {
                const int t2 = fdiv(m, p.dWo);
                const int wo = m - t2 * p.Wo;
                const int bb = fdiv(t2, p.dHo);
                const int ho = t2 - bb * p.Ho;
                const int pix = (bb * p.shuf_h + 2 * ho + (ij >> 1)) * p.shuf_w + 2 * wo + (ij & 1);
                o = (unsigned)(pix * co + cj[j]) * EB;
            }
            orow[i][j] = o;
        }
    }
    f32x4 bv[FN][4];
    const __amdgpu_buffer_rsrc_t rb = epi_rsrc(p.bias, true);
#pragma unroll
    for (int j = 0; j < FN; ++j) epi_bias_frag(rb, nc0 + j * 32 < p.N, cj[j], bv[j]);
    const __amdgpu_buffer_rsrc_t rd = epi_rsrc(p.dst0, true);
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                v += bv[j][q];
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                buf_st4(p.dst0, v, rd, orow[i][j], 8 * EB * q);
            }
}

// ------------------------------------------------------------------------------------- split-K
// Raw partial tile of K split KZ -> part[KZ][m][n] (float4 over 4 consecutive n; N % 4 == 0); M0 / NC0:
// the first row / column of the wave's [FM][FN] fragments ACC.  A macro, not a function: as a
// function (const or plain reference to ACC) it cost igemm_dma_kernel<128, 64> one SGPR and
// igemm_bf16_lean_kernel<256, 128> one VGPR against the loop written out.
#define PU_STORE_PARTIAL_TILE(P_, ACC, KZ, M0, NC0, LR, LH)                                      \
    do {                                                                                         \
        float* part_ = (P_).part + (long long)(KZ) * (P_).M * (P_).N;                            \
        _Pragma("unroll") for (int i = 0; i < FM; ++i) {                                         \
            const int m = M0 + i * 32 + LR;                                                      \
            if (m >= (P_).M) continue;                                                           \
            _Pragma("unroll") for (int j = 0; j < FN; ++j)                                       \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                  \
                    const int n = NC0 + j * 32 + 8 * q + 4 * LH;                                 \
                    if (n >= (P_).N) continue;                                                   \
                    f32x4 v;                                                                     \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) v[e] = ACC[i][j][4 * q + e];   \
                    *reinterpret_cast<f32x4*>(part_ + (long long)m * (P_).N + n) = v;            \
                }                                                                                \
        }                                                                                        \
    } while (0)

// split-K second pass, one thread per quad: sum the partial tiles in split order (deterministic)
// + the fused epilogue
template <typename P>
__device__ __forceinline__ void splitk_finish(const P& p) {
    const int nq = p.N >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.M * nq) return;
    const int m = (int)(idx / nq);
    const int n = (int)(idx - (long long)m * nq) * 4;
    const long long mn = (long long)p.M * p.N;
    const float* src = p.part + (long long)m * p.N + n;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
    for (int z = 1; z < p.ksplit; ++z) v += *reinterpret_cast<const f32x4*>(src + z * mn);
    epi_store4(p, epi_row(p, m), n, v);
}

// ---------------------------------------------------------------------------------------- host
// What one call runs: the kernel, its tile, its K split and the scratch the planned split needs.
// Each entry point launches its plan; its two queries report it.
struct ConvPlan {
    int kind, bm, bn;
    int mode;               // pu_conv_igemm_tile's loader mode (fp32 entry only)
    int ksplit, t_per;      // the split this call runs: 1 without the scratch the plan asks for
    size_t ws_bytes;        // fp32 partial tiles of the planned split (0: the plan does not split)
};

// The argument rules that are one rule in both entries (who: the entry's name, bk: its K stage);
// *M = the GEMM rows.  Each entry adds the checks of its own.
inline int conv_check_args(const pu_conv_args* a, const char* who, int bk, long long* M) {
    PU_REQUIRE(a != nullptr, "%s: null args", who);
    PU_REQUIRE(a->batch > 0 && a->in_h > 0 && a->in_w > 0 && a->out_h > 0 && a->out_w > 0,
               "%s: bad grid %dx%dx%d -> %dx%d", who, a->batch, a->in_h, a->in_w, a->out_h, a->out_w);
    PU_REQUIRE(a->kh > 0 && a->kw > 0 && a->stride > 0 && a->pad >= 0, "%s: bad taps", who);
    PU_REQUIRE(a->kh * a->kw <= 32, "%s: at most 32 taps", who);
    PU_REQUIRE(a->src0 && a->c0 > 0, "%s: src0 missing", who);
    PU_REQUIRE(a->c1 == 0 || a->src1, "%s: src1 missing for c1=%d", who, a->c1);
    PU_REQUIRE(a->weight && a->dst0 && a->n > 0, "%s: weight/dst0/n", who);
    const int K = a->kh * a->kw * (a->c0 + a->c1);
    PU_REQUIRE(a->k_pad >= K && a->k_pad % bk == 0, "%s: k_pad %d must be >= %d and a multiple of %d", who, a->k_pad, K, bk);
    const bool shuffle = a->flags & PU_EPI_SHUFFLE2;
    if (a->flags & PU_EPI_RESID) {
        PU_REQUIRE(a->resid && !shuffle && (a->n0 == a->n), "%s: RESID needs resid, a single destination, no SHUFFLE2", who);
    }
    if (shuffle) {
        PU_REQUIRE(a->n % 4 == 0, "%s: SHUFFLE2 needs n %% 4 == 0", who);
        PU_REQUIRE(a->shuf_off >= 0 && a->shuf_h >= 0 && a->shuf_w >= 0, "%s: shuffle geometry", who);
    } else {
        PU_REQUIRE(a->n0 > 0 && a->n0 <= a->n, "%s: n0 %d out of range", who, a->n0);
        PU_REQUIRE(a->n0 == a->n || a->dst1, "%s: dst1 missing", who);
    }
    *M = (long long)a->batch * a->out_h * a->out_w;
    PU_REQUIRE(*M < (1LL << 31) && (long long)a->batch * a->in_h * a->in_w < (1LL << 31), "%s: too many pixels", who);
    return PU_OK;
}

// the fields of ConvParams<T> that follow from the arguments (a has passed conv_check_args); the
// plan's fields (gn, ksplit, t_per, part) are the launcher's
template <typename P>
inline void conv_fill_params(const pu_conv_args* a, long long M, P* pp) {
    typedef typename P::elem_t T;
    P& p = *pp;
    const bool shuffle = a->flags & PU_EPI_SHUFFLE2;
    const int C = a->c0 + a->c1;
    p.M = (int)M; p.N = a->n; p.K = a->kh * a->kw * C; p.k_pad = a->k_pad;
    p.Hi = a->in_h; p.Wi = a->in_w; p.Ho = a->out_h; p.Wo = a->out_w;
    p.kh = a->kh; p.kw = a->kw; p.stride = a->stride; p.pad = a->pad;
    p.C = C; p.c0 = a->c0; p.c1 = a->c1;
    p.src0 = (const T*)a->src0; p.src1 = (const T*)a->src1; p.wt = (const T*)a->weight; p.bias = a->bias;
    p.dst0 = (T*)a->dst0; p.dst1 = (T*)a->dst1; p.mask0 = (const T*)a->mask0; p.mask1 = (const T*)a->mask1;
    p.n0 = shuffle ? a->n : a->n0; p.flags = a->flags;
    p.resid = (a->flags & PU_EPI_RESID) ? (const T*)a->resid : nullptr;
    p.shuf_h = a->shuf_h ? a->shuf_h : 2 * a->out_h;
    p.shuf_w = a->shuf_w ? a->shuf_w : 2 * a->out_w;
    p.shuf_off = a->shuf_off;
    p.dWo = make_fastdiv(a->out_w); p.dHo = make_fastdiv(a->out_h);
    p.dC = make_fastdiv(C); p.dKw = make_fastdiv(a->kw); p.dCo = make_fastdiv(shuffle ? a->n / 4 : 1);
    p.taps = a->kh * a->kw;
    p.dTaps = make_fastdiv(p.taps);
    p.cgroup = a->cgroup;
    p.in_pix = a->batch * a->in_h * a->in_w;
}

// Winograd F(2x2,3x3) path (winograd.hip), dispatched from pu_conv_igemm
bool wino_ok(const pu_conv_args* a, bool vec_epi);
size_t wino_workspace_bytes(const pu_conv_args* a);
void wino_launch(const pu_conv_args* a, IgemmParams p, hipStream_t s);   // p.ksplit: the planned K splits
int wino_item_channels(const pu_conv_args* a);   // output channels per Winograd item (64 or 128)
// 8/16-channel 3x3 convolutions on 16x16x32 bf16 MFMAs (smallconv.hip)
bool smallx6_ok(const pu_conv_args* a, bool vec_epi);
int smallx6_launch(const pu_conv_args* a, const IgemmParams& p, hipStream_t s);

}  // namespace pu
