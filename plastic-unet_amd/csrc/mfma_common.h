// What the MFMA kernels share below the level of a tile: the convolutions through conv_common.h
// (igemm.hip, igemm_bf16.hip, winograd.hip, smallconv.hip) and the weight gradients (wgrad.hip).
//   * the vector types of MFMA operands and packed words, one name each;
//   * the wave-uniform buffer descriptor (uniform_rsrc) and the lean loaders' lean_load;
//   * the exact 3-term bf16 split of fp32 operands, pair form (split3_pair / split3_pairs);
//   * the six products of two split operands in their one order (mma6);
//   * the transposed LDS fragment read (tr_frag) and the LDS barrier (lds_barrier).
#pragma once
#include "common.h"

namespace pu {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef short i16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) i16x4_t lds_i16x4_t;

// a buffer descriptor over [base, base + bytes) from wave-uniform inputs, made provably uniform
// (no waterfall loops around the accesses); bytes == 0 drops every lane (loads give zeros)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, unsigned bytes) {
    const unsigned long long b = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    void* ub = (void*)(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(ub, 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// buffer_load_dwordx4 ... lds of 16 B per lane (zeros land in LDS for dropped lanes).  Kept out of
// the kernel template so the host pass never sees the descriptor type.
__device__ __forceinline__ void lean_load(const void* base, unsigned bytes, void* lds_dst, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(uniform_rsrc(base, bytes), (lds_void_t*)lds_dst, 16, voff,
                                             __builtin_amdgcn_readfirstlane(soff), 0, 0);
}

// x = hi + mid + lo exactly (round-to-nearest at each step), both lanes of a pair at once:
// v_cvt_pk_bf16_f32 rounds two values, the residuals are v_pk_add_f32 (4.5 VALU / element).
// Each result is a packed word: the bf16 of x[0] in the low half, of x[1] in the high half.
__device__ __forceinline__ unsigned pk_bf16(f32x2 v) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void split3_pair(const f32x2 x, unsigned& h, unsigned& m, unsigned& l) {
#pragma clang fp contract(off)
    const unsigned a = pk_bf16(x);
    const f32x2 r = x - f32x2{__builtin_bit_cast(float, a << 16), __builtin_bit_cast(float, a & 0xffff0000u)};
    const unsigned b = pk_bf16(r);
    h = a;
    m = b;
    l = pk_bf16(r - f32x2{__builtin_bit_cast(float, b << 16), __builtin_bit_cast(float, b & 0xffff0000u)});
}

// 8 elements as 4 pairs -> one MFMA operand per plane
__device__ __forceinline__ void split3_pairs(const f32x4 lo4, const f32x4 hi4, bf16x8_t& h, bf16x8_t& m, bf16x8_t& l) {
    u32x4_t hv, mv, lv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned a, b, c;
        split3_pair(q < 2 ? f32x2{lo4[2 * q], lo4[2 * q + 1]} : f32x2{hi4[2 * q - 4], hi4[2 * q - 3]}, a, b, c);
        hv[q] = a;
        mv[q] = b;
        lv[q] = c;
    }
    h = __builtin_bit_cast(bf16x8_t, hv);
    m = __builtin_bit_cast(bf16x8_t, mv);
    l = __builtin_bit_cast(bf16x8_t, lv);
}

// c += q * p for q = qh + qm + ql, p = ph + pm + pl as six bf16 MFMAs with fp32 accumulation; the
// three smallest products (qm pl, ql pm, ql pl) are dropped.  Small terms first:
// qm pm, ql ph, qh pl, qm ph, qh pm, qh ph - the large product is added last, to a sum that
// already holds the corrections.  The order is part of the numerics: every 6-product kernel
// accumulates in it, and kernels documented as bit-identical to one another rely on it.
__device__ __forceinline__ f32x16 mma6(const bf16x8_t qh, const bf16x8_t qm, const bf16x8_t ql, const bf16x8_t ph,
                                       const bf16x8_t pm, const bf16x8_t pl, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qm, pm, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ql, ph, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qh, pl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qm, ph, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qh, pm, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qh, ph, c, 0, 0, 0);
    return c;
}

// One MFMA operand (8 k-values of the lane's column) from a row-major bf16 LDS image: two
// ds_read_b64_tr_b16, of the fragment's rows +0 and +4, at byte offsets o0 and o4 of base.  On
// 128-byte rows the two rows share their swizzle (o4 = o0 + 4 * 128); 256-byte rows pass a pair.
__device__ __forceinline__ bf16x8_t tr_frag(const char* base, int o0, int o4) {
    const i16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t*)(base + o0));
    const i16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t*)(base + o4));
    const i16x8_t av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    return __builtin_bit_cast(bf16x8_t, av);
}

// This wave's LDS accesses are done, then every wave's.  s_barrier is no compiler fence: the empty
// asm keeps the LDS reads that follow behind it.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace pu
