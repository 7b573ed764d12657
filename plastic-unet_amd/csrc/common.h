// Shared helpers of libplastic_unet.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <type_traits>

#include "plastic_unet.h"

namespace pu {

// ------------------------------------------------------------------------------ error reporting
extern thread_local char g_last_error[512];

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}

// PU_DEBUG builds (build_native.py --variant debug -> lib/libplastic_unet_debug.so) synchronise
// after every launch, so an asynchronous fault is reported by the entry point that caused it
// (the HIP_LAUNCH_BLOCKING / AMD_SERIALIZE_KERNEL discipline, per call instead of per process).
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PU_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
#ifdef PU_DEBUG
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(PU_ERR_LAUNCH, "%s (PU_DEBUG synchronous check): %s", what, hipGetErrorString(e));
#endif
    return PU_OK;
}

#define PU_REQUIRE(cond, ...)                                          \
    do {                                                               \
        if (!(cond)) return ::pu::fail(PU_ERR_INVALID, __VA_ARGS__);   \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ----------------------------------------------------------- integer division by a runtime divisor
// q = umulhi(x, mul) >> shift  for 0 <= x < 2^31, d >= 1 (Granlund-Montgomery round-up method)
struct FastDiv {
    uint32_t d, mul, shift;
};

inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    if (d == 1) {
        f.mul = 0;
        f.shift = 0;
        return f;
    }
    uint32_t l = 0;
    while ((1u << l) < d) ++l;
    // mul = ceil(2^(32+l) / d) - 2^32 ... use the simpler 64-bit form
    uint64_t m = ((uint64_t(1) << (32 + l)) + d - 1) / d;
    f.mul = uint32_t(m);  // m < 2^33; keep the low 32 bits, add x back (see div())
    f.shift = l;
    return f;
}

__device__ __forceinline__ uint32_t fdiv(uint32_t x, const FastDiv& f) {
    // q = (x + umulhi(x, mul_lo)) >> l  where mul = 2^32 + mul_lo ;  x < 2^31 so no overflow.
    // Branch-free: d == 1 has mul_lo = 0, l = 0 (keeps hot loops one basic block).
    uint32_t hi = __umulhi(x, f.mul);
    return (hi + x) >> f.shift;
}

inline int ceil_div(long long a, long long b) { return int((a + b - 1) / b); }

// compute units of the current device (cached per device; 256 when the query fails)
inline int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n >= 8) ? n : 256;
    }
    return cus[dev];
}

// ------------------------------------- tile and split-K choice of the tiled implicit-GEMM kernels
// (igemm.hip's igemm_kernel / igemm_dma_kernel, igemm_bf16.hip's igemm_bf16_kernel)
inline int blocks_for(long long M, int N, int bm, int bn) { return ceil_div(M, bm) * ceil_div(N, bn); }

// the largest tile that still gives >= ~2 blocks per CU (256 CUs)
inline void choose_tile(long long M, int N, int* bm, int* bn) {
    const int target = 480;
    if (N <= 64) {
        if (blocks_for(M, N, 256, 64) >= target) { *bm = 256; *bn = 64; }
        else if (blocks_for(M, N, 128, 64) >= target) { *bm = 128; *bn = 64; }
        else { *bm = 64; *bn = 64; }
    } else {
        if (blocks_for(M, N, 128, 128) >= target) { *bm = 128; *bn = 128; }
        else if (blocks_for(M, N, 128, 64) >= target) { *bm = 128; *bn = 64; }
        else { *bm = 64; *bn = 64; }
    }
}

// When the M x N tile grid fills fewer than the resident block slots of the chip (256 CUs x blocks
// per CU of the tile), split the k_pad / bk K stages so that it does, keeping >= min_stages stages
// per split.
inline void plan_split(int k_pad, int bk, int min_stages, long long M, int N, int bm, int bn, int* ksplit, int* t_per) {
    const int T = k_pad / bk;
    *ksplit = 1;
    *t_per = T;
    const int occ = (bm == 256) ? 2 : (bm == 128 && bn == 128) ? 3 : 4;   // LDS-limited (3-deep ring)
    int ks = (256 * occ) / blocks_for(M, N, bm, bn);
    if (ks > T / min_stages) ks = T / min_stages;
    if (ks < 2) return;
    *t_per = ceil_div(T, ks);
    *ksplit = ceil_div(T, *t_per);
}

// 4-term dot product as an explicit fma chain (v0 w0 first): the 1x1 outconv's per-lane sum, shared
// by outconv_fwd_kernel and the fused head so both produce bit-identical logits
template <typename V>
__device__ __forceinline__ float dot4_fma(const V v, const V w) {
    return fmaf(v[3], w[3], fmaf(v[2], w[2], fmaf(v[1], w[1], v[0] * w[0])));
}

// sum over the L lanes (a power of two up to 16) that share a pixel, by an xor tree inside the
// 16-lane group: the other half of that promise.  outconv_fwd_kernel always runs L = 16 (idle lanes
// carry zeros); the fused head runs L = C / 4 lanes and skips the steps that would add those zeros.
template <int L>
__device__ __forceinline__ float lane_tree16(float t) {
    if (L >= 16) t += __shfl_xor(t, 8, 16);
    if (L >= 8) t += __shfl_xor(t, 4, 16);
    if (L >= 4) t += __shfl_xor(t, 2, 16);
    if (L >= 2) t += __shfl_xor(t, 1, 16);
    return t;
}

// fp64 sum over the block's 256 threads by a halving tree through LDS, valid in thread 0; every
// thread of the block calls it.  The first barrier comes after the write of `s`, so it also
// publishes whatever else the caller stored to LDS before the call.
__device__ __forceinline__ double block_tree256(double s) {
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// XCD-aware block order: the dispatcher deals blocks round-robin over the 8 XCDs (block b runs on
// XCD b % 8).  Map hardware block b to a logical tile so that each XCD gets one CONTIGUOUS range
// of logical tiles (neighbouring tiles share input rows/halos -> reuse in that XCD's L2).
// Bijective for any total (the ragged variant of cdna_hip_programming.md T1).
__device__ __forceinline__ int xcd_remap(int b, int total) {
    const int xcd = b & 7, local = b >> 3;
    const int q = total >> 3, r = total & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}


// compile-time loop: f(integral_constant<int, I>) for I = 0 .. N-1 (unrolled; I usable as a constant)
template <int N, typename F, int I = 0>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, F, I + 1>(static_cast<F&&>(f));
    }
}
// lean implicit-GEMM loaders: an out-of-image tap gets this byte offset, outside every buffer
// descriptor's range, so the range check writes zeros into LDS (probed: tools/probes/oob_lds.hip)
constexpr unsigned LEAN_OOB = 0x80000000u;

// vector and address-space types (those of the MFMA kernels alone: mfma_common.h)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

// 4 consecutive activation elements as fp32: fp32 as they are; bf16 widened, and rounded once (to
// nearest even) at the store
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const __bf16* p) {
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4(__bf16* p, f32x4 v) {
    bf16x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x4_t*>(p) = o;
}

// blocks of a grid-stride launch over `total` items
inline int grid_for(long long total, int block = 256, int cap = 8192) {
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace pu
