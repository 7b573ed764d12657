// Submission masks on the device: threshold a batch of probability maps y[batch][h][w] and run-length
// encode each mask in column-major order (utils/rle_encode.py), in three launches:
//   rle_bits_kernel   grid (64x64 tiles, batch), one wave per tile: the transposed bitmap
//   rle_count_kernel  grid (batch): pairs of image b -> counts[b]
//   rle_emit_kernel   grid (batch): offsets[b], then the (start, length) pairs of image b in order
// mask[i][j] = (double)y[i][j] > th; the host turns th into f, the smallest fp32 above it, and the
// kernel tests y >= f (NaN is background, +inf foreground).  Pixel (i, j) has the column-major position
// p = j h + i.  The bitmap holds one column after the other, each starting on a word boundary:
// word (j, k), at index j K + k with K = ceil(h / 64), has the rows 64 k .. 64 k + 63 of column j in
// its bits 0 .. 63, zero for the rows past h.  An edge is a position where the column-major mask
// changes, with a zero before the first pixel and after the last.  Edge e (0-based, in order) at
// position p has the value p + 1: an even e is the 1-based start of a run, an odd e gives its length
// as its value minus the value of the edge before it.  No atomics: the order of the pairs is part of
// the result, and every store is a plain store to a cell no other thread writes.
#include "common.h"

#include <math.h>

namespace pu {

typedef unsigned long long u64;

constexpr int RLE_THREADS = 256;
constexpr long long RLE_MAX_N = 1LL << 30;

// Lane l owns column j0 + l.  The wave reads the 64 rows of its tile, one coalesced 256-B read per
// row, all issued before the first use; a row or column past the image is read at the last one (in
// bounds) and dropped after.  Each lane stores its own word: no LDS, no two lanes on one word.
__global__ __launch_bounds__(64) void rle_bits_kernel(const float* __restrict__ y, int h, int w, int K, int col_tiles,
                                                      float f, u64* __restrict__ bits) {
    const int tile_j = blockIdx.x % col_tiles, k = blockIdx.x / col_tiles;
    const int j = tile_j * 64 + (int)threadIdx.x, i0 = k * 64;
    const float* ys = y + (size_t)blockIdx.y * ((size_t)h * w) + (j < w ? j : w - 1);
    float v[64];
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        const int i = i0 + r < h ? i0 + r : h - 1;
        v[r] = ys[(size_t)i * w];
    }
    u64 word = 0;
#pragma unroll
    for (int r = 0; r < 64; ++r) word |= (u64)(v[r] >= f && i0 + r < h) << r;
    if (j < w) bits[((size_t)blockIdx.y * w + j) * K + k] = word;
}

// The edges among the positions of word wi of an image (0 <= wi <= W = w K) as a bit set, and in *p0
// the position of its bit 0.  The bit before a word's first is the top bit of the word before it in
// the same column, or the last pixel of the column before; word W stands for the position after the
// last pixel, which is an edge when that pixel is set.
__device__ __forceinline__ u64 rle_edge_word(const u64* __restrict__ bits, int wi, int W, int K, int h, int* p0) {
    const int j = wi / K, k = wi - j * K;
    const u64 word = wi < W ? bits[wi] : 0;
    u64 carry = 0;
    if (wi > 0) carry = (bits[wi - 1] >> (k ? 63 : (h - 1) & 63)) & 1;
    const int rows = wi == W ? 1 : (h - 64 * k < 64 ? h - 64 * k : 64);
    const u64 valid = rows == 64 ? ~0ull : (1ull << rows) - 1;
    *p0 = j * h + 64 * k;
    return (word ^ ((word << 1) | carry)) & valid;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_count_kernel(const u64* __restrict__ bits, int W, int K, int h,
                                                                int* __restrict__ counts) {
    __shared__ int wave_sum[RLE_THREADS / 64];
    const u64* img = bits + (size_t)blockIdx.x * W;
    int c = 0, p0;
    for (int wi = threadIdx.x; wi <= W; wi += RLE_THREADS) c += __popcll(rle_edge_word(img, wi, W, K, h, &p0));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3])) >> 1;
}

// (edges, value of the last edge) of a stretch of positions; a, the earlier stretch, then b
struct EdgeSum {
    int c, last;
};
__device__ __forceinline__ EdgeSum edge_join(EdgeSum a, EdgeSum b) { return {a.c + b.c, b.c ? b.last : a.last}; }

__global__ __launch_bounds__(RLE_THREADS) void rle_emit_kernel(const u64* __restrict__ bits, const int* __restrict__ counts,
                                                               int batch, int W, int K, int h, long long cap,
                                                               int* __restrict__ offsets, int* __restrict__ runs) {
    __shared__ int wave_sum[RLE_THREADS / 64];
    __shared__ EdgeSum wave_edges[RLE_THREADS / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int off = 0;
    for (int i = threadIdx.x; i < b; i += RLE_THREADS) off += counts[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) off += __shfl_xor(off, d);
    if (lane == 0) wave_sum[wave] = off;
    __syncthreads();
    off = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    if (threadIdx.x == 0) {
        offsets[b] = off;
        if (b == batch - 1) offsets[batch] = off + counts[b];
    }
    const u64* img = bits + (size_t)b * W;
    EdgeSum before = {0, 0};                                  // every word of the steps already walked
    for (int base = 0; base <= W; base += RLE_THREADS) {
        const int wi = base + (int)threadIdx.x;
        int p0 = 0;
        u64 T = wi <= W ? rle_edge_word(img, wi, W, K, h, &p0) : 0;
        const EdgeSum mine = {(int)__popcll(T), T ? p0 + 64 - (int)__clzll(T) : 0};
        EdgeSum incl = mine;                                  // scan over the wave, then over its four totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const EdgeSum o = {__shfl_up(incl.c, d), __shfl_up(incl.last, d)};
            if (lane >= d) incl = edge_join(o, incl);
        }
        EdgeSum excl = {__shfl_up(incl.c, 1), __shfl_up(incl.last, 1)};
        if (lane == 0) excl = {0, 0};
        __syncthreads();                                      // the step before has read wave_edges
        if (lane == 63) wave_edges[wave] = incl;
        __syncthreads();
        EdgeSum lead = before;
        for (int v = 0; v < RLE_THREADS / 64; ++v) {
            if (v == wave) excl = edge_join(lead, excl);
            lead = edge_join(lead, wave_edges[v]);
        }
        before = lead;
        long long slot = 2ll * off + excl.c;                  // even: a start, odd: the length of its run
        int prev = excl.last;
        while (T) {
            const int value = p0 + __builtin_ctzll(T) + 1;
            T &= T - 1;
            if ((slot >> 1) < cap) runs[slot] = (slot & 1) ? value - prev : value;
            prev = value;
            ++slot;
        }
    }
}

// the smallest fp32 whose value exceeds th: y >= f  <=>  (double)y > th for every fp32 y (as metrics.hip)
static float rle_bound_above(double th) {
    float f = (float)th;
    if ((double)f <= th) f = nextafterf(f, INFINITY);
    return f;
}

static bool rle_shape_ok(int batch, int h, int w) {
    if (batch < 1 || batch > 65535 || h < 1 || w < 1) return false;
    const long long n = (long long)h * w;
    return n <= RLE_MAX_N && (long long)batch * ((n + 1) / 2) < (1LL << 31);
}

}  // namespace pu

using namespace pu;

extern "C" size_t pu_rle_encode_workspace_bytes(int batch, int h, int w) {
    if (!rle_shape_ok(batch, h, w)) return 0;
    return (size_t)batch * (size_t)w * (size_t)((h + 63) / 64) * sizeof(u64) + (size_t)batch * sizeof(int);
}

extern "C" int pu_rle_encode(const float* y, int batch, int h, int w, double threshold, int* offsets, int* runs,
                             long long cap, void* workspace, size_t ws_bytes, void* stream) {
    PU_REQUIRE(y, "pu_rle_encode: y is null");
    PU_REQUIRE(offsets, "pu_rle_encode: offsets is null");
    PU_REQUIRE(cap >= 0, "pu_rle_encode: cap %lld is negative", cap);
    PU_REQUIRE(runs || cap == 0, "pu_rle_encode: runs is null with cap %lld", cap);
    PU_REQUIRE(workspace, "pu_rle_encode: workspace is null");
    PU_REQUIRE(batch >= 1 && batch <= 65535, "pu_rle_encode: batch %d (1 .. 65535)", batch);
    PU_REQUIRE(h >= 1 && w >= 1, "pu_rle_encode: image of h %d x w %d", h, w);
    PU_REQUIRE((long long)h * w <= RLE_MAX_N, "pu_rle_encode: h %d x w %d pixels per image (1 .. 2^30)", h, w);
    PU_REQUIRE(rle_shape_ok(batch, h, w), "pu_rle_encode: batch %d of h %d x w %d may have 2^31 pairs or more", batch, h, w);
    PU_REQUIRE(isfinite(threshold), "pu_rle_encode: threshold is not finite");
    PU_REQUIRE(((uintptr_t)workspace & 7) == 0, "pu_rle_encode: workspace must be 8-byte aligned");   // 64-bit words
    const size_t need = pu_rle_encode_workspace_bytes(batch, h, w);
    if (ws_bytes < need)
        return fail(PU_ERR_WORKSPACE, "pu_rle_encode: workspace of %zu bytes at %p, needs %zu", ws_bytes, workspace, need);
    const int K = (h + 63) / 64, col_tiles = (w + 63) / 64, W = w * K;
    u64* bits = static_cast<u64*>(workspace);
    int* counts = reinterpret_cast<int*>(bits + (size_t)batch * W);
    hipLaunchKernelGGL(rle_bits_kernel, dim3(col_tiles * K, batch), dim3(64), 0, as_stream(stream), y, h, w, K, col_tiles,
                       rle_bound_above(threshold), bits);
    hipLaunchKernelGGL(rle_count_kernel, dim3(batch), dim3(RLE_THREADS), 0, as_stream(stream), (const u64*)bits, W, K, h,
                       counts);
    hipLaunchKernelGGL(rle_emit_kernel, dim3(batch), dim3(RLE_THREADS), 0, as_stream(stream), (const u64*)bits,
                       (const int*)counts, batch, W, K, h, cap, offsets, runs);
    return check_launch("pu_rle_encode");
}
