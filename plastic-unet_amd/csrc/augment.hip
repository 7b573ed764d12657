// Training augmentation and flip-averaged inference on the device: two pure data movers.
//   augment_kernel    pu_augment: slot b's image planes x[b][cx][h][w] and mask planes t[b][ct][h][w] are
//                     translated by (dy, dx) with reflected borders (the edge pixel is not repeated) and
//                     then mirrored left-right when flip is set, all planes of a slot by the same table
//                     row {flip, dy, dx, 0}:
//                       out[i][j] = in[R(i - dy, h)][R(jj - dx, w)],  jj = flip ? w - 1 - j : j,
//                       R(k, n) = k < 0 ? -k : (k >= n ? 2 (n - 1) - k : k)
//   flip_mean_kernel  pu_flip_mean: out[b][i][j] = 0.5f * (y[b][i][j] + y_mirror[b][i][w - 1 - j])
// Thread mapping: a block is 4 waves; lane l owns column j0 + l of its 64-column run, so every store of
// a wave is one run of up to 256 contiguous bytes of an output row, at any row alignment (w = 101).  A
// source row is read forwards or, mirrored, backwards: the same whole cache lines either way; only the
// up to max_shift reflected columns at an edge fold back on lines the wave reads anyway.  Every lane has
// 8 loads in flight, all issued before its first store; the source column is computed once per lane and
// run, the source row once per wave and row.  A row or column past the image is read at the last one (in
// bounds) and not stored.  No LDS, no atomics: every output word is written by exactly one lane, a bit
// copy of an input word in pu_augment (the words travel as integers: NaN payloads and denormals survive).
//   augment_kernel    tile of 128 columns x 16 rows: wave v takes the rows i0 + v + 4 k, k = 0 .. 3, and of
//                     each two 64-column runs side by side.  With dx != 0 a wave's 256-byte read starts off
//                     the line boundary its store sits on and touches one 128-byte line more, the line the
//                     neighbouring tile reads too.  The hardware deals consecutive blocks to the 8 XCDs in
//                     turn, so neighbours would each pull that line into another L2: blocks are renumbered
//                     (xcd_remap) so that an XCD works on a contiguous range of tiles, and the shifted
//                     transform then costs what the unshifted one does (measured).
//   flip_mean_kernel  tile of 64 columns x 32 rows over the batch h rows, k = 0 .. 7; its reads are aligned
//                     like its stores, mirrored or not.
// Safety: the kernel clamps dy and dx of the table to +-max_shift and uses flip & 1, and the entry
// admits max_shift <= min(h, w) - 1 only.  Then for 0 <= i < n and |d| <= n - 1 the index R(i - d, n)
// lies in [0, n): no table content can make a lane read outside its plane.
#include "common.h"

namespace pu {

constexpr int AUG_COLS = 64, AUG_WAVES = 4, AUG_ROWS_PER_WAVE = 8;
constexpr int AUG_THREADS = AUG_COLS * AUG_WAVES, AUG_TILE_ROWS = AUG_WAVES * AUG_ROWS_PER_WAVE;
constexpr int AUG_RUNS = 2;                                // 64-column runs per lane of augment_kernel
constexpr int AUG_RUN_ROWS = AUG_ROWS_PER_WAVE / AUG_RUNS;    // ... and its rows per wave: 8 loads per lane

__device__ __forceinline__ int aug_clamp(int v, int s) { return v < -s ? -s : (v > s ? s : v); }
__device__ __forceinline__ int aug_reflect(int k, int n) { return k < 0 ? -k : (k >= n ? 2 * (n - 1) - k : k); }

__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ t,
                                                             uint32_t* __restrict__ x_out, uint32_t* __restrict__ t_out,
                                                             int cx, int ct, int h, int w, int col_tiles,
                                                             const int* __restrict__ table, int max_shift) {
    constexpr int CPL = AUG_RUNS, RPW = AUG_RUN_ROWS;
    const int b = blockIdx.z, ch = blockIdx.y;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_j = bx % col_tiles, tile_i = bx / col_tiles;
    const int lane = threadIdx.x & (AUG_COLS - 1), wave = threadIdx.x / AUG_COLS;
    const int flip = table[4 * b] & 1;
    const int dy = aug_clamp(table[4 * b + 1], max_shift), dx = aug_clamp(table[4 * b + 2], max_shift);
    const size_t plane = (size_t)h * w;
    const uint32_t* src;
    uint32_t* dst;
    if (ch < cx) {
        src = x + ((size_t)b * cx + ch) * plane;
        dst = x_out + ((size_t)b * cx + ch) * plane;
    } else {
        src = t + ((size_t)b * ct + (ch - cx)) * plane;
        dst = t_out + ((size_t)b * ct + (ch - cx)) * plane;
    }
    int j[CPL], sj[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        j[c] = (tile_j * CPL + c) * AUG_COLS + lane;
        const int jc = j[c] < w ? j[c] : w - 1;
        sj[c] = aug_reflect((flip ? w - 1 - jc : jc) - dx, w);
    }
    const int i0 = tile_i * AUG_WAVES * RPW + wave;
    uint32_t v[RPW][CPL];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + AUG_WAVES * k;
        const int si = aug_reflect((i < h ? i : h - 1) - dy, h);
#pragma unroll
        for (int c = 0; c < CPL; ++c) v[k][c] = src[(size_t)si * w + sj[c]];
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + AUG_WAVES * k;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
            if (i < h && j[c] < w) dst[(size_t)i * w + j[c]] = v[k][c];
    }
}

// rows = batch h rows of w pixels as one tall plane.  out may be y itself: a lane reads
// its own y[i][j] before it stores there and nobody else touches that word.
__global__ __launch_bounds__(AUG_THREADS) void flip_mean_kernel(const float* y, const float* __restrict__ y_mirror, float* out,
                                                               int rows, int w, int col_tiles) {
    const int tile_j = blockIdx.x % col_tiles, tile_i = blockIdx.x / col_tiles;
    const int lane = threadIdx.x & (AUG_COLS - 1), wave = threadIdx.x / AUG_COLS;
    const int j = tile_j * AUG_COLS + lane;
    const int jc = j < w ? j : w - 1;
    const int i0 = tile_i * AUG_TILE_ROWS + wave;
    float a[AUG_ROWS_PER_WAVE], m[AUG_ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < AUG_ROWS_PER_WAVE; ++k) {
        const int i = i0 + AUG_WAVES * k;
        const size_t row = (size_t)(i < rows ? i : rows - 1) * w;
        a[k] = y[row + jc];
        m[k] = y_mirror[row + (w - 1 - jc)];
    }
#pragma unroll
    for (int k = 0; k < AUG_ROWS_PER_WAVE; ++k) {
        const int i = i0 + AUG_WAVES * k;
        if (i < rows && j < w) out[(size_t)i * w + j] = 0.5f * (a[k] + m[k]);
    }
}

// [p, p + bytes) and [q, q + bytes2) share a byte
static bool aug_overlap(const void* p, size_t bytes, const void* q, size_t bytes2) {
    const uintptr_t a = (uintptr_t)p, c = (uintptr_t)q;
    return p && q && bytes && bytes2 && a < c + bytes2 && c < a + bytes;
}

}  // namespace pu

using namespace pu;

extern "C" int pu_augment(const float* x, const float* t, float* x_out, float* t_out, int batch, int cx, int ct, int h, int w,
                          const int* table, int max_shift, void* stream) {
    PU_REQUIRE(batch >= 1 && batch <= 65535, "pu_augment: batch %d (1 .. 65535)", batch);
    PU_REQUIRE(cx >= 1 && ct >= 0 && (long long)cx + ct <= 65535, "pu_augment: %d image and %d mask planes per slot (1 .. , 0 .. ; 65535 together)", cx, ct);
    PU_REQUIRE(h >= 1 && w >= 1, "pu_augment: plane of h %d x w %d", h, w);
    PU_REQUIRE((long long)h * w <= (1LL << 30), "pu_augment: h %d x w %d pixels per plane (1 .. 2^30)", h, w);
    PU_REQUIRE(max_shift >= 0, "pu_augment: max_shift %d is negative", max_shift);
    PU_REQUIRE(max_shift <= (h < w ? h : w) - 1, "pu_augment: max_shift %d above min(h %d, w %d) - 1: a reflection would leave the plane",
               max_shift, h, w);
    PU_REQUIRE(x, "pu_augment: x is null");
    PU_REQUIRE(x_out, "pu_augment: x_out is null");
    PU_REQUIRE(table, "pu_augment: table is null");
    PU_REQUIRE(ct == 0 || (t && t_out), "pu_augment: t or t_out is null with %d mask planes", ct);
    PU_REQUIRE((((uintptr_t)x | (uintptr_t)t | (uintptr_t)x_out | (uintptr_t)t_out | (uintptr_t)table) & 3) == 0,
               "pu_augment: x, t, x_out, t_out and table must be 4-byte aligned");
    const size_t xb = (size_t)batch * cx * h * w * sizeof(float), tb = (size_t)batch * ct * h * w * sizeof(float);
    PU_REQUIRE(!aug_overlap(x_out, xb, x, xb) && !aug_overlap(x_out, xb, t, tb) && !aug_overlap(t_out, tb, x, xb) &&
                   !aug_overlap(t_out, tb, t, tb),
               "pu_augment: an output aliases an input (the transform is not in place)");
    PU_REQUIRE(!aug_overlap(x_out, xb, t_out, tb), "pu_augment: x_out and t_out overlap");
    PU_REQUIRE(!aug_overlap(x_out, xb, table, (size_t)batch * 16) && !aug_overlap(t_out, tb, table, (size_t)batch * 16),
               "pu_augment: an output aliases the table");
    const int col_tiles = ceil_div(w, AUG_COLS * AUG_RUNS), row_tiles = ceil_div(h, AUG_WAVES * AUG_RUN_ROWS);
    hipLaunchKernelGGL(augment_kernel, dim3(col_tiles * row_tiles, cx + ct, batch), dim3(AUG_THREADS), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(x), reinterpret_cast<const uint32_t*>(t),
                       reinterpret_cast<uint32_t*>(x_out), reinterpret_cast<uint32_t*>(t_out), cx, ct, h, w, col_tiles, table,
                       max_shift);
    return check_launch("pu_augment");
}

extern "C" int pu_flip_mean(const float* y, const float* y_mirror, float* out, int batch, int h, int w, void* stream) {
    PU_REQUIRE(batch >= 1 && h >= 1 && w >= 1, "pu_flip_mean: batch %d of h %d x w %d", batch, h, w);
    PU_REQUIRE((long long)batch * h < (1LL << 31) && (long long)batch * h * w <= (1LL << 40),
               "pu_flip_mean: batch %d of h %d x w %d: 2^31 rows or more", batch, h, w);
    PU_REQUIRE(y, "pu_flip_mean: y is null");
    PU_REQUIRE(y_mirror, "pu_flip_mean: y_mirror is null");
    PU_REQUIRE(out, "pu_flip_mean: out is null");
    PU_REQUIRE((((uintptr_t)y | (uintptr_t)y_mirror | (uintptr_t)out) & 3) == 0, "pu_flip_mean: y, y_mirror and out must be 4-byte aligned");
    const size_t nb = (size_t)batch * h * w * sizeof(float);
    PU_REQUIRE(!aug_overlap(out, nb, y_mirror, nb), "pu_flip_mean: out overlaps y_mirror (only out == y is in place)");
    PU_REQUIRE(out == y || !aug_overlap(out, nb, y, nb), "pu_flip_mean: out overlaps y without being y");
    const int rows = batch * h;
    const int col_tiles = ceil_div(w, AUG_COLS);
    const long long blocks = (long long)col_tiles * ceil_div(rows, AUG_TILE_ROWS);
    PU_REQUIRE(blocks < (1LL << 31), "pu_flip_mean: batch %d of h %d x w %d needs 2^31 blocks or more", batch, h, w);
    hipLaunchKernelGGL(flip_mean_kernel, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, as_stream(stream), y, y_mirror, out, rows, w,
                       col_tiles);
    return check_launch("pu_flip_mean");
}
