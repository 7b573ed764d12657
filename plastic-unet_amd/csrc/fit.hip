// Fitting data of one size to a net of another, on the device (pu_fit): planes in [h][w] gathered into planes
// out [H][W].
//   fit_move_kernel    PU_FIT_PAD:   out[i][j] = in[R(i - top, h)][R(j - left, w)],
//                                    R(k, n) = k < 0 ? -k : (k >= n ? 2 (n - 1) - k : k)   (augment.hip's)
//                      PU_FIT_CROP:  out[i][j] = in[top + i][left + j]
//                      a bit copy either way: the words travel as integers, NaN payloads and denormals survive.
//   fit_resize_kernel  PU_FIT_RESIZE: bilinear, sample points at the pixel centres, zeros outside the plane.  The
//                      source coordinate of output row r is the rational ((2 r + 1) h - H) / 2H, taken apart in
//                      integers (fit_coord): y0 = floor, fy = the remainder over 2H rounded to fp32 once, gy =
//                      1.0f - fy; columns likewise.  The three lerps, in this order (plastic_unet.h):
//                        top = fmaf(b, fx, a * gx);  bot = fmaf(d, fx, c * gx);  out = fmaf(bot, fy, top * gy)
//                      An fp32 (r + 0.5) * h / H would put y0 one row off where the quotient is a whole number.
//                      Index arithmetic in 32 bits where (2 max(H, W) + 1) max(h, w) < 2^31, in 64 bits above.
// Thread mapping, as augment_kernel: a block is 4 waves; lane l owns column j0 + l of a 64-column run, so every
// store of a wave is one run of up to 256 contiguous bytes of an output row at any row alignment (W = 101 or 128
// alike).  A tile is 128 columns x 16 rows: wave v takes the rows i0 + v + 4 k, k = 0 .. 3, and of each two runs
// side by side.  The source columns (and weights) are computed once per lane and run, the source row (and
// weights) once per wave and row; all of a lane's loads - 8 words, 32 in the resize - are issued before its
// first store.  An output row or column past the plane is computed at the last one (in bounds) and not stored.
// No LDS, no atomics; every output word is written by exactly one lane; plain vector loads and stores.  Blocks
// are renumbered (xcd_remap) so that an XCD works on a contiguous range of tiles: with left != 0 a wave's read
// starts off the line its store sits on, and the neighbouring tile reads that line too.
// Safety: a lane's output position is clamped to 0 <= i < H, 0 <= j < W before it is mapped.
//   PAD     the entry admits 0 <= top <= h - 1 and H - h - top <= h - 1 only, so -(h - 1) <= i - top <= 2 (h - 1)
//           and R(i - top, h) lies in [0, h); columns likewise.
//   CROP    the entry admits 0 <= top <= h - H only, so top + i <= h - 1; columns likewise.
//   RESIZE  n = (2 i + 1) h - H lies in [h - H, 2 H h - h - H], so y0 = floor(n / 2H) lies in [-1, h - 1]; y0 and
//           y0 + 1 are clamped to [0, h - 1] for the load and the loaded value is replaced by 0 where the
//           unclamped index was outside: no value is ever read out of bounds.
// So no argument that passes the entry can make a lane read outside its plane; a block whose plane number is
// not below `planes` (the last slice of the grid's z axis) returns before any access.
#include "common.h"

namespace pu {

constexpr int FIT_COLS = 64, FIT_WAVES = 4, FIT_RUNS = 2, FIT_RUN_ROWS = 4;
constexpr int FIT_THREADS = FIT_COLS * FIT_WAVES;
constexpr int FIT_TILE_COLS = FIT_COLS * FIT_RUNS, FIT_TILE_ROWS = FIT_WAVES * FIT_RUN_ROWS;
constexpr int FIT_GRID_Y = 32768;       // planes along y; the rest along z

__device__ __forceinline__ int fit_reflect(int k, int n) { return k < 0 ? -k : (k >= n ? 2 * (n - 1) - k : k); }

// the plane of this block, or -1 past the last one
__device__ __forceinline__ long long fit_plane(long long planes) {
    const long long p = (long long)blockIdx.z * gridDim.y + blockIdx.y;
    return p < planes ? p : -1;
}

__global__ __launch_bounds__(FIT_THREADS) void fit_move_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                              long long planes, int h, int w, int H, int W, int pad, int top,
                                                              int left, int col_tiles) {
    constexpr int CPL = FIT_RUNS, RPW = FIT_RUN_ROWS;
    const long long p = fit_plane(planes);
    if (p < 0) return;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_j = bx % col_tiles, tile_i = bx / col_tiles;
    const int lane = threadIdx.x & (FIT_COLS - 1), wave = threadIdx.x / FIT_COLS;
    const uint32_t* src = in + (size_t)p * h * w;
    uint32_t* dst = out + (size_t)p * H * W;
    int j[CPL], sj[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        j[c] = (tile_j * CPL + c) * FIT_COLS + lane;
        const int jc = j[c] < W ? j[c] : W - 1;
        sj[c] = pad ? fit_reflect(jc - left, w) : jc + left;
    }
    const int i0 = tile_i * FIT_TILE_ROWS + wave;
    uint32_t v[RPW][CPL];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + FIT_WAVES * k;
        const int ic = i < H ? i : H - 1;
        const int si = pad ? fit_reflect(ic - top, h) : ic + top;
#pragma unroll
        for (int c = 0; c < CPL; ++c) v[k][c] = src[(size_t)si * w + sj[c]];
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + FIT_WAVES * k;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
            if (i < H && j[c] < W) dst[(size_t)i * W + j[c]] = v[k][c];
    }
}

// Output index r of N from n source samples: i0 = floor(((2 r + 1) n - N) / 2N) in [-1, n - 1], and f = the
// remainder over 2N, rounded to fp32 once.  I: int where (2 N + 1) n < 2^31, long long above.  The numerator is
// above -2N, so a negative one has the floor -1; the remainder and 2N are exact in fp32 up to 2^24 (one
// correctly rounded division), above that the fp64 quotient is rounded to fp32.
template <typename I>
__device__ __forceinline__ void fit_coord(int r, int n, int N, int* i0, float* f) {
    typedef typename std::make_unsigned<I>::type U;
    const I num = (I)(2 * (I)r + 1) * (I)n - (I)N;
    const U den = 2 * (U)N;
    const I q = num < 0 ? (I)-1 : (I)((U)num / den);
    const U rem = (U)(num - q * (I)den);
    *i0 = (int)q;
    *f = den <= (U)(1 << 24) ? (float)rem / (float)den : (float)((double)rem / (double)den);
}

template <typename I>
__global__ __launch_bounds__(FIT_THREADS) void fit_resize_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                long long planes, int h, int w, int H, int W, int col_tiles) {
    constexpr int CPL = FIT_RUNS, RPW = FIT_RUN_ROWS;
    const long long p = fit_plane(planes);
    if (p < 0) return;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_j = bx % col_tiles, tile_i = bx / col_tiles;
    const int lane = threadIdx.x & (FIT_COLS - 1), wave = threadIdx.x / FIT_COLS;
    const float* src = in + (size_t)p * h * w;
    float* dst = out + (size_t)p * H * W;
    int j[CPL], x0[CPL], x1[CPL];
    bool in0[CPL], in1[CPL];
    float fx[CPL], gx[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        j[c] = (tile_j * CPL + c) * FIT_COLS + lane;
        int q;
        fit_coord<I>(j[c] < W ? j[c] : W - 1, w, W, &q, &fx[c]);
        gx[c] = 1.0f - fx[c];
        in0[c] = q >= 0;
        in1[c] = q + 1 <= w - 1;
        x0[c] = in0[c] ? q : 0;
        x1[c] = in1[c] ? q + 1 : w - 1;
    }
    const int i0 = tile_i * FIT_TILE_ROWS + wave;
    float a[RPW][CPL], b[RPW][CPL], cc[RPW][CPL], d[RPW][CPL], fy[RPW];
    bool up[RPW], dn[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + FIT_WAVES * k;
        int q;
        fit_coord<I>(i < H ? i : H - 1, h, H, &q, &fy[k]);
        up[k] = q >= 0;
        dn[k] = q + 1 <= h - 1;
        const size_t r0 = (size_t)(up[k] ? q : 0) * w, r1 = (size_t)(dn[k] ? q + 1 : h - 1) * w;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            a[k][c] = src[r0 + x0[c]];
            b[k][c] = src[r0 + x1[c]];
            cc[k][c] = src[r1 + x0[c]];
            d[k][c] = src[r1 + x1[c]];
        }
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = i0 + FIT_WAVES * k;
        const float gy = 1.0f - fy[k];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const float va = up[k] && in0[c] ? a[k][c] : 0.0f, vb = up[k] && in1[c] ? b[k][c] : 0.0f;
            const float vc = dn[k] && in0[c] ? cc[k][c] : 0.0f, vd = dn[k] && in1[c] ? d[k][c] : 0.0f;
            const float t = fmaf(vb, fx[c], va * gx[c]);
            const float u = fmaf(vd, fx[c], vc * gx[c]);
            if (i < H && j[c] < W) dst[(size_t)i * W + j[c]] = fmaf(u, fy[k], t * gy);
        }
    }
}

}  // namespace pu

using namespace pu;

extern "C" int pu_fit(const float* in, float* out, long long planes, int h, int w, int H, int W, int mode, int top, int left,
                      void* stream) {
    PU_REQUIRE(mode == PU_FIT_PAD || mode == PU_FIT_CROP || mode == PU_FIT_RESIZE, "pu_fit: mode %d (PU_FIT_PAD 0, PU_FIT_CROP 1, PU_FIT_RESIZE 2)", mode);
    PU_REQUIRE(planes >= 1 && planes <= (long long)FIT_GRID_Y * 65535, "pu_fit: %lld planes (1 .. %lld)", planes, (long long)FIT_GRID_Y * 65535);
    PU_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, "pu_fit: planes of h %d x w %d to H %d x W %d", h, w, H, W);
    PU_REQUIRE((long long)h * w <= (1LL << 30) && (long long)H * W <= (1LL << 30),
               "pu_fit: h %d x w %d or H %d x W %d pixels per plane (1 .. 2^30)", h, w, H, W);
    if (mode == PU_FIT_PAD) {
        PU_REQUIRE(H >= h && W >= w, "pu_fit: pad of h %d x w %d to a smaller H %d x W %d", h, w, H, W);
        PU_REQUIRE(top >= 0 && top <= h - 1 && H - h - top >= 0 && H - h - top <= h - 1,
                   "pu_fit: pad rows: top %d and bottom %d outside 0 .. h - 1 = %d: a reflection would leave the plane", top,
                   H - h - top, h - 1);
        PU_REQUIRE(left >= 0 && left <= w - 1 && W - w - left >= 0 && W - w - left <= w - 1,
                   "pu_fit: pad columns: left %d and right %d outside 0 .. w - 1 = %d: a reflection would leave the plane", left,
                   W - w - left, w - 1);
    } else if (mode == PU_FIT_CROP) {
        PU_REQUIRE(H <= h && W <= w, "pu_fit: crop of h %d x w %d to a larger H %d x W %d", h, w, H, W);
        PU_REQUIRE(top >= 0 && top <= h - H && left >= 0 && left <= w - W,
                   "pu_fit: crop window at top %d, left %d of H %d x W %d leaves the plane h %d x w %d", top, left, H, W, h, w);
    } else {
        PU_REQUIRE(top == 0 && left == 0, "pu_fit: resize takes top = left = 0 (got %d, %d)", top, left);
    }
    PU_REQUIRE(in, "pu_fit: in is null");
    PU_REQUIRE(out, "pu_fit: out is null");
    PU_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "pu_fit: in and out must be 4-byte aligned");
    // planes <= 2^31 and a plane <= 2^32 bytes: the sizes fit 64 bits
    const uint64_t in_bytes = (uint64_t)planes * h * w * sizeof(float), out_bytes = (uint64_t)planes * H * W * sizeof(float);
    const uintptr_t a = (uintptr_t)in, c = (uintptr_t)out;
    PU_REQUIRE(!(a < c + out_bytes && c < a + in_bytes), "pu_fit: out overlaps in (the map is not in place)");
    const int col_tiles = ceil_div(W, FIT_TILE_COLS), row_tiles = ceil_div(H, FIT_TILE_ROWS);
    const long long tiles = (long long)col_tiles * row_tiles;
    PU_REQUIRE(tiles < (1LL << 24), "pu_fit: H %d x W %d needs 2^24 blocks or more per plane (tiles of %d x %d)", H, W,
               FIT_TILE_ROWS, FIT_TILE_COLS);
    const unsigned gy = planes < FIT_GRID_Y ? (unsigned)planes : FIT_GRID_Y, gz = (unsigned)((planes + gy - 1) / gy);
    const dim3 grid((unsigned)tiles, gy, gz), block(FIT_THREADS);
    if (mode != PU_FIT_RESIZE) {
        hipLaunchKernelGGL(fit_move_kernel, grid, block, 0, as_stream(stream), reinterpret_cast<const uint32_t*>(in),
                           reinterpret_cast<uint32_t*>(out), planes, h, w, H, W, mode == PU_FIT_PAD ? 1 : 0, top, left, col_tiles);
    } else {
        const long long big = (2LL * (H > W ? H : W) + 1) * (h > w ? h : w);
        if (big < (1LL << 31))
            hipLaunchKernelGGL(fit_resize_kernel<int>, grid, block, 0, as_stream(stream), in, out, planes, h, w, H, W, col_tiles);
        else
            hipLaunchKernelGGL(fit_resize_kernel<long long>, grid, block, 0, as_stream(stream), in, out, planes, h, w, H, W,
                               col_tiles);
    }
    return check_launch("pu_fit");
}
