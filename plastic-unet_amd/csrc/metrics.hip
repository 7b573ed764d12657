// Validation metrics of a batch of probability maps against their targets, in one pass over y and t:
//   seg_metrics_partial_kernel  grid (G, batch): per block the fp64 BCE sum and the pixel counts
//   seg_metrics_finish_kernel   grid (batch): loss[b] and the int64 count row of sample b
// Per sample b over its n pixels, with T <= 32 thresholds th_k:
//   loss[b]       mean BCE, the bits pu_bce_fwd gives on the sample's slice: G = bce_grid(n) blocks of
//                 256 threads own the elements bce_partial_kernel's blocks own, add them in the same
//                 order into the same fp64 sums, and the finish is bce_final_kernel's (bce_common.h)
//   agree[b]      pixels with (t > 0) == (y > 0.5f)
//   tcount[b]     foreground targets, 0.5 <= t <= 1
//   pcount[b][k]  pixels with (double)y > th_k; icount[b][k]: those that are foreground targets too
// The host turns th_k into f_k, the smallest fp32 above it, so that y >= f_k is the fp64 comparison.
// The counts are integers: any order of summation gives the same bits.  They are taken per wave by
// ballot and population count; no atomics, the block partials are plain stores into the workspace.
// Reads 8 B per pixel once.
#include "bce_common.h"

namespace pu {

constexpr int METRICS_MAX_T = 32;
constexpr int METRICS_COLS = 2 + 2 * METRICS_MAX_T;      // agree, tcount, pcount[32], icount[32]

// by value in the kernel arguments; entries past n_thr are NaN and never count
struct MetricBounds {
    float f[METRICS_MAX_T];
};

// workspace: double loss_partial[batch][G], then uint32 count_partial[batch][G][cols], cols = 2 + 2 T
__global__ __launch_bounds__(256) void seg_metrics_partial_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                                  long long n, int n_thr, const MetricBounds bounds,
                                                                  double* __restrict__ loss_partial,
                                                                  unsigned* __restrict__ count_partial) {
    __shared__ unsigned wave_count[4][METRICS_COLS];
    const long long sample = (long long)blockIdx.y * n;
    const float* ys = y + sample;
    const float* ts = t + sample;
    double s = 0.0;
    unsigned agree = 0, tcount = 0;
    // The 64 threshold counters start from a zero defined in a vector register: as wave-uniform values
    // the compiler would hold them in scalar registers, next to the 32 bounds, and spill.
    unsigned zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    unsigned pc[METRICS_MAX_T], ic[METRICS_MAX_T];
#pragma unroll
    for (int k = 0; k < METRICS_MAX_T; ++k) pc[k] = ic[k] = zero;
    // Every count is taken per wave with a ballot over the lanes still in the loop, so the counters
    // hold wave totals and need no tree.  Lane 0 owns the lowest elements of its wave: it leaves the
    // loop last and its counters are the complete ones.  A block counts at most 256 * ceil(n / (256 G))
    // elements: below 2^32 for every n the entry accepts.
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float yy = ys[i], tt = ts[i];
        s += (double)bce_element(yy, tt);
        const unsigned long long fg = __ballot(tt >= 0.5f && tt <= 1.f);
        agree += __popcll(__ballot((tt > 0.f) == (yy > 0.5f)));
        tcount += __popcll(fg);
        if (n_thr > 0) {
#pragma unroll
            for (int k = 0; k < METRICS_MAX_T; ++k) {
                const unsigned long long p = __ballot(yy >= bounds.f[k]);
                pc[k] += __popcll(p);
                ic[k] += __popcll(p & fg);
            }
        }
    }
    const int cols = 2 + 2 * n_thr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        wave_count[wave][0] = agree;
        wave_count[wave][1] = tcount;
#pragma unroll
        for (int k = 0; k < METRICS_MAX_T; ++k) {
            if (k < n_thr) {
                wave_count[wave][2 + k] = pc[k];
                wave_count[wave][2 + n_thr + k] = ic[k];
            }
        }
    }
    s = block_tree256(s);                                // its barriers also order wave_count
    const long long block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) loss_partial[block] = s;
    if ((int)threadIdx.x < cols)
        count_partial[block * cols + threadIdx.x] = (wave_count[0][threadIdx.x] + wave_count[1][threadIdx.x]) +
                                                    (wave_count[2][threadIdx.x] + wave_count[3][threadIdx.x]);
}

// counts row of sample b: agree, tcount, pcount[0..T), icount[0..T)
__global__ __launch_bounds__(256) void seg_metrics_finish_kernel(const double* __restrict__ loss_partial,
                                                                 const unsigned* __restrict__ count_partial, int np,
                                                                 long long n, int n_thr, float* __restrict__ loss,
                                                                 long long* __restrict__ counts) {
    __shared__ long long wave_count[4][METRICS_COLS];
    const int cols = 2 + 2 * n_thr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned* rows = count_partial + (long long)blockIdx.x * np * cols;
    // wave w adds the rows of blocks w, w + 4, ...; lane l the columns l and l + 64
    for (int c = lane; c < cols; c += 64) {
        long long v = 0;
        for (int g = wave; g < np; g += 4) v += rows[(long long)g * cols + c];
        wave_count[wave][c] = v;
    }
    const float mean = bce_finish(loss_partial + (long long)blockIdx.x * np, np, n);     // barriers inside
    if (threadIdx.x == 0) loss[blockIdx.x] = mean;
    if ((int)threadIdx.x < cols)
        counts[(long long)blockIdx.x * cols + threadIdx.x] = (wave_count[0][threadIdx.x] + wave_count[1][threadIdx.x]) +
                                                             (wave_count[2][threadIdx.x] + wave_count[3][threadIdx.x]);
}

// the largest n whose per-block counts stay below 2^32 at 512 blocks of 256 threads
constexpr long long METRICS_MAX_N = 1LL << 40;

static bool metrics_shape_ok(int batch, long long n, int n_thr) {
    return batch > 0 && batch <= 65535 && n > 0 && n <= METRICS_MAX_N && n_thr >= 0 && n_thr <= METRICS_MAX_T;
}

// the smallest fp32 whose value exceeds th: y >= f  <=>  (double)y > th for every fp32 y
static float bound_above(double th) {
    float f = (float)th;
    if ((double)f <= th) f = nextafterf(f, INFINITY);
    return f;
}

}  // namespace pu

using namespace pu;

extern "C" size_t pu_seg_metrics_workspace_bytes(int batch, long long n, int n_thr) {
    if (!metrics_shape_ok(batch, n, n_thr)) return 0;
    const size_t blocks = (size_t)batch * (size_t)bce_grid(n);
    return blocks * sizeof(double) + blocks * (size_t)(2 + 2 * n_thr) * sizeof(unsigned);
}

extern "C" int pu_seg_metrics(const float* y, const float* t, int batch, long long n, const double* thresholds, int n_thr,
                              float* loss, long long* counts, void* workspace, size_t ws_bytes, void* stream) {
    PU_REQUIRE(y && t, "pu_seg_metrics: y or t is null");
    PU_REQUIRE(loss && counts, "pu_seg_metrics: loss or counts is null");
    PU_REQUIRE(batch > 0 && batch <= 65535, "pu_seg_metrics: batch %d (1 .. 65535)", batch);
    PU_REQUIRE(n > 0 && n <= METRICS_MAX_N, "pu_seg_metrics: n %lld (1 .. 2^40 pixels per sample)", n);
    PU_REQUIRE(n_thr >= 0 && n_thr <= METRICS_MAX_T, "pu_seg_metrics: n_thr %d (0 .. %d)", n_thr, METRICS_MAX_T);
    PU_REQUIRE(n_thr == 0 || thresholds, "pu_seg_metrics: thresholds is null with n_thr %d", n_thr);
    MetricBounds bounds;
    for (int k = 0; k < METRICS_MAX_T; ++k) bounds.f[k] = NAN;
    for (int k = 0; k < n_thr; ++k) {
        PU_REQUIRE(isfinite(thresholds[k]), "pu_seg_metrics: thresholds[%d] is not finite", k);
        PU_REQUIRE(k == 0 || thresholds[k] > thresholds[k - 1], "pu_seg_metrics: thresholds[%d] is not above thresholds[%d]",
                   k, k - 1);
        bounds.f[k] = bound_above(thresholds[k]);
    }
    const size_t need = pu_seg_metrics_workspace_bytes(batch, n, n_thr);
    if (!workspace || ws_bytes < need)
        return fail(PU_ERR_WORKSPACE, "pu_seg_metrics: workspace of %zu bytes at %p, needs %zu", ws_bytes, workspace, need);
    PU_REQUIRE(((uintptr_t)workspace & 7) == 0, "pu_seg_metrics: workspace must be 8-byte aligned");   // fp64 partials
    const int G = bce_grid(n);
    double* loss_partial = static_cast<double*>(workspace);
    unsigned* count_partial = reinterpret_cast<unsigned*>(loss_partial + (size_t)batch * G);
    hipLaunchKernelGGL(seg_metrics_partial_kernel, dim3(G, batch), dim3(256), 0, as_stream(stream), y, t, n, n_thr, bounds,
                       loss_partial, count_partial);
    hipLaunchKernelGGL(seg_metrics_finish_kernel, dim3(batch), dim3(256), 0, as_stream(stream),
                       (const double*)loss_partial, (const unsigned*)count_partial, G, n, n_thr, loss, counts);
    return check_launch("pu_seg_metrics");
}
