// Lovasz loss on probabilities (the Lovasz extension of the Jaccard loss, Berman's lovasz_softmax for
// the one foreground class), per image, mean over the batch:
//   lovasz_image_kernel<CAP>  grid (batch), one workgroup per image: sort, Jaccard gradient, D, image sum
//   lovasz_finish_kernel      one block: loss_per_image and the mean over the images, in image order
//   lovasz_bwd_kernel         elementwise: dy = D * (grad_loss / batch)
// Image b, n pixels: fg_i = 0.5 <= t_i <= 1 (the rule of pu_seg_metrics), e_i = fg_i ? 1.f - y_i : y_i in
// fp32.  The pixels are ranked by e descending, equal e by pixel index ascending: the kernel sorts the
// 64-bit keys  ~bits(e_i) << 32 | i << 1 | fg_i  ascending (bits(e) orders as e does for e >= 0, a -0
// taken as +0; the keys are unique, so the network's result is that order whatever its schedule) with a
// bitonic network over P = the power of two >= max(n, 16), padded with all-ones keys, which no pixel has
// and which end up at the ranks n .. P-1.  The keys live in LDS (CAP of them: 8 KiB, 32 KiB or 128 KiB);
// thread c owns the ranks 16 c .. 16 c + 15: the stages of stride < 16 run in its registers without a
// barrier, the wider ones through LDS, up to four stages per pass and barrier (lovasz_lds_pass).  After
// the sort a block scan over the fg bits (shuffles within a wave, the wave totals through LDS, as
// rle_emit_kernel) gives every thread the foreground count before its ranks; it walks them in order:
// with G = sum fg, cf / cb the foreground / background among ranks 0..k,
//   J_k = 1 - (G - cf) / (G + cb),  J_-1 = 0,  g_k = J_k - J_k-1        (fp64, from the integer counts)
// adds (double)e g to its sum and stores D[b][i] = (float)(fg ? -g : +g) at the pixel the key names.  The
// thread sums meet in one fixed tree.  No atomics, every cell has one writer, no host synchronisation.
// A store's address comes from the index bits of a key, checked against n: never from a value of y.
#include "common.h"

namespace pu {

typedef unsigned long long u64;

constexpr int LOVASZ_MAX_N = 16384;
constexpr int LOVASZ_CHUNK = 16;         // ranks per thread

// Key i lives in slot i ^ ((i >> 5) & 15): a permutation inside every aligned group of 16.  The 32 lanes
// of a half wave that read element e of their chunks (i = 16 lane + e) then hit 32 different 8-byte bank
// pairs instead of two; a run of 32 consecutive i stays a run of 32 different slots.
__device__ __forceinline__ int lovasz_slot(int i) { return i ^ ((i >> 5) & 15); }

__device__ __forceinline__ void lovasz_cswap(u64& a, u64& b, bool ascending) {
    if ((a > b) == ascending) {
        const u64 x = a;
        a = b;
        b = x;
    }
}

// the stages of stride J, J / 2, .. 1 of the merge of size k on the 16 keys at ranks base .. base + 15
template <int J>
__device__ __forceinline__ void lovasz_register_stages(u64 (&v)[LOVASZ_CHUNK], int base, int k) {
#pragma unroll
    for (int j = J; j >= 1; j >>= 1) {
#pragma unroll
        for (int e = 0; e < LOVASZ_CHUNK; ++e)
            if ((e & j) == 0) lovasz_cswap(v[e], v[e | j], ((base | e) & k) == 0);
    }
}

// One pass through LDS over the R stages of stride j, j / 2, .. s = j >> (R - 1) (all >= 16) of the merge
// of size k.  The keys i0 + e s, e < 2^R, meet only each other in these stages: a thread reads 16 / 2^R
// such groups (group q = tid + m chunks: i0 has the bits of q below s in place and the others moved up
// by R), runs the R stages on each in registers and writes them back; every key has one owner per pass.
template <int R>
__device__ __forceinline__ void lovasz_lds_pass(u64* keys, int tid, int chunks, int j, int k) {
    constexpr int E = 1 << R, GROUPS = LOVASZ_CHUNK / E;
    const int s = j >> (R - 1);
    u64 v[LOVASZ_CHUNK];
    int i0[GROUPS];
#pragma unroll
    for (int m = 0; m < GROUPS; ++m) {
        const int q = tid + m * chunks;
        i0[m] = ((q & ~(s - 1)) << R) | (q & (s - 1));
#pragma unroll
        for (int e = 0; e < E; ++e) v[m * E + e] = keys[lovasz_slot(i0[m] | (e * s))];
    }
#pragma unroll
    for (int m = 0; m < GROUPS; ++m) {
        const bool ascending = (i0[m] & k) == 0;
#pragma unroll
        for (int bit = E >> 1; bit >= 1; bit >>= 1) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((e & bit) == 0) lovasz_cswap(v[m * E + e], v[m * E + (e | bit)], ascending);
        }
    }
#pragma unroll
    for (int m = 0; m < GROUPS; ++m) {
#pragma unroll
        for (int e = 0; e < E; ++e) keys[lovasz_slot(i0[m] | (e * s))] = v[m * E + e];
    }
}

// 1 - (G - cf) / (G + cb): the Jaccard loss of the first ranks, cf of them foreground and cb background
__device__ __forceinline__ double lovasz_jaccard(int G, int cf, int cb) {
#pragma clang fp contract(off)
    return 1.0 - (double)(G - cf) / (double)(G + cb);
}

template <int CAP>
__global__ __launch_bounds__(CAP / LOVASZ_CHUNK) void lovasz_image_kernel(const float* __restrict__ y,
                                                                          const float* __restrict__ t, int n, int P,
                                                                          float* __restrict__ dtab,
                                                                          double* __restrict__ image_sum) {
#pragma clang fp contract(off)
    constexpr int T = CAP / LOVASZ_CHUNK, WAVES = T / 64;
    __shared__ u64 keys[CAP];
    __shared__ int wave_fg[WAVES];
    __shared__ double wave_sum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t image = (size_t)blockIdx.x * n;
    for (int i = tid; i < P; i += T) {
        u64 key = ~0ull;
        if (i < n) {
            const float yy = y[image + i], tt = t[image + i];
            const unsigned fg = tt >= 0.5f && tt <= 1.f;
            const float e = fg ? 1.f - yy : yy;
            unsigned ebits = __float_as_uint(e);
            if (ebits == 0x80000000u) ebits = 0;             // e = -0 (a background y of -0) ties with +0, by index
            key = (u64)~ebits << 32 | (u64)((unsigned)i << 1 | fg);
        }
        keys[lovasz_slot(i)] = key;
    }
    __syncthreads();
    const int chunks = P / LOVASZ_CHUNK;                     // threads that own keys
    const bool own = tid < chunks;
    const int base = tid * LOVASZ_CHUNK;
    u64 v[LOVASZ_CHUNK];
    if (own) {
#pragma unroll
        for (int e = 0; e < LOVASZ_CHUNK; ++e) v[e] = keys[lovasz_slot(base + e)];
        lovasz_register_stages<1>(v, base, 2);
        lovasz_register_stages<2>(v, base, 4);
        lovasz_register_stages<4>(v, base, 8);
        lovasz_register_stages<8>(v, base, 16);
    }
    // the merge of size k = 2^(4 + wide): `wide` stages through LDS, up to four per pass (the first pass
    // takes the remainder), then the four of stride 8 .. 1 in the registers of the chunk's owner
    for (int wide = 1; (LOVASZ_CHUNK << wide) <= P; ++wide) {
        const int k = LOVASZ_CHUNK << wide;
        if (own) {
#pragma unroll
            for (int e = 0; e < LOVASZ_CHUNK; ++e) keys[lovasz_slot(base + e)] = v[e];
        }
        __syncthreads();
        int j = k >> 1, r = (wide & 3) ? (wide & 3) : 4;
        for (int left = wide; left > 0; left -= r, j >>= r, r = 4) {
            if (own) {
                if (r == 4) lovasz_lds_pass<4>(keys, tid, chunks, j, k);
                else if (r == 3) lovasz_lds_pass<3>(keys, tid, chunks, j, k);
                else if (r == 2) lovasz_lds_pass<2>(keys, tid, chunks, j, k);
                else lovasz_lds_pass<1>(keys, tid, chunks, j, k);
            }
            __syncthreads();
        }
        if (own) {
#pragma unroll
            for (int e = 0; e < LOVASZ_CHUNK; ++e) v[e] = keys[lovasz_slot(base + e)];
            lovasz_register_stages<8>(v, base, k);
        }
    }
    // v: the keys at the thread's ranks.  Foreground among them, then among the ranks before them.
    int c = 0;
    if (own) {
#pragma unroll
        for (int e = 0; e < LOVASZ_CHUNK; ++e) c += base + e < n ? (int)(v[e] & 1) : 0;
    }
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_fg[wave] = incl;
    __syncthreads();
    int cf = incl - c, G = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) cf += wave_fg[w];
        G += wave_fg[w];
    }
    double s = 0.0;
    if (own && base < n) {
        double before = base == 0 ? 0.0 : lovasz_jaccard(G, cf, base - cf);          // J at rank base - 1
#pragma unroll
        for (int e = 0; e < LOVASZ_CHUNK; ++e) {
            const int k = base + e;
            if (k < n) {
                const int fg = (int)(v[e] & 1);
                cf += fg;
                const double J = lovasz_jaccard(G, cf, k + 1 - cf);
                const double g = J - before;
                before = J;
                s += (double)__uint_as_float(~(unsigned)(v[e] >> 32)) * g;
                const int i = (int)(((unsigned)v[e] >> 1) & (unsigned)(CAP - 1));
                if (dtab && i < n) dtab[image + i] = (float)(fg ? -g : g);
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) wave_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double total = wave_sum[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) total += wave_sum[w];
        image_sum[blockIdx.x] = total;
    }
}

// loss_b = (float)image_sum[b]; loss = (float)((sum of (double)loss_b in image order) / batch): thread i
// adds its run of consecutive images, thread 0 the 256 runs in order
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* __restrict__ image_sum, int batch,
                                                            float* __restrict__ loss, float* __restrict__ loss_per_image) {
#pragma clang fp contract(off)
    __shared__ double run[256];
    const int per = (batch + 255) / 256;
    const int lo = (int)threadIdx.x * per, hi = lo + per < batch ? lo + per : batch;
    double s = 0.0;
    for (int b = lo; b < hi; ++b) {
        const float l = (float)image_sum[b];
        if (loss_per_image) loss_per_image[b] = l;
        s += (double)l;
    }
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = run[0];
        for (int i = 1; i < 256; ++i) total += run[i];
        loss[0] = (float)(total / (double)batch);
    }
}

__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ dtab, const float* __restrict__ g,
                                                         long long total, int batch, float* __restrict__ dy) {
#pragma clang fp contract(off)
    const float scale = (g ? g[0] : 1.f) / (float)batch;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        dy[i] = dtab[i] * scale;
}

static bool lovasz_shape_ok(int batch, int n) { return batch >= 1 && batch <= 65535 && n >= 1 && n <= LOVASZ_MAX_N; }

}  // namespace pu

using namespace pu;

extern "C" size_t pu_lovasz_workspace_bytes(int batch, int n) {
    if (!lovasz_shape_ok(batch, n)) return 0;
    return (size_t)batch * sizeof(double);
}

extern "C" int pu_lovasz_fwd(const float* y, const float* t, int batch, int n, float* loss, float* loss_per_image,
                             float* dtab, void* workspace, size_t ws_bytes, void* stream) {
    PU_REQUIRE(y, "pu_lovasz_fwd: y is null");
    PU_REQUIRE(t, "pu_lovasz_fwd: t is null");
    PU_REQUIRE(loss, "pu_lovasz_fwd: loss is null");
    PU_REQUIRE(workspace, "pu_lovasz_fwd: workspace is null");
    PU_REQUIRE(batch >= 1 && batch <= 65535, "pu_lovasz_fwd: batch %d (1 .. 65535)", batch);
    PU_REQUIRE(n >= 1, "pu_lovasz_fwd: n %d pixels per image", n);
    if (n > LOVASZ_MAX_N)
        return fail(PU_ERR_UNSUPPORTED, "pu_lovasz_fwd: n %d pixels per image, more than the %d one workgroup sorts in LDS",
                    n, LOVASZ_MAX_N);
    PU_REQUIRE((((uintptr_t)y | (uintptr_t)t | (uintptr_t)loss | (uintptr_t)loss_per_image | (uintptr_t)dtab) & 3) == 0,
               "pu_lovasz_fwd: y, t, loss, loss_per_image and dtab must be 4-byte aligned");
    PU_REQUIRE(((uintptr_t)workspace & 7) == 0, "pu_lovasz_fwd: workspace must be 8-byte aligned");   // fp64 image sums
    const size_t need = pu_lovasz_workspace_bytes(batch, n);
    if (ws_bytes < need)
        return fail(PU_ERR_WORKSPACE, "pu_lovasz_fwd: workspace of %zu bytes at %p, needs %zu", ws_bytes, workspace, need);
    int P = LOVASZ_CHUNK;
    while (P < n) P <<= 1;
    double* image_sum = static_cast<double*>(workspace);
    if (P <= 1024)
        hipLaunchKernelGGL(lovasz_image_kernel<1024>, dim3(batch), dim3(1024 / LOVASZ_CHUNK), 0, as_stream(stream), y, t, n, P,
                           dtab, image_sum);
    else if (P <= 4096)
        hipLaunchKernelGGL(lovasz_image_kernel<4096>, dim3(batch), dim3(4096 / LOVASZ_CHUNK), 0, as_stream(stream), y, t, n, P,
                           dtab, image_sum);
    else
        hipLaunchKernelGGL(lovasz_image_kernel<16384>, dim3(batch), dim3(16384 / LOVASZ_CHUNK), 0, as_stream(stream), y, t, n,
                           P, dtab, image_sum);
    hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const double*)image_sum, batch, loss,
                       loss_per_image);
    return check_launch("pu_lovasz_fwd");
}

extern "C" int pu_lovasz_bwd(const float* dtab, const float* grad_loss, int batch, int n, float* dy, void* stream) {
    PU_REQUIRE(dtab, "pu_lovasz_bwd: dtab is null");
    PU_REQUIRE(dy, "pu_lovasz_bwd: dy is null");
    PU_REQUIRE(batch >= 1 && batch <= 65535, "pu_lovasz_bwd: batch %d (1 .. 65535)", batch);
    PU_REQUIRE(n >= 1, "pu_lovasz_bwd: n %d pixels per image", n);
    if (n > LOVASZ_MAX_N)
        return fail(PU_ERR_UNSUPPORTED, "pu_lovasz_bwd: n %d pixels per image, more than the %d of pu_lovasz_fwd", n,
                    LOVASZ_MAX_N);
    PU_REQUIRE((((uintptr_t)dtab | (uintptr_t)grad_loss | (uintptr_t)dy) & 3) == 0,
               "pu_lovasz_bwd: dtab, grad_loss and dy must be 4-byte aligned");
    const long long total = (long long)batch * n;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(lovasz_bwd_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), dtab, grad_loss, total, batch,
                       dy);
    return check_launch("pu_lovasz_bwd");
}
