// The plastic head, its trace update, its backward, and BCELoss: the entry points, their launch
// rules and workspace layouts.  The kernels are in head_fwd.h and head_bwd.h, what they share in
// head_common.h; all of them are compiled here, into this file's object.
//
// Reference (yaricom/Plastic-UNet) src/unet/unet_p.py:69-88 (== unet_p_res.py:115-134):
//   activ    = activin.mm(w + alpha*hebb)           -> head_fwd_kernel (Weff built in the loader), or
//   activout = sigmoid(activ)                          head_fused_fwd_kernel / head_pipe_fwd_kernel
//                                                      with the 1x1 outconv in front
//   hebb'    = Hebb (:82) or Oja (:84) from ROW 0   -> fused into those, or trace_kernel(_v4)
// and nn.BCELoss (src/train.py:70,101-105) + the autograd backward of all of it (train.py:110).
// Batched over per-slot traces: slot b uses X_b, H_b; w/alpha/eta are shared.
//
// Element-wise formulas keep the reference's operation order with FP contraction off, so the
// trace update is bit-identical to the ATen CPU ops for the same inputs.
#include "bce_common.h"   // the BCE element, grid and finish, shared with metrics.hip
#include "head_bwd.h"
#include "head_fwd.h"

namespace pu {

// --------------------------------------------------------------------------------------------- BCE
__global__ void bce_partial_kernel(const float* __restrict__ y, const float* __restrict__ t, long long n,
                                   double* __restrict__ partial) {
    double s = 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        s += (double)bce_element(y[i], t[i]);
    s = block_tree256(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void bce_final_kernel(const double* __restrict__ partial, int np, long long n, float* __restrict__ loss) {
    const float mean = bce_finish(partial, np, n);
    if (threadIdx.x == 0) loss[0] = mean;
}

__global__ void bce_bwd_kernel(const float* __restrict__ y, const float* __restrict__ t, long long n,
                               const float* __restrict__ g, float* __restrict__ dy) {
#pragma clang fp contract(off)
    const float gg = g ? g[0] : 1.f;
    const float inv_n = (float)n;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float yy = y[i], tt = t[i];
        const float d = gg * (yy - tt) / fmaxf((1.f - yy) * yy, 1e-12f);
        dy[i] = d / inv_n;
    }
}

// ------------------------------------------------------------------------------------ launch rules
// the reference's own message (unet_p.py), whichever entry point meets the rule
static int check_rule(int rule) {
    PU_REQUIRE(rule == PU_RULE_HEBB || rule == PU_RULE_OJA, "Must select one learning rule ('hebb' or 'oja')");
    return PU_OK;
}

// 64-tiles when they give >= 2 blocks per CU, else 32-tiles (bs 32 x 128^2: 512 blocks)
static bool head_small_tiles(int B, int N) {
    const long long t64 = (long long)ceil_div(N, 64) * ceil_div(N, 64) * B;
    return t64 < 512;
}

// f(integral_constant<int, T>) with the tile T of the VALU GEMMs for B slots of N x N
template <typename F>
static void with_head_tile(int B, int N, F&& f) {
    if (head_small_tiles(B, N)) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

template <int T>
static void launch_head_fwd(const pu_plastic_args* a, float* hn, hipStream_t s) {
    dim3 grid(ceil_div(a->nbf, T), ceil_div(a->nbf, T), a->batch);
    hipLaunchKernelGGL(head_fwd_kernel<T>, grid, dim3(256), 0, s, a->x, a->hebb, a->w, a->alpha, a->y, hn, a->eta,
                       a->nbf, a->rule);
}

// dx (when asked for) and the per-slot (T_b, T_b * H_b) into ws (when given); EX: with the trace
// backward's row-0 extras dx0 / dy0
template <int T, bool EX>
static void launch_head_bwd(const pu_plastic_bwd_args* a, float* ws, const float* dx0, const float* dy0, hipStream_t s) {
    const int N = a->nbf, B = a->batch;
    dim3 grid(ceil_div(N, T), ceil_div(N, T), B);
    if (a->dx)
        hipLaunchKernelGGL((head_dx_kernel<T, EX>), grid, dim3(256), 0, s, a->y, a->dy, a->hebb, a->w, a->alpha, a->dx, N,
                           dy0, dx0);
    if (ws) hipLaunchKernelGGL((head_dw_kernel<T, EX>), grid, dim3(256), 0, s, a->x, a->y, a->dy, a->hebb, ws, N, dy0);
}

// the slot sum of what head_dw_kernel left in ws
static void launch_dw_reduce(const float* ws, int B, int N, float* dw, float* dalpha, hipStream_t s) {
    hipLaunchKernelGGL(head_dw_reduce_kernel, dim3(ceil_div((long long)N * N, 256)), dim3(256), 0, s, ws, B, N, dw, dalpha);
}

// ---- the instantiation of head_fused_fwd_kernel for a call: feature type, L lanes per pixel, and
// (column tiles per wave, rows per block).  One column tile per wave means N <= 128, and 32-row
// blocks need N >= 256 (16 tiles or more, two per wave): <.., 1, 32> cannot be launched and is not
// instantiated.
struct FusedHeadLaunch {
    dim3 grid;
    size_t lds;
    FastDiv dN;
    int kc;
    hipStream_t s;
};

template <typename T, int L, int TPW, int R>
static void launch_fused_head(const pu_plastic_head_args* a, const FusedHeadLaunch& p) {
    hipLaunchKernelGGL((head_fused_fwd_kernel<T, L, TPW, R>), p.grid, dim3(FH_NT), p.lds, p.s, (const T*)a->feat, a->out_w,
                       a->out_b, a->channels, a->hebb, a->w, a->alpha, a->eta, a->x, a->y, a->hebb_out, a->nbf, p.dN, p.kc,
                       a->rule);
}

template <typename T, int L>
static void fused_head_by_tiles(const pu_plastic_head_args* a, const FusedHeadLaunch& p, int tpw, int R) {
    if (tpw <= 1) launch_fused_head<T, L, 1, FH_R>(a, p);
    else if (tpw <= 2) R == 32 ? launch_fused_head<T, L, 2, 32>(a, p) : launch_fused_head<T, L, 2, FH_R>(a, p);
    else R == 32 ? launch_fused_head<T, L, 4, 32>(a, p) : launch_fused_head<T, L, 4, FH_R>(a, p);
}

template <typename T>
static void fused_head_by_lanes(const pu_plastic_head_args* a, const FusedHeadLaunch& p, int L, int tpw, int R) {
    switch (L) {
        case 1: fused_head_by_tiles<T, 1>(a, p, tpw, R); break;
        case 2: fused_head_by_tiles<T, 2>(a, p, tpw, R); break;
        case 4: fused_head_by_tiles<T, 4>(a, p, tpw, R); break;
        case 8: fused_head_by_tiles<T, 8>(a, p, tpw, R); break;
        default: fused_head_by_tiles<T, 16>(a, p, tpw, R); break;
    }
}

// workspace of pu_plastic_bwd_trace: [per-slot (T_b, T_b * H_b)] [deta partials, fp64]
// [dx0] [dy0] [row partials] [column partials]; sized for the scalar path's narrower strips
struct TraceBwdWs {
    size_t head, etap, dx0, dy0, rowp, colp, total;   // byte offsets
};

static TraceBwdWs trace_bwd_ws(int B, int N) {
    const size_t nchunks = ceil_div(N, TB_ROWS), nstrips = ceil_div(N, 32);
    TraceBwdWs o;
    o.head = 0;
    o.etap = (size_t)B * 2 * N * N * sizeof(float);
    o.dx0 = o.etap + (size_t)B * nchunks * nstrips * sizeof(double);
    o.dy0 = o.dx0 + (size_t)B * N * sizeof(float);
    o.rowp = o.dy0 + (size_t)B * N * sizeof(float);
    o.colp = o.rowp + (size_t)B * N * nstrips * sizeof(float);
    o.total = o.colp + (size_t)B * nchunks * N * sizeof(float);
    return o;
}

}  // namespace pu

using namespace pu;

extern "C" int pu_trace_update(const float* hebb, const float* x, const float* y, const float* eta, float* hebb_out,
                               int batch, int nbf, int rule, void* stream) {
    PU_REQUIRE(hebb && x && y && eta && hebb_out && batch > 0 && nbf > 0, "pu_trace_update: bad args");
    if (int st = check_rule(rule)) return st;
    PU_REQUIRE((long long)nbf * nbf < (1ll << 31), "pu_trace_update: nbf too large");
    if (nbf % 4 == 0 && ((((uintptr_t)hebb) | ((uintptr_t)hebb_out) | ((uintptr_t)y)) & 15) == 0) {
        dim3 grid(ceil_div((long long)nbf * nbf / 4, 256), batch);
        hipLaunchKernelGGL(trace_kernel_v4, grid, dim3(256), 0, as_stream(stream), hebb, x, y, eta, hebb_out, nbf, rule);
    } else {
        dim3 grid(ceil_div((long long)nbf * nbf, 256), batch);
        hipLaunchKernelGGL(trace_kernel, grid, dim3(256), 0, as_stream(stream), hebb, x, y, eta, hebb_out, nbf, rule);
    }
    return check_launch("pu_trace_update");
}

extern "C" int pu_plastic_fwd(const pu_plastic_args* a, void* stream) {
    PU_REQUIRE(a && a->x && a->hebb && a->w && a->alpha && a->y && a->batch > 0 && a->nbf > 0, "pu_plastic_fwd: bad args");
    if (int st = check_rule(a->rule)) return st;
    PU_REQUIRE(!a->hebb_out || a->eta, "pu_plastic_fwd: eta missing");
    // the fused update writes H' while other blocks still read H: an aliased output takes the
    // two-launch path (GEMM, then the stand-alone update)
    const bool fuse = a->hebb_out && a->hebb_out != a->hebb;
    hipStream_t s = as_stream(stream);
    float* hn = fuse ? a->hebb_out : nullptr;
    with_head_tile(a->batch, a->nbf, [&](auto T) { launch_head_fwd<decltype(T)::value>(a, hn, s); });
    int st = check_launch("pu_plastic_fwd");
    if (st != PU_OK || !a->hebb_out || fuse) return st;
    return pu_trace_update(a->hebb, a->x, a->y, a->eta, a->hebb_out, a->batch, a->nbf, a->rule, stream);
}


extern "C" int pu_plastic_head_fwd(const pu_plastic_head_args* a, void* stream) {
    PU_REQUIRE(a && a->feat && a->out_w && a->hebb && a->w && a->alpha && a->x && a->y && a->batch > 0,
               "pu_plastic_head_fwd: bad args");
    const int N = a->nbf, C = a->channels;
    PU_REQUIRE(N >= 16 && N % 16 == 0 && N <= 512, "pu_plastic_head_fwd: nbf %d must be a multiple of 16 in [16, 512]", N);
    PU_REQUIRE(C >= 4 && C % 4 == 0, "pu_plastic_head_fwd: channels %d must be a multiple of 4", C);
    PU_REQUIRE((((uintptr_t)a->feat | (uintptr_t)a->out_w) & 15) == 0 || (a->feat_bf16 && ((uintptr_t)a->feat & 7) == 0 &&
               ((uintptr_t)a->out_w & 15) == 0), "pu_plastic_head_fwd: feat / out_w alignment");
    if (int st = check_rule(a->rule)) return st;
    PU_REQUIRE(!a->hebb_out || (a->eta && a->hebb_out != a->hebb), "pu_plastic_head_fwd: hebb_out needs eta and no aliasing");
    PU_REQUIRE((long long)N * N * C * a->batch < (1LL << 40), "pu_plastic_head_fwd: too large");
    PU_REQUIRE((((uintptr_t)a->hebb | (uintptr_t)a->w | (uintptr_t)a->alpha | (uintptr_t)a->hebb_out) & 15) == 0,
               "pu_plastic_head_fwd: hebb / w / alpha / hebb_out must be 16-byte aligned");
    const int q = C / 4;
    const int L = q >= 16 ? 16 : (q & (q - 1)) == 0 ? q : 16;    // lanes per pixel
    // the pipelined kernel: N = 128, L = 16 lanes per pixel, the fused trace update
    // (PU_HEAD_PIPE=0 keeps the phase-serial kernel: A/B runs)
    static const bool pipe_on = [] {
        const char* e = getenv("PU_HEAD_PIPE");
        return !(e && e[0] == '0');
    }();
    // C >= 64: every streamer lane's first float4 (channels lane*4 .. lane*4+3 of the 16 lanes)
    // and its outconv weights lie inside the pixel; C = 12, 24, 48, 60 also give L = 16 but would
    // read the next pixel's channels (and past the end of wo / feat) - they take the serial kernel
    if (pipe_on && N == HP_N && L == 16 && C >= 64 && a->hebb_out) {
        const dim3 pg(N / 16, a->batch);
        if (a->feat_bf16)
            hipLaunchKernelGGL((head_pipe_fwd_kernel<__bf16>), pg, dim3(HP_NT), 0, as_stream(stream), (const __bf16*)a->feat,
                               a->out_w, a->out_b, C, a->hebb, a->w, a->alpha, a->eta, a->x, a->y, a->hebb_out, a->rule);
        else
            hipLaunchKernelGGL((head_pipe_fwd_kernel<float>), pg, dim3(HP_NT), 0, as_stream(stream), (const float*)a->feat,
                               a->out_w, a->out_b, C, a->hebb, a->w, a->alpha, a->eta, a->x, a->y, a->hebb_out, a->rule);
        return check_launch("pu_plastic_head_fwd");
    }
    const int kc = fused_head_chunk(N);                           // Weff rows per LDS chunk
    // rows per block: every block re-forms the whole W_eff = w + alpha (.) H of its slot, so at
    // nbf >= 256 (C4 / C5) 32-row blocks halve that work and feed each W fragment to two MFMA row
    // tiles (the LDS of 16-row blocks already held them to one block per CU there)
    const int R = (N >= 256 && N % 32 == 0 && ((size_t)(32 + 1) * N + (size_t)kc * N + N) * sizeof(float) <= 160 * 1024) ? 32 : FH_R;
    const size_t lds = ((size_t)(R + 1) * N + (size_t)kc * N + N) * sizeof(float);
    const FusedHeadLaunch p = {dim3(N / R, a->batch), lds, make_fastdiv(N), kc, as_stream(stream)};
    const int tpw = (N / 16 + FH_WAVES - 1) / FH_WAVES;           // column tiles per wave
    if (a->feat_bf16) fused_head_by_lanes<__bf16>(a, p, L, tpw, R);
    else fused_head_by_lanes<float>(a, p, L, tpw, R);
    return check_launch("pu_plastic_head_fwd");
}

extern "C" size_t pu_plastic_bwd_workspace_bytes(int batch, int nbf) {
    return (size_t)batch * 2 * nbf * nbf * sizeof(float);      // per-slot (T_b, T_b * H_b)
}

extern "C" int pu_plastic_bwd(const pu_plastic_bwd_args* a, void* workspace, size_t ws_bytes, void* stream) {
    PU_REQUIRE(a && a->x && a->hebb && a->w && a->alpha && a->y && a->dy && a->batch > 0 && a->nbf > 0,
               "pu_plastic_bwd: bad args");
    const int N = a->nbf, B = a->batch;
    hipStream_t s = as_stream(stream);
    float* ws = nullptr;
    if (a->dw || a->dalpha) {
        PU_REQUIRE(a->dw && a->dalpha, "pu_plastic_bwd: dw and dalpha go together");
        const size_t need = pu_plastic_bwd_workspace_bytes(B, N);
        if (!workspace || ws_bytes < need) return fail(PU_ERR_WORKSPACE, "pu_plastic_bwd: workspace %zu < %zu", ws_bytes, need);
        ws = (float*)workspace;
    }
    with_head_tile(B, N, [&](auto T) { launch_head_bwd<decltype(T)::value, false>(a, ws, nullptr, nullptr, s); });
    int st = check_launch("pu_plastic_bwd");
    if (st != PU_OK || !ws) return st;
    launch_dw_reduce(ws, B, N, a->dw, a->dalpha, s);
    return check_launch("pu_plastic_bwd (dw)");
}

extern "C" size_t pu_plastic_bwd_trace_workspace_bytes(int batch, int nbf) {
    if (batch <= 0 || nbf <= 0) return 0;
    return trace_bwd_ws(batch, nbf).total;
}

// trace backward -> head backward (with the row-0 extras) -> slot reduction -> dH finish, one stream.
// Without dhebb_out (no gradient reached H') the head kernels are pu_plastic_bwd's own
// instantiations: dx, dw, dalpha are bitwise that entry's.
extern "C" int pu_plastic_bwd_trace(const pu_plastic_bwd_trace_args* a, void* workspace, size_t ws_bytes, void* stream) {
    PU_REQUIRE(a && a->x && a->hebb && a->w && a->alpha && a->y && a->batch > 0 && a->nbf > 0,
               "pu_plastic_bwd_trace: bad args");
    PU_REQUIRE(a->dy || a->dhebb_out, "pu_plastic_bwd_trace: neither dy nor dhebb_out");
    if (int st = check_rule(a->rule)) return st;
    PU_REQUIRE(!a->dhebb_out || (a->eta && a->deta), "pu_plastic_bwd_trace: dhebb_out needs eta and deta");
    PU_REQUIRE((long long)a->nbf * a->nbf < (1ll << 31), "pu_plastic_bwd_trace: nbf too large");
    PU_REQUIRE(a->batch <= 65535, "pu_plastic_bwd_trace: batch too large");
    PU_REQUIRE(!a->dw == !a->dalpha, "pu_plastic_bwd_trace: dw and dalpha go together");
    const int N = a->nbf, B = a->batch;
    const TraceBwdWs L = trace_bwd_ws(B, N);
    if (!workspace || ws_bytes < L.total)
        return fail(PU_ERR_WORKSPACE, "pu_plastic_bwd_trace: workspace %zu < %zu", ws_bytes, L.total);
    PU_REQUIRE(((uintptr_t)workspace & 15) == 0, "pu_plastic_bwd_trace: workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    char* base = (char*)workspace;
    float* wsh = (a->dw || a->dhebb) ? (float*)(base + L.head) : nullptr;
    const bool vec = N % 4 == 0;
    const pu_plastic_bwd_args h = {B, N, a->x, a->hebb, a->w, a->alpha, a->y, a->dy, a->dx, nullptr, nullptr};
    if (a->dhebb_out) {
        double* etap = (double*)(base + L.etap);
        float* dx0 = (float*)(base + L.dx0);
        float* dy0 = (float*)(base + L.dy0);
        float* rowp = (float*)(base + L.rowp);
        float* colp = (float*)(base + L.colp);
        const int nchunks = ceil_div(N, TB_ROWS);
        int nstrips;
        if (vec && ((((uintptr_t)a->dhebb_out) | ((uintptr_t)a->hebb)) & 15) == 0) {
            nstrips = ceil_div(N, 128);
            hipLaunchKernelGGL(trace_bwd_partial_kernel<4>, dim3(nstrips, nchunks, B), dim3(256), 0, s, a->dhebb_out, a->hebb,
                               a->x, a->y, N, a->rule, rowp, colp, etap);
        } else {
            nstrips = ceil_div(N, 32);
            hipLaunchKernelGGL(trace_bwd_partial_kernel<1>, dim3(nstrips, nchunks, B), dim3(256), 0, s, a->dhebb_out, a->hebb,
                               a->x, a->y, N, a->rule, rowp, colp, etap);
        }
        hipLaunchKernelGGL(trace_bwd_finish_kernel, dim3(grid_for((long long)B * N, 256, 1024)), dim3(256), 0, s,
                           (const float*)rowp, (const float*)colp, (const double*)etap, a->eta, B, N, nstrips, nchunks,
                           B * nchunks * nstrips, dx0, dy0, a->deta);
        int st = check_launch("pu_plastic_bwd_trace (trace)");
        if (st != PU_OK) return st;
        with_head_tile(B, N, [&](auto T) { launch_head_bwd<decltype(T)::value, true>(&h, wsh, dx0, dy0, s); });
    } else {
        with_head_tile(B, N, [&](auto T) { launch_head_bwd<decltype(T)::value, false>(&h, wsh, nullptr, nullptr, s); });
    }
    int st = check_launch("pu_plastic_bwd_trace (head)");
    if (st != PU_OK || !wsh) return st;
    if (a->dw) launch_dw_reduce(wsh, B, N, a->dw, a->dalpha, s);
    if (a->dhebb) {
        const float* P = a->dhebb_out;
        if (vec && ((((uintptr_t)P) | ((uintptr_t)a->dhebb) | ((uintptr_t)a->alpha)) & 15) == 0)
            hipLaunchKernelGGL(head_dh_kernel<4>, dim3(ceil_div((long long)N * N / 4, 256), B), dim3(256), 0, s, P, a->y,
                               a->alpha, (const float*)wsh, a->eta, N, a->rule, a->dhebb);
        else
            hipLaunchKernelGGL(head_dh_kernel<1>, dim3(ceil_div((long long)N * N, 256), B), dim3(256), 0, s, P, a->y,
                               a->alpha, (const float*)wsh, a->eta, N, a->rule, a->dhebb);
    }
    return check_launch("pu_plastic_bwd_trace (dw, dH)");
}

extern "C" size_t pu_bce_workspace_bytes(long long n) {
    (void)n;
    return BCE_BLOCKS * sizeof(double);
}

extern "C" int pu_bce_fwd(const float* y, const float* t, long long n, float* loss, void* workspace, size_t ws_bytes,
                          void* stream) {
    PU_REQUIRE(y && t && loss && n > 0, "pu_bce_fwd: bad args");
    if (!workspace || ws_bytes < pu_bce_workspace_bytes(n)) return fail(PU_ERR_WORKSPACE, "pu_bce_fwd: workspace");
    PU_REQUIRE(((uintptr_t)workspace & 7) == 0, "pu_bce_fwd: workspace must be 8-byte aligned");   // fp64 partials
    int blocks = bce_grid(n);
    hipLaunchKernelGGL(bce_partial_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), y, t, n, (double*)workspace);
    hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const double*)workspace, blocks, n,
                       loss);
    return check_launch("pu_bce_fwd");
}

extern "C" int pu_bce_bwd(const float* y, const float* t, long long n, const float* grad_loss, float* dy, void* stream) {
    PU_REQUIRE(y && t && dy && n > 0, "pu_bce_bwd: bad args");
    hipLaunchKernelGGL(bce_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), y, t, n, grad_loss, dy);
    return check_launch("pu_bce_bwd");
}
