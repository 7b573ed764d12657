"""Every kernel of csrc/plastic.hip and csrc/adam.hip against fp64, launch branch by launch branch: the
case table, the launchers' rules, the references with their per-entry bounds and the guarded device
runner shared by test_head_matrix.py (CPU) and test_head_matrix_gpu.py.  Built in the shape of
tests/layer_matrix.py (Row / P / FORMS / excluded / kernel_of / pinned, Guarded / _dev).

The two files compile to 74 kernel instantiations: head_fused_fwd_kernel<T, L, TPW, R> x 50,
head_pipe_fwd_kernel<T> x 2, head_fwd_kernel<32 / 64>, head_dx_kernel / head_dw_kernel<32 / 64, EX>,
trace_bwd_partial_kernel<4 / 1>, head_dh_kernel<4 / 1>, trace_kernel, trace_kernel_v4,
head_dw_reduce_kernel, trace_bwd_finish_kernel, the three BCE kernels and adam_kernel.  Every call goes
through the C ABI (punet._lib): only it can pass NULL operands, a pointer four bytes off 16-byte
alignment and a workspace of exactly the queried size.

Entry points (Row.entry): head = pu_plastic_head_fwd, fwd = pu_plastic_fwd, trace = pu_trace_update,
bwd = pu_plastic_bwd, bwdt = pu_plastic_bwd_trace, bce_fwd, bce_bwd, adam = pu_adam_multi.

Bounds (derived, not measured), u = 2^-24, e = 2^-53, M the sum of the absolute values of the terms of
the entry.  A value that passed through d roundings on its way into a sum carries at most d u of
itself, so a sum is bounded by (the deepest path) u M:
  bit-exact    the trace update H' (every entry point that writes one, given the call's own X[:, 0] and
               Y[:, 0]), bce_bwd, Adam's p / m / v (scalars cast to float32 as the entry does),
               head_dw_reduce_kernel given the slab the call left in the workspace: the same float32
               expressions evaluated op by op in numpy (both files disable contraction; hipcc rounds
               fp32 division and sqrt correctly by default, and the build passes no fast-math flag);
               the identities (fused head = outconv, then pu_plastic_fwd; fused trace = GEMM, then
               pu_trace_update; no-dhebb_out trace backward = pu_plastic_bwd; pipelined = serial):  0
  outconv X    a lane's dot4 (a product and three fmas: 4), one addition per channel round
               (ceil(C / 4L) rounds), log2 L shuffle additions, the bias, one unit of slack:
               (ceil(C / 4L) + log2 L + 6) u M,  M = sum |feat| |wo| + |bo|
  Weff         w + alpha H: the product and the sum, bound_W = 2 u (|w| + |alpha| |H|) = 2 u M_W
  a = X Weff   an N-term fma chain (the MFMA is the same k-ordered chain), Weff's two roundings, slack:
               (N + 3) u (|X| M_W) + bound_X M_W
  sigmoid      Y = 1 / (1 + expf(-a)): bound_Y = s'(a*) bound_a + k u Y + 2^-126 with a* the point of
               [a - bound_a, a + bound_a] nearest 0 (s' decreases in |a|) and k = 2 ULP_EXP + 3: expf
               is off by ULP_EXP ulps = 2 ULP_EXP u of exp(-a), which moves Y by at most that; one
               addition, one division, slack.  2^-126 covers a result below the normal range
  H' in fp64   (the CPU sensitivity checks and a second GPU check) five operations on
               M = |H| + eta |x0| |y0| (Oja: + eta |H| y0^2) plus eta (|y0| bound_x0 + |x0| bound_y0)
               (Oja: + 2 eta |H| |y0| bound_y0)
  G            dY (1 - Y) Y: three roundings, carried in the chain counts below
  dX           G Weff^T, an N-term chain: (N + 6) u (|G| M_W^T)       (3 of G, 2 of Weff, slack)
  T_b, dw, da  T_b = X_b^T G_b: (N + 4) u M_T, M_T = |X|^T |G|; dw adds the B slots in order:
               + B u sum_b M_T; dalpha = sum_b T_b H_b one product more: (N + B + 5) u sum_b M_T |H_b|
               (H = 0: bound 0, dalpha is exactly 0)
  dx0          per strip V in-lane products added in turn (V), a 32-lane xor tree (5), the strips in
               order (nstrips), times eta, slack: (V + nstrips + 7) u M, M = eta sum_j |P| |y0|
  dy0          a term takes up to 4 roundings (Oja: h y0, x0 - 2 h y0, the product, the addition), two
               rows per lane (2), the 8 groups (8), the chunks in order (nchunks), times eta, slack:
               (nchunks + 16) u M, M = eta sum_k |P| (|x0| + 2 |H| |y0|)   (Hebb: eta sum_k |P| |x0|)
  EX extras    row 0 of dY gains dy0 (one addition): bound_G[0] = (1 - y) y (bound_dy0 + u (|dY| + M_dy0))
               enters dX through M_W and T_b through |X[0]|; row 0 of dX gains dx0 (one addition):
               + bound_dx0 + u (M_dX + M_dx0)
  dH           p f + alpha t with f = 1 - eta (1 rounding) or 1 - eta y0^2 (3): 6 u (|P| (1 + eta y0^2)
               + |alpha| M_T) + |alpha| bound_T; without P one product: 2 u |alpha| M_T + |alpha| bound_T
  deta         fp32 terms of at most 4 roundings summed in fp64 in some order, stored once:
               4 u M + (n + 2) e M + u |deta|, n = B N^2, M = sum |P| (|x0| |y0| + |H|)
               (Oja: sum |P| |y0| (|x0| + |H| |y0|))
  BCE loss     a term (t - 1) max(log1p(-y), -100) - t max(log y, -100): the logarithm is off by
               ULP_LOG ulps = 2 ULP_LOG u, t - 1, the product, the subtraction, slack:
               ((2 ULP_LOG + 4) u + (n + 3) e) M / n + u |loss|
ULP_EXP = 1 and ULP_LOG = 2 (logf 2, log1pf 1) are the figures of the HIP programming guide's table of
math-function accuracy as recalled: no copy of the ROCm documentation is installed beside the toolkit
this was written against (DESIGN.md 4d records that).  No constant here is fitted to a kernel's
output; test_head_matrix.py checks that every bound rejects the mutants of MUTANTS.
"""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

from punet import _lib
from conv_epilogue import Guarded, _dev    # the shared sentinel idiom
from layer_matrix import BF, E53, F32, F64, INVALID, OK, WORKSPACE, P, Row, U, ratio  # noqa: F401

ULP_EXP, ULP_LOG = 1, 2
K_SIG = 2 * ULP_EXP + 3
TINY = 2.0 ** -126
ETA = float(np.float32(0.0137))
FH_LDS_W, FH_WAVES, HK, TB_ROWS, BCE_BLOCKS, ADAM_MAX_T, ADAM_CHUNK = 16384, 8, 16, 16, 512, 32, 4096
SOURCES = ("plastic.hip", "adam.hip")
KERNEL_COUNT = 74
_T = {"f32": "f", "bf16": "b"}
_DT = {"f32": F32, "bf16": BF}


def _r(name, entry, kernels, **p):
    return Row(name, entry, frozenset([kernels] if isinstance(kernels, str) else kernels), P(p))


def _forms(*items):
    return collections.OrderedDict((nm, P(opts)) for nm, opts in items)


# ------------------------------------------------------------------------------------------- forms
FORMS = {
    # train: hebb_out passed; bias: out_b passed
    "head": _forms(("train", dict(train=1, bias=1)), ("eval", dict(bias=1)), ("train, no bias", dict(train=1)),
                   ("eval, no bias", {})),
    "fwd": _forms(("no hebb_out", {}), ("fused", dict(train=1)), ("aliased", dict(train=1, alias=1))),
    "trace": _forms(("plain", dict(train=1))),
    "bwd": _forms(("dx", dict(dx=1)), ("dw", dict(dw=1)), ("both", dict(dx=1, dw=1)), ("both, dw + 4 B", dict(dx=1, dw=1, dwmis=1))),
    # dy, P = dhebb_out: the two incoming gradients; dx, dw (with dalpha), dh = dhebb: the outputs asked for
    "bwdt": _forms(("all", dict(dy=1, P=1, dx=1, dw=1, dh=1)), ("no dy", dict(P=1, dx=1, dw=1, dh=1)),
                   ("no dhebb", dict(dy=1, P=1, dx=1, dw=1)), ("no dx", dict(dy=1, P=1, dw=1, dh=1)),
                   ("no dw", dict(dy=1, P=1, dx=1, dh=1)), ("no dhebb_out", dict(dy=1, dx=1, dw=1, dh=1))),
    "bce_fwd": _forms(("plain", {})),
    "bce_bwd": _forms(("no grad_loss", {}), ("grad_loss", dict(g=1))),
    "adam": _forms(("plain", {})),
}


def excluded(r, f):
    """The explicit rules that leave a (row, form) pair out."""
    if r.p.big and r.entry == "bwdt" and not (f.dy and f.P and f.dx and f.dw and f.dh):
        return "the 17 MB row runs with every operand only"
    if r.entry == "bwdt" and ((r.p.mis == "dhebb_out" and not f.P) or (r.p.mis == "dhebb" and not f.dh)):
        return "the misaligned operand is absent"
    return None


# ---------------------------------------------------------------------------------- launchers' rules
def head_small_tiles(B, N):
    return (-(-N // 64)) ** 2 * B < 512


def fused_head_chunk(N):
    if N * N <= FH_LDS_W:
        return N
    best, d = 16, 4
    while d * N <= FH_LDS_W and d <= N:
        if N % d == 0:
            best = d
        d += 4
    return best


def head_plan(N, C):
    """(L, TPW, R, kc) of pu_plastic_head_fwd's serial kernel"""
    q = C // 4
    L = 16 if q >= 16 else q if q & (q - 1) == 0 else 16
    kc = fused_head_chunk(N)
    R = 32 if N >= 256 and N % 32 == 0 and (33 * N + kc * N + N) * 4 <= 160 * 1024 else 16
    tpw = (N // 16 + FH_WAVES - 1) // FH_WAVES
    return L, 1 if tpw <= 1 else 2 if tpw <= 2 else 4, R, kc


def grid_for(total, block=256, cap=8192):
    return max(1, min(-(-total // block), cap))


def trace_plan(p, f):
    """pu_plastic_bwd_trace: (V of trace_bwd_partial_kernel, nstrips, nchunks, V of head_dh_kernel)"""
    vec = p.N % 4 == 0
    V = 4 if vec and p.mis not in ("dhebb_out", "hebb") else 1
    Vh = 4 if vec and not (p.mis == "dhebb_out" and f.P) and p.mis not in ("dhebb", "alpha") else 1
    return V, -(-p.N // (32 * V)), -(-p.N // TB_ROWS), Vh


def bwdt_ws(B, N):
    """the workspace of pu_plastic_bwd_trace: the slab, the fp64 deta partials, dx0, dy0, the row and
    column partials - the strips counted at 32 columns, whichever kernel runs"""
    nch, ns = -(-N // TB_ROWS), -(-N // 32)
    return 8 * B * N * N + 8 * B * nch * ns + 8 * B * N + 4 * B * N * ns + 4 * B * nch * N


def adam_launches(numels):
    """block counts of the launches of pu_adam_multi: 32 tensors a launch, empty ones not counted"""
    full = [n for n in numels if n]
    return [sum(-(-n // ADAM_CHUNK) for n in full[i:i + ADAM_MAX_T]) for i in range(0, len(full), ADAM_MAX_T)]


def kernel_of(r, f=None):
    """The instantiations the row's call launches in form f (None: in any of its forms): the
    launcher's rule applied to its arguments."""
    if f is None:
        return frozenset().union(*(kernel_of(r, g) for _, g in forms(r)))
    p, e = r.p, r.entry
    if e == "head":
        L, TPW, R, kc = head_plan(p.N, p.C)
        if p.N == 128 and L == 16 and p.C >= 64 and f.train:
            return frozenset(["head_pipe_fwd_kernel<%s>" % _T[p.dt]])
        return frozenset(["head_fused_fwd_kernel<%s,%d,%d,%d>" % (_T[p.dt], L, TPW, R)])
    tile = 32 if head_small_tiles(p.B or 1, p.N or 1) else 64
    if e == "fwd":
        ks = ["head_fwd_kernel<%d>" % tile]
        if f.alias:
            ks.append("trace_kernel_v4" if p.N % 4 == 0 else "trace_kernel")
        return frozenset(ks)
    if e == "trace":
        return frozenset(["trace_kernel_v4" if p.N % 4 == 0 and p.mis is None else "trace_kernel"])
    if e == "bwd":
        ks = ["head_dx_kernel<%d,0>" % tile] if f.dx else []
        return frozenset(ks + (["head_dw_kernel<%d,0>" % tile, "head_dw_reduce_kernel"] if f.dw else []))
    if e == "bwdt":
        V, _, _, Vh = trace_plan(p, f)
        ex = 1 if f.P else 0
        ks = ["trace_bwd_partial_kernel<%d>" % V, "trace_bwd_finish_kernel"] if f.P else []
        if f.dx:
            ks.append("head_dx_kernel<%d,%d>" % (tile, ex))
        if f.dw or f.dh:
            ks.append("head_dw_kernel<%d,%d>" % (tile, ex))
        if f.dw:
            ks.append("head_dw_reduce_kernel")
        if f.dh:
            ks.append("head_dh_kernel<%d>" % Vh)
        return frozenset(ks)
    if e == "bce_fwd":
        return frozenset(["bce_partial_kernel", "bce_final_kernel"])
    if e == "bce_bwd":
        return frozenset(["bce_bwd_kernel"])
    if e == "adam":
        return frozenset(["adam_kernel"])
    raise KeyError(e)


def plan_of(r):
    """what the launcher's rule and the library's queries (no GPU) give for the row, in the order of pinned()"""
    L, p, e = _lib.load(), r.p, r.entry
    if e == "head":
        return head_plan(p.N, p.C)
    tile = 32 if head_small_tiles(p.B or 1, p.N or 1) else 64
    if e in ("fwd", "trace"):
        return (tile,)
    if e == "bwd":
        return tile, L.pu_plastic_bwd_workspace_bytes(p.B, p.N)
    if e == "bwdt":
        V, ns, nch, Vh = trace_plan(p, FORMS["bwdt"]["all"])
        return tile, V, ns, nch, Vh, L.pu_plastic_bwd_trace_workspace_bytes(p.B, p.N)
    if e == "bce_fwd":
        return grid_for(p.n, 256, BCE_BLOCKS), L.pu_bce_workspace_bytes(p.n)
    if e == "bce_bwd":
        return (grid_for(p.n),)
    if e == "adam":
        return (tuple(adam_launches(p.numels)),)
    raise KeyError(e)


def pinned(r):
    p, e = r.p, r.entry
    if e == "head":
        return p.L, p.TPW, p.R, p.kc
    if e in ("fwd", "trace"):
        return (p.tile,)
    if e == "bwd":
        return p.tile, p.ws
    if e == "bwdt":
        return p.tile, p.V, p.ns, p.nch, p.Vh, p.ws
    if e == "bce_fwd":
        return p.blocks, 4096
    if e == "bce_bwd":
        return (p.blocks,)
    if e == "adam":
        return (p.launches,)
    raise KeyError(e)


# ---------------------------------------------------------------------------------------- case table
def _h(dt, B, N, C, rule, L, TPW, R, kc, **kw):
    t = _T[dt]
    ks = ["head_fused_fwd_kernel<%s,%d,%d,%d>" % (t, L, TPW, R)]
    if N == 128 and C >= 64:
        ks.append("head_pipe_fwd_kernel<%s>" % t)
    name = "head %s B %d N %d C %d %s%s" % (dt, B, N, C, ("hebb", "oja")[rule], " " + kw["data"] if kw.get("data") else "")
    return _r(name, "head", ks, dt=dt, B=B, N=N, C=C, rule=rule, L=L, TPW=TPW, R=R, kc=kc, **kw)


def _f(B, N, rule, tile, **kw):
    name = "fwd B %d N %d %s%s" % (B, N, ("hebb", "oja")[rule], " " + kw["data"] if kw.get("data") else "")
    ks = ["head_fwd_kernel<%d>" % tile, "trace_kernel_v4" if N % 4 == 0 else "trace_kernel"]
    return _r(name, "fwd", ks, B=B, N=N, rule=rule, tile=tile, **kw)


def _b(B, N, tile, **kw):
    name = "bwd B %d N %d%s" % (B, N, " " + kw["data"] if kw.get("data") else "")
    ks = ["head_dx_kernel<%d,0>" % tile, "head_dw_kernel<%d,0>" % tile, "head_dw_reduce_kernel"]
    return _r(name, "bwd", ks, B=B, N=N, tile=tile, ws=8 * B * N * N, **kw)


def _bt(B, N, rule, tile, V, ns, nch, Vh, ws, mis=None, **kw):
    name = "bwdt B %d N %d %s%s%s" % (B, N, ("hebb", "oja")[rule], ", %s + 4 B" % mis if mis else "",
                                      " " + kw["data"] if kw.get("data") else "")
    ks = ["trace_bwd_partial_kernel<%d>" % V, "trace_bwd_finish_kernel", "head_dw_reduce_kernel"]
    ks += ["head_dx_kernel<%d,1>" % tile, "head_dw_kernel<%d,1>" % tile]
    if not kw.get("big") and mis != "dhebb_out":   # the no-dhebb_out form: pu_plastic_bwd's own instantiations
        ks += ["head_dx_kernel<%d,0>" % tile, "head_dw_kernel<%d,0>" % tile]
    ks += ["head_dh_kernel<%d>" % Vh]
    return _r(name, "bwdt", ks, B=B, N=N, rule=rule, tile=tile, V=V, ns=ns, nch=nch, Vh=Vh, ws=ws, mis=mis, **kw)


def _adam(name, numels, launches, **kw):
    return _r("adam " + name, "adam", "adam_kernel", numels=tuple(numels), launches=tuple(launches), **kw)


HEAD = [
    # ---- every reachable <T, L, TPW, R> of the serial kernel: (dt, B, N, C, rule | L, TPW, R, kc pinned)
    _h("f32", 2, 16, 4, 0, 1, 1, 16, 16), _h("f32", 2, 144, 4, 1, 1, 2, 16, 72), _h("f32", 2, 256, 4, 0, 1, 2, 32, 64),
    _h("f32", 1, 272, 4, 1, 1, 4, 16, 16), _h("f32", 1, 512, 4, 0, 1, 4, 32, 32),
    _h("f32", 2, 48, 8, 1, 2, 1, 16, 48), _h("f32", 2, 160, 8, 0, 2, 2, 16, 80), _h("f32", 1, 256, 8, 1, 2, 2, 32, 64),
    _h("f32", 1, 272, 8, 0, 2, 4, 16, 16), _h("f32", 1, 384, 8, 1, 2, 4, 32, 32),
    _h("f32", 2, 16, 16, 0, 4, 1, 16, 16), _h("f32", 1, 192, 16, 1, 4, 2, 16, 64), _h("f32", 1, 256, 16, 0, 4, 2, 32, 64),
    _h("f32", 1, 272, 16, 1, 4, 4, 16, 16), _h("f32", 1, 320, 16, 0, 4, 4, 32, 40),
    _h("f32", 2, 48, 32, 1, 8, 1, 16, 48), _h("f32", 2, 144, 32, 0, 8, 2, 16, 72), _h("f32", 1, 256, 32, 1, 8, 2, 32, 64),
    _h("f32", 1, 272, 32, 0, 8, 4, 16, 16), _h("f32", 1, 288, 32, 1, 8, 4, 32, 48),
    _h("f32", 2, 16, 64, 0, 16, 1, 16, 16), _h("f32", 1, 160, 64, 1, 16, 2, 16, 80), _h("f32", 1, 256, 20, 0, 16, 2, 32, 64),
    _h("f32", 1, 272, 12, 1, 16, 4, 16, 16), _h("f32", 1, 288, 20, 0, 16, 4, 32, 48),
    _h("bf16", 2, 48, 4, 1, 1, 1, 16, 48), _h("bf16", 2, 160, 4, 0, 1, 2, 16, 80), _h("bf16", 1, 256, 4, 1, 1, 2, 32, 64),
    _h("bf16", 1, 272, 4, 0, 1, 4, 16, 16), _h("bf16", 1, 384, 4, 1, 1, 4, 32, 32),
    _h("bf16", 2, 16, 8, 0, 2, 1, 16, 16), _h("bf16", 1, 192, 8, 1, 2, 2, 16, 64), _h("bf16", 2, 256, 8, 0, 2, 2, 32, 64),
    _h("bf16", 1, 272, 8, 1, 2, 4, 16, 16), _h("bf16", 1, 512, 8, 0, 2, 4, 32, 32),
    _h("bf16", 2, 48, 16, 1, 4, 1, 16, 48), _h("bf16", 2, 144, 16, 0, 4, 2, 16, 72), _h("bf16", 1, 256, 16, 1, 4, 2, 32, 64),
    _h("bf16", 1, 272, 16, 0, 4, 4, 16, 16), _h("bf16", 1, 288, 16, 1, 4, 4, 32, 48),
    _h("bf16", 2, 16, 32, 0, 8, 1, 16, 16), _h("bf16", 1, 160, 32, 1, 8, 2, 16, 80), _h("bf16", 1, 256, 32, 0, 8, 2, 32, 64),
    _h("bf16", 1, 272, 32, 1, 8, 4, 16, 16), _h("bf16", 1, 320, 32, 0, 8, 4, 32, 40),
    _h("bf16", 2, 48, 64, 1, 16, 1, 16, 48), _h("bf16", 1, 192, 20, 0, 16, 2, 16, 64), _h("bf16", 1, 256, 12, 1, 16, 2, 32, 64),
    _h("bf16", 1, 272, 20, 0, 16, 4, 16, 16), _h("bf16", 1, 384, 12, 1, 16, 4, 32, 32),
    # ---- C no power of two (L = 16 with idle lanes) and C = 128 (two channel rounds) at one tile per wave
    _h("f32", 1, 48, 12, 0, 16, 1, 16, 48), _h("bf16", 1, 16, 20, 1, 16, 1, 16, 16),
    _h("f32", 1, 16, 128, 1, 16, 1, 16, 16), _h("bf16", 1, 48, 128, 0, 16, 1, 16, 48),
    # ---- N = 128: the pipelined kernel with hebb_out (C 64: no second round; 68: lane 0 only; 96; 128),
    # the serial one without; C 48 is serial in both forms.  B 8 and 9: the XCD block order with
    # every slot on one XCD, and with one slot across two (16.8 and 18.9 MB of bf16 features)
    _h("f32", 1, 128, 64, 0, 16, 1, 16, 128), _h("f32", 1, 128, 68, 1, 16, 1, 16, 128),
    _h("f32", 1, 128, 96, 0, 16, 1, 16, 128), _h("f32", 1, 128, 128, 1, 16, 1, 16, 128),
    _h("f32", 2, 128, 64, 1, 16, 1, 16, 128),
    _h("bf16", 1, 128, 64, 1, 16, 1, 16, 128), _h("bf16", 1, 128, 68, 0, 16, 1, 16, 128),
    _h("bf16", 1, 128, 96, 1, 16, 1, 16, 128), _h("bf16", 1, 128, 128, 0, 16, 1, 16, 128),
    _h("bf16", 8, 128, 64, 0, 16, 1, 16, 128, big=1), _h("bf16", 9, 128, 64, 1, 16, 1, 16, 128, big=1),
    _h("f32", 2, 128, 48, 0, 16, 1, 16, 128), _h("bf16", 2, 128, 48, 1, 16, 1, 16, 128),
    # ---- saturated pre-activations: |a| > 88 and 17 < |a| < 88
    _h("f32", 2, 48, 64, 0, 16, 1, 16, 48, data="sat"), _h("f32", 1, 128, 64, 1, 16, 1, 16, 128, data="sat"),
]

CASES = HEAD + [
    # ---- pu_plastic_fwd (B, N, rule | the tile)
    _f(1, 1, 0, 32), _f(5, 3, 1, 32), _f(1, 16, 0, 32), _f(2, 17, 1, 32), _f(3, 50, 0, 32), _f(512, 16, 1, 64),
    _f(128, 72, 0, 64), _f(32, 200, 1, 64), _f(3, 50, 1, 32, data="sat"),
    # ---- pu_trace_update
    _r("trace v4 N 16", "trace", "trace_kernel_v4", B=2, N=16, rule=0, tile=32),
    _r("trace N 18", "trace", "trace_kernel", B=2, N=18, rule=1, tile=32),
    _r("trace N 16, hebb + 4 B", "trace", "trace_kernel", B=2, N=16, rule=1, tile=32, mis="hebb"),
    _r("trace N 16, hebb_out + 4 B", "trace", "trace_kernel", B=2, N=16, rule=0, tile=32, mis="hebb_out"),
    _r("trace N 16, y + 4 B", "trace", "trace_kernel", B=2, N=16, rule=1, tile=32, mis="y"),
    # ---- pu_plastic_bwd (B, N | the tile): the shapes of HEAD_BWD_CASES (tests/test_train_tail_gpu.py)
    _b(1, 16, 32), _b(2, 17, 32), _b(5, 3, 32), _b(3, 50, 32), _b(2, 200, 32), _b(128, 72, 64), _b(32, 200, 64),
    _b(3, 50, 32, data="zero_h"), _b(128, 72, 64, data="zero_h"), _b(2, 17, 32, data="sat"),
    # ---- pu_plastic_bwd_trace (B, N, rule | tile, V, nstrips, nchunks, V of head_dh, workspace bytes)
    _bt(2, 128, 0, 32, 4, 1, 8, 4, 276992), _bt(2, 128, 1, 32, 4, 1, 8, 4, 276992),
    _bt(2, 132, 0, 32, 4, 2, 9, 4, 296400), _bt(2, 132, 1, 32, 4, 2, 9, 4, 296400),
    _bt(2, 18, 0, 32, 1, 1, 2, 1, 5936), _bt(2, 18, 1, 32, 1, 1, 2, 1, 5936),
    _bt(2, 34, 0, 32, 1, 2, 3, 1, 20496), _bt(2, 34, 1, 32, 1, 2, 3, 1, 20496),
    _bt(3, 50, 1, 32, 1, 2, 4, 1, 64992),
    _bt(2, 132, 1, 32, 1, 5, 9, 1, 296400, mis="dhebb_out"), _bt(2, 132, 0, 32, 1, 5, 9, 4, 296400, mis="hebb"),
    _bt(2, 16, 0, 32, 4, 1, 1, 1, 4624, mis="dhebb"), _bt(2, 16, 1, 32, 4, 1, 1, 1, 4624, mis="alpha"),
    _bt(128, 72, 1, 64, 4, 1, 5, 4, 5692416),
    _bt(3, 50, 0, 32, 1, 2, 4, 1, 64992, data="zero_h"), _bt(2, 34, 1, 32, 1, 2, 3, 1, 20496, data="sat"),
    # B N = 262160 > 1024 blocks x 256 threads: trace_bwd_finish_kernel at its block cap and on the second
    # trip of its grid-stride loop; 16385 x 16 x 16 floats = 16.8 MB per operand
    _bt(16385, 16, 1, 64, 4, 1, 1, 4, 37882120, big=1),
    # ---- BCE (n | blocks)
    _r("bce fwd n 1", "bce_fwd", {"bce_partial_kernel", "bce_final_kernel"}, n=1, blocks=1),
    _r("bce fwd n 255", "bce_fwd", {"bce_partial_kernel", "bce_final_kernel"}, n=255, blocks=1),
    _r("bce fwd n 257", "bce_fwd", {"bce_partial_kernel", "bce_final_kernel"}, n=257, blocks=2),
    _r("bce fwd n 5000", "bce_fwd", {"bce_partial_kernel", "bce_final_kernel"}, n=5000, blocks=20),
    _r("bce fwd block cap, second trip", "bce_fwd", {"bce_partial_kernel", "bce_final_kernel"}, n=131072 + 257, blocks=512),
    _r("bce bwd n 1", "bce_bwd", "bce_bwd_kernel", n=1, blocks=1),
    _r("bce bwd n 255", "bce_bwd", "bce_bwd_kernel", n=255, blocks=1),
    _r("bce bwd n 257", "bce_bwd", "bce_bwd_kernel", n=257, blocks=2),
    _r("bce bwd n 5000", "bce_bwd", "bce_bwd_kernel", n=5000, blocks=20),
    # 8192 blocks x 256 threads + 5: 8.4 MB per operand
    _r("bce bwd block cap, second trip", "bce_bwd", "bce_bwd_kernel", n=8192 * 256 + 5, blocks=8192, big=1),
    # ---- multi-tensor Adam (numels | blocks per launch)
    _adam("sizes, step 1", (1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 5), (12,), wd=0.0, step=1),
    _adam("sizes, weight decay, step 1000", (1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 5), (12,), wd=0.01, step=1000),
    _adam("p + 4 B", (4097, 9), (3,), wd=0.01, step=7, mis=(0, "p")),
    _adam("g + 4 B", (4097, 9), (3,), wd=0.0, step=7, mis=(0, "g")),
    _adam("m + 4 B", (4097, 9), (3,), wd=0.0, step=1, mis=(0, "m")),
    _adam("v + 4 B", (9, 4097), (3,), wd=0.01, step=1000, mis=(1, "v")),
    _adam("an empty tensor between full ones", (4096, 0, 5), (2,), wd=0.0, step=3),
    _adam("33 tensors", tuple(range(1, 34)), (32, 1), wd=0.01, step=2),
    _adam("65 tensors", tuple(7 + (i % 5) for i in range(65)), (32, 32, 1), wd=0.0, step=1000),
]
CASE = {r.name: r for r in CASES}
assert len(CASE) == len(CASES)
PAIR_COUNT = 467          # pinned: test_head_matrix.py derives it from the table and the exclusion rules


def forms(r):
    return [(nm, f) for nm, f in FORMS[r.entry].items() if excluded(r, f) is None]


def pairs():
    return [(r.name, nm) for r in CASES for nm, _ in forms(r)]


# --------------------------------------------------------------------------------------------- values
def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def values(name):
    """The operands of a row (CPU fp32 tensors; bf16 rows hold bf16 values), at the scales of the head
    tests of test_kernels_gpu.py.  Seeded by the name; computed once and left unchanged."""
    r = CASE[name]
    p, e = r.p, r.entry
    g = _gen(name)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    v = {}
    if e in ("head", "fwd", "trace", "bwd", "bwdt"):
        B, N = p.B, p.N
        H = 0.2 * rn(B, N, N)
        if p.data == "zero_h":
            H = torch.zeros(B, N, N)                         # the first step's trace: dalpha is exactly 0
        w = 0.05 * rn(N, N) * (100.0 if p.data == "sat" else 1.0)
        v.update(H=H, w=w, al=0.05 * ru(N, N), eta=torch.tensor([ETA]))
    if e == "head":
        feat = rn(p.B, p.N, p.N, p.C).relu_()
        v.update(feat=feat.to(BF).float() if p.dt == "bf16" else feat, wo=0.2 * rn(p.C), bo=rn(1))
    elif e in ("fwd", "trace", "bwd", "bwdt"):
        v["X"] = 2.0 * rn(p.B, p.N, p.N)
    if e in ("trace", "bwd", "bwdt"):
        Y = ru(p.B, p.N, p.N)
        if e != "trace":
            if p.data == "sat":                              # the forward's own Y of saturated pre-activations
                Y = torch.sigmoid(v["X"] @ (v["w"] + v["al"] * v["H"]))
            Y.view(-1)[::7] = 0.0                            # exact 0 and 1: G = 0 exactly
            Y.view(-1)[3::11] = 1.0
            s = 2.0 ** -4 if p.big else 1.0
            v.update(dY=rn(p.B, p.N, p.N) * s, P=rn(p.B, p.N, p.N) * s)
        v["Y"] = Y
    if e in ("bce_fwd", "bce_bwd"):
        n = p.n
        y = ru(n).clamp_(1e-6, 1 - 1e-6)
        t = (ru(n) > 0.5).float()
        if n > 16:
            # y of exactly 0 and 1 against either target (the -100 clamp; bwd: the 1e-12 floor), a y
            # whose (1 - y) y is below the floor, the last y below 1, soft targets
            y[:10] = torch.tensor([0.0, 1.0, 0.0, 1.0, 1e-30, 1e-13, 1.0 - 2.0 ** -24, 1e-30, 0.25, 0.75])
            t[:10] = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.3, 0.7])
        v.update(y=y, t=t, g=torch.tensor([0.37]))
    if e == "adam":
        late = p.step > 1
        for k in "pgmv":
            v[k] = [rn(n) * (1.0 if k in "pg" else 0.1 if late else 0.0) for n in p.numels]
        v["v"] = [t.abs() * 0.1 for t in v["v"]]
    return v


# ----------------------------------------------------------------------------------------- references
# every reference returns {output name: (value, bound)}: the fp64 value (an exact class: the tensor in
# float32) and the absolute bound of every entry; bound 0 = bit for bit
MUTANTS = ("trace from slot 0's row 0", "x0 and y0 swapped", "oja without - h y0", "Weff as (w + alpha) H",
           "last k of the GEMM dropped", "outconv last channel group dropped", "outconv bias dropped",
           "one strip's row partial dropped", "last chunk's column partial dropped", "deta of slot 0 only",
           "dy0 added to every row", "dx0 omitted", "oja dy0 without the factor 2", "slot sum without the last slot",
           "bce without the clamp", "bce dy without / n", "adam beta2 as 1 - beta2", "adam bias correction of step t - 1")


def _zero(t):
    return torch.zeros(t.shape, dtype=F64)


def trace_np(H, x0, y0, eta, rule, mutant=None):
    """H' in numpy float32, one operation at a time, in the order of trace_rule (csrc/head_common.h):
    H [B, N, N], x0 / y0 [B, N], eta a float32"""
    f = np.float32
    H, x0, y0, eta = (np.asarray(t, dtype=f) for t in (H, x0, y0, eta))
    eta = f(eta.reshape(-1)[0])
    if mutant == "trace from slot 0's row 0":
        x0, y0 = np.broadcast_to(x0[:1], x0.shape), np.broadcast_to(y0[:1], y0.shape)
    if mutant == "x0 and y0 swapped":
        x0, y0 = y0, x0
    xk, yj = x0[:, :, None], y0[:, None, :]
    if rule == 0:
        one_m = f(1) - eta
        out = (one_m * H).astype(f) + (eta * (xk * yj).astype(f)).astype(f)
    elif mutant == "oja without - h y0":
        out = H + (eta * (xk * yj).astype(f)).astype(f)
    else:
        out = H + (eta * ((xk - (H * yj).astype(f)).astype(f) * yj).astype(f)).astype(f)
    return torch.from_numpy(np.ascontiguousarray(out.astype(f)))


def _trace64(rule, eta, H, x0, y0, bx0, by0, mutant):
    if mutant == "trace from slot 0's row 0":
        x0, y0, bx0, by0 = (t[:1].expand_as(t) for t in (x0, y0, bx0, by0))
    if mutant == "x0 and y0 swapped":
        x0, y0, bx0, by0 = y0, x0, by0, bx0
    xk, yj, bxk, byj = x0[:, :, None], y0[:, None, :], bx0[:, :, None], by0[:, None, :]
    if rule == 0:
        Hn = (1 - eta) * H + eta * xk * yj
        M = H.abs() + eta * xk.abs() * yj.abs()
        b = 5 * U * M + eta * (yj.abs() * bxk + xk.abs() * byj + bxk * byj)
    else:
        Hn = H + eta * xk * yj if mutant == "oja without - h y0" else H + eta * (xk - H * yj) * yj
        M = H.abs() + eta * (xk.abs() + H.abs() * yj.abs()) * yj.abs()
        b = 5 * U * M + eta * (yj.abs() * bxk + (xk.abs() + 2 * H.abs() * yj.abs()) * byj + (bxk + H.abs() * byj) * byj)
    return Hn, b


def _head_tail(p, v, X, bX, mutant):
    """Y and H' of X: {Y, Hn}"""
    N = p.N
    H, w, al = v["H"].double(), v["w"].double(), v["al"].double()
    eta = float(v["eta"])
    MW = w.abs() + al.abs() * H.abs()
    Weff = (w + al) * H if mutant == "Weff as (w + alpha) H" else w + al * H
    if mutant == "last k of the GEMM dropped":
        a = X[..., :-1] @ Weff[:, :-1, :]
    else:
        a = X @ Weff
    ba = (N + 3) * U * (X.abs() @ MW) + bX @ MW
    Y = torch.sigmoid(a)
    an = (a.abs() - ba).clamp_min(0.0)
    bY = torch.sigmoid(an) * torch.sigmoid(-an) * ba + K_SIG * U * Y + TINY     # s' = s(a) s(-a): no 1 - s near 1
    Hn, bH = _trace64(p.rule, eta, H, X[:, 0], Y[:, 0], bX[:, 0], bY[:, 0], mutant)
    return {"Y": (Y, bY), "Hn": (Hn, bH), "a": (a, ba)}


@functools.lru_cache(maxsize=64)
def _head_full(name, bias, mutant):
    r = CASE[name]
    p, v = r.p, values(name)
    if r.entry == "head":
        feat, wo = v["feat"].double(), v["wo"].double()
        MX = feat.abs() @ wo.abs()
        if mutant == "outconv last channel group dropped":
            wo = wo.clone()
            wo[-4:] = 0.0
        X = feat @ wo
        if bias:
            MX = MX + v["bo"].double().abs()
            if mutant != "outconv bias dropped":
                X = X + v["bo"].double()
        c = -(-p.C // (4 * p.L)) + int(math.log2(p.L)) + 6
        bX = c * U * MX
    else:
        X = v["X"].double()
        bX = _zero(X)
    out = _head_tail(p, v, X, bX, mutant)
    if r.entry == "head":
        out["X"] = (X, bX)
    return out


def head_ref(r, f, mutant=None):
    full = _head_full(r.name, bool(f.bias), mutant)
    keep = [k for k in ("X", "Y") if k in full] + (["Hn"] if f.train else [])
    return {k: full[k] for k in keep}


def trace_ref(r, f, mutant=None):
    v = values(r.name)
    Hn = trace_np(v["H"], v["X"][:, 0], v["Y"][:, 0], v["eta"], r.p.rule, mutant)
    return {"Hn": (Hn, _zero(Hn))}


def bwd_ref(r, f, mutant=None, v=None):
    """pu_plastic_bwd (f.P absent) and pu_plastic_bwd_trace in fp64 with the bounds of the module
    docstring; r.entry 'bwd': dY always, no trace path"""
    p, v = r.p, v or values(r.name)
    B, N = p.B, p.N
    X, H, w, al, Y = (v[k].double() for k in ("X", "H", "w", "al", "Y"))
    eta = float(v["eta"])
    trace = r.entry == "bwdt"
    dY = v["dY"].double() if (f.dy or not trace) else _zero(X)
    MdY = dY.abs()
    out = {}
    s = (1 - Y) * Y
    bG = _zero(X)
    dx0 = None
    if trace and f.P:
        Pg = v["P"].double()
        x0, y0 = X[:, 0], Y[:, 0]
        V, ns, nch, _ = trace_plan(p, f)
        Pr = Pg
        if mutant == "one strip's row partial dropped":
            Pr = Pg.clone()
            Pr[:, :, (ns - 1) * 32 * V:] = 0.0
        dx0 = eta * torch.einsum("bkj,bj->bk", Pr, y0)
        Mdx0 = eta * torch.einsum("bkj,bj->bk", Pg.abs(), y0.abs())
        bdx0 = (V + ns + 7) * U * Mdx0
        if p.rule == 0:
            term, Mt = Pg * x0[:, :, None], Pg.abs() * x0.abs()[:, :, None]
            et, Met = Pg * (x0[:, :, None] * y0[:, None, :] - H), Pg.abs() * (x0.abs()[:, :, None] * y0.abs()[:, None, :] + H.abs())
        else:
            two = 1.0 if mutant == "oja dy0 without the factor 2" else 2.0
            term = Pg * (x0[:, :, None] - two * H * y0[:, None, :])
            Mt = Pg.abs() * (x0.abs()[:, :, None] + 2 * H.abs() * y0.abs()[:, None, :])
            et = Pg * y0[:, None, :] * (x0[:, :, None] - H * y0[:, None, :])
            Met = Pg.abs() * y0.abs()[:, None, :] * (x0.abs()[:, :, None] + H.abs() * y0.abs()[:, None, :])
        if mutant == "last chunk's column partial dropped":
            term = term.clone()
            term[:, (nch - 1) * TB_ROWS:, :] = 0.0
        dy0, Mdy0 = eta * term.sum(1), eta * Mt.sum(1)
        bdy0 = (nch + 16) * U * Mdy0
        deta = (et[0] if mutant == "deta of slot 0 only" else et).sum()
        Me = Met.sum()
        out["deta"] = (deta.reshape(1), (4 * U * Me + (B * N * N + 2) * E53 * Me + U * deta.abs()).reshape(1))
        dY = dY.clone()
        if mutant == "dy0 added to every row":
            dY += dy0[:, None, :]
        else:
            dY[:, 0] += dy0
        bG[:, 0] = s[:, 0] * (bdy0 + U * (MdY[:, 0] + Mdy0))
        MdY = MdY.clone()
        MdY[:, 0] += Mdy0
        if mutant == "dx0 omitted":
            dx0 = _zero(dx0)
    G, MG = dY * s, MdY * s
    MW = w.abs() + al.abs() * H.abs()
    if f.dx:
        dX = torch.einsum("bij,bkj->bik", G, w + al * H)
        MdX = torch.einsum("bij,bkj->bik", MG, MW)
        bdX = (N + 6) * U * MdX
        if dx0 is not None:
            bdX[:, 0] += torch.einsum("bj,bkj->bk", bG[:, 0], MW)
        if dx0 is not None:
            dX[:, 0] += dx0
            bdX[:, 0] += bdx0 + U * (MdX[:, 0] + Mdx0)
        out["dx"] = (dX, bdX)
    if f.dw or f.dh:
        T = torch.einsum("bik,bij->bkj", X, G)
        MT = torch.einsum("bik,bij->bkj", X.abs(), MG)
        bT = (N + 4) * U * MT + X.abs()[:, 0, :, None] * bG[:, 0][:, None, :]
        if f.dw:
            nb = B - 1 if mutant == "slot sum without the last slot" else B
            out["dw"] = (T[:nb].sum(0), bT.sum(0) + B * U * MT.sum(0))
            out["dalpha"] = ((T * H)[:nb].sum(0), (bT * H.abs()).sum(0) + (B + 1) * U * (MT * H.abs()).sum(0))
        if f.dh:
            if f.P:
                y2 = (Y[:, 0] ** 2)[:, None, :]
                fac = (1 - eta) if p.rule == 0 else 1 - eta * y2
                dH = v["P"].double() * fac + al * T
                bdH = 6 * U * (v["P"].double().abs() * (1 + eta * y2) + al.abs() * MT) + al.abs() * bT
            else:
                dH, bdH = al * T, 2 * U * al.abs() * MT + al.abs() * bT
            out["dhebb"] = (dH, bdH)
    return out


def bce_fwd_ref(r, f, mutant=None):
    v = values(r.name)
    y, t, n = v["y"].double(), v["t"].double(), r.p.n
    with np.errstate(all="ignore"):
        l1, l0 = torch.log1p(-y), torch.log(y)
    if mutant != "bce without the clamp":
        l1, l0 = l1.clamp_min(-100.0), l0.clamp_min(-100.0)
    loss = ((t - 1) * l1 - t * l0).sum() / n
    M = ((t - 1).abs() * l1.clamp_min(-100.0).abs() + t * l0.clamp_min(-100.0).abs()).sum()
    return {"loss": (loss.reshape(1), (((2 * ULP_LOG + 4) * U + (n + 3) * E53) * M / n + U * loss.abs()).reshape(1))}


def bce_bwd_np(y, t, n, g=None, mutant=None):
    f = np.float32
    y, t = np.asarray(y, dtype=f), np.asarray(t, dtype=f)
    gg = f(1) if g is None else f(np.asarray(g, dtype=f).reshape(-1)[0])
    den = np.maximum(((f(1) - y).astype(f) * y).astype(f), f(1e-12))
    d = ((gg * (y - t).astype(f)).astype(f) / den).astype(f)
    if mutant != "bce dy without / n":
        d = (d / f(n)).astype(f)
    return torch.from_numpy(d)


def bce_bwd_ref(r, f, mutant=None):
    v = values(r.name)
    dy = bce_bwd_np(v["y"].numpy(), v["t"].numpy(), r.p.n, v["g"].numpy() if f.g else None, mutant)
    return {"dy": (dy, _zero(dy))}


ADAM_HP = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_scalars(p, mutant=None):
    """the doubles punet.optim hands to pu_adam_multi"""
    t = p.step - 1 if mutant == "adam bias correction of step t - 1" else p.step
    b1, b2 = ADAM_HP["b1"], ADAM_HP["b2"]
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return b1, b2, ADAM_HP["eps"], p.wd, (ADAM_HP["lr"] / bc1 if bc1 else float("inf")), math.sqrt(bc2)


def adam_np(p, v, mutant=None):
    """adam_one (csrc/adam.hip) in numpy float32, one operation at a time, the scalars cast as the entry casts them"""
    f = np.float32
    b1, b2, eps, wd, ss, bc = adam_scalars(p, mutant)
    omb1, b2f, omb2 = f(1.0 - b1), f(b2), f(1.0 - b2)
    if mutant == "adam beta2 as 1 - beta2":
        b2f, omb2 = f(1.0 - b2), f(b2)
    eps, wdf, ss, bc = f(eps), f(wd), f(ss), f(bc)
    outs = {"p": [], "m": [], "v": []}
    with np.errstate(all="ignore"):
        for pp, g, m, vv in zip(*(v[k] for k in "pgmv")):
            pp, g, m, vv = (t.numpy().astype(f) for t in (pp, g, m, vv))
            if wd != 0.0:
                g = (g + (wdf * pp).astype(f)).astype(f)
            m = (m + (omb1 * (g - m).astype(f)).astype(f)).astype(f)
            vv = ((vv * b2f).astype(f) + ((omb2 * g).astype(f) * g).astype(f)).astype(f)
            den = ((np.sqrt(vv).astype(f) / bc).astype(f) + eps).astype(f)
            pp = (pp + ((-ss) * (m / den).astype(f)).astype(f)).astype(f)
            for k, a in zip("pmv", (pp, m, vv)):
                outs[k].append(torch.from_numpy(a))
    return {k: torch.cat(t) for k, t in outs.items()}


def adam_ref(r, f, mutant=None):
    return {k: (t, _zero(t)) for k, t in adam_np(r.p, values(r.name), mutant).items()}


_REFS = {"head": head_ref, "fwd": head_ref, "trace": trace_ref, "bwd": bwd_ref, "bwdt": bwd_ref, "bce_fwd": bce_fwd_ref,
         "bce_bwd": bce_bwd_ref, "adam": adam_ref}


@functools.lru_cache(maxsize=None)
def _reference(name, form):
    r = CASE[name]
    return _REFS[r.entry](r, FORMS[r.entry][form])


def reference(name, form):
    """{output: (value, bound)} of a (row, form) pair; the 17 MB rows are not kept"""
    if CASE[name].p.big:
        return _reference.__wrapped__(name, form)
    return _reference(name, form)


def mutated(name, form, mutant):
    r = CASE[name]
    return _REFS[r.entry](r, FORMS[r.entry][form], mutant)


def applies(r, f, mutant):
    """whether a mutant changes what the (row, form) pair computes"""
    p, e = r.p, r.entry
    hn = e in ("head", "fwd", "trace") and bool(f.train)
    tr = e == "bwdt" and bool(f.P)
    if mutant == "trace from slot 0's row 0":
        return hn and p.B > 1
    if mutant == "x0 and y0 swapped":
        return hn and p.N > 1
    if mutant == "oja without - h y0":
        return hn and p.rule == 1 and p.data != "zero_h"
    if mutant in ("Weff as (w + alpha) H", "last k of the GEMM dropped"):
        return e in ("head", "fwd")
    if mutant == "outconv last channel group dropped":
        return e == "head"
    if mutant == "outconv bias dropped":
        return e == "head" and bool(f.bias)
    if mutant == "one strip's row partial dropped":
        return tr and bool(f.dx) and p.ns > 1
    if mutant == "last chunk's column partial dropped":
        return tr and p.nch > 1
    if mutant == "deta of slot 0 only":
        return tr and p.B > 1
    if mutant == "dy0 added to every row":
        return tr
    if mutant == "dx0 omitted":
        return tr and bool(f.dx)
    if mutant == "oja dy0 without the factor 2":
        return tr and p.rule == 1 and p.data != "zero_h"
    if mutant == "slot sum without the last slot":
        # one slot is about 1 / B of the sum and the in-order fp32 sum is bounded by B u of it: past
        # B^2 u = 1 (the 16385-slot row) the bound cannot tell
        return e in ("bwd", "bwdt") and bool(f.dw) and p.B > 1 and p.B * p.B * U < 1
    if mutant == "bce without the clamp":
        return e == "bce_fwd" and p.n > 16
    if mutant == "bce dy without / n":
        return e == "bce_bwd" and p.n > 1
    if mutant in ("adam beta2 as 1 - beta2", "adam bias correction of step t - 1"):
        return e == "adam"
    raise KeyError(mutant)


# ------------------------------------------------------------------------------------- device runner
Result = collections.namedtuple("Result", "rc outs intact untouched kept extra ws same")


class _Call:
    """the guarded buffers and device operands of one call"""

    def __init__(self, over):
        self.over, self.guards, self.outs, self.keep, self.ws, self.checked = over, [], {}, [], None, []
        self.mis = set(over.get("mis", ()))
        self.null = set(over.get("null", ()))

    def src(self, name, t, dtype=F32, check=False):
        if name in self.null:
            return None
        d = _dev(t, dtype, 1 if name in self.mis else 0)
        self.keep.append(d)
        if check:
            self.checked.append((d, t.reshape(-1).to(dtype)))
        return d.data_ptr()

    def dst(self, name, numel, dtype=F32, seed=None, written=None):
        g = Guarded(numel, dtype, off=1 if name in self.mis else 0)
        if seed is not None:
            g.inner.copy_(seed.reshape(-1).to(dtype))
        self.guards.append(g)
        self.outs[name] = (g, written)
        return None if name in self.null else g.ptr()

    def call(self, fn, *args):
        self.before = [g.inner.clone() for g in self.guards]
        return fn(*args)

    def workspace(self, need):
        """exactly the queried bytes between the bands, NaN-filled; ws_short / ws_null / ws_mis: the rejected calls"""
        if self.over.get("ws_null"):
            return None, 0
        g = Guarded(max(need // 4, 1), F32, off=1 if self.over.get("ws_mis") else 0)
        self.guards.append(g)
        self.ws = g
        return g.ptr(), need - self.over.get("ws_short", 0)


def _launch(r, f, c, stream):
    L, p, e = _lib.load(), r.p, r.entry
    v = values(r.name)
    if p.mis and e != "adam":
        c.mis.add(p.mis)
    rule = c.over.get("rule", p.rule)
    if e in ("head", "fwd", "trace", "bwd", "bwdt"):
        B, N = c.over.get("B", p.B), c.over.get("N", p.N)
        nn = p.B * p.N * p.N
    if e == "head":
        feat = c.src("feat", v["feat"], _DT[p.dt])
        a = _lib.PlasticHeadArgs(B, N, c.over.get("C", p.C), feat, int(p.dt == "bf16"), c.src("out_w", v["wo"]),
                                 c.src("out_b", v["bo"]) if f.bias else None, c.src("hebb", v["H"], check=True),
                                 c.src("w", v["w"]), c.src("alpha", v["al"]), c.src("eta", v["eta"]), c.dst("X", nn), c.dst("Y", nn),
                                 c.dst("Hn", nn) if f.train else None, rule)
        if c.over.get("alias"):
            a.hebb_out = a.hebb
        return c.call(L.pu_plastic_head_fwd, ctypes.byref(a), stream)
    if e == "fwd":
        x = c.src("x", v["X"])
        if f.alias:
            hebb = hn = c.dst("Hn", nn, seed=v["H"])
        else:
            hebb, hn = c.src("hebb", v["H"], check=True), c.dst("Hn", nn) if f.train else None
        a = _lib.PlasticArgs(B, N, x, hebb, c.src("w", v["w"]), c.src("alpha", v["al"]), c.src("eta", v["eta"]), c.dst("Y", nn),
                             hn, rule)
        return c.call(L.pu_plastic_fwd, ctypes.byref(a), stream)
    if e == "trace":
        return c.call(L.pu_trace_update, c.src("hebb", v["H"], check=True), c.src("x", v["X"]), c.src("y", v["Y"]),
                      c.src("eta", v["eta"]), c.dst("hebb_out", nn), B, N, rule, stream)
    if e == "bwd":
        if f.dwmis:
            c.mis.add("dw")
        a = _lib.PlasticBwdArgs(B, N, c.src("x", v["X"]), c.src("hebb", v["H"], check=True), c.src("w", v["w"]),
                                c.src("alpha", v["al"]), c.src("y", v["Y"]), c.src("dy", v["dY"]),
                                c.dst("dx", nn) if f.dx else None, c.dst("dw", p.N * p.N) if f.dw else None,
                                c.dst("dalpha", p.N * p.N) if f.dw else None)
        ws = c.workspace(L.pu_plastic_bwd_workspace_bytes(p.B, p.N)) if f.dw or c.over.get("ws") else (None, 0)
        return c.call(L.pu_plastic_bwd, ctypes.byref(a), ws[0], ws[1], stream)
    if e == "bwdt":
        a = _lib.PlasticBwdTraceArgs(B, N, rule, c.src("x", v["X"]), c.src("hebb", v["H"], check=True), c.src("w", v["w"]),
                                     c.src("alpha", v["al"]), c.src("eta", v["eta"]), c.src("y", v["Y"]),
                                     c.src("dy", v["dY"]) if f.dy else None, c.src("dhebb_out", v["P"]) if f.P else None,
                                     c.dst("dx", nn) if f.dx else None, c.dst("dw", p.N * p.N) if f.dw else None,
                                     c.dst("dalpha", p.N * p.N) if f.dw else None, c.dst("dhebb", nn) if f.dh else None,
                                     c.dst("deta", 1, written=None if f.P else 0))
        ws = c.workspace(L.pu_plastic_bwd_trace_workspace_bytes(p.B, p.N))
        return c.call(L.pu_plastic_bwd_trace, ctypes.byref(a), ws[0], ws[1], stream)
    if e == "bce_fwd":
        ws = c.workspace(L.pu_bce_workspace_bytes(p.n))
        return c.call(L.pu_bce_fwd, c.src("y", v["y"]), c.src("t", v["t"]), c.over.get("n", p.n), c.dst("loss", 1), ws[0], ws[1], stream)
    if e == "bce_bwd":
        return c.call(L.pu_bce_bwd, c.src("y", v["y"]), c.src("t", v["t"]), c.over.get("n", p.n), c.src("g", v["g"]) if f.g else None,
                      c.dst("dy", p.n), stream)
    if e == "adam":
        ts = []
        for i, n in enumerate(p.numels):
            if n == 0:
                ts.append(_lib.AdamTensor(None, None, None, None, 0))
                continue
            off = lambda k: ["%s%d" % (k, i)] if p.mis == (i, k) else []      # noqa: E731
            c.mis = set(off("p") + off("g") + off("m") + off("v"))
            ts.append(_lib.AdamTensor(c.dst("p%d" % i, n, seed=v["p"][i]), c.src("g%d" % i, v["g"][i], check=True),
                                      c.dst("m%d" % i, n, seed=v["m"][i]), c.dst("v%d" % i, n, seed=v["v"][i]), n))
        bad = c.over.get("adam_bad")              # (tensor, field): a NULL pointer or a negative numel
        if bad:
            setattr(ts[bad[0]], bad[1], -1 if bad[1] == "numel" else None)
        arr = (_lib.AdamTensor * len(ts))(*ts)
        return c.call(L.pu_adam_multi, None if c.over.get("adam_null") else arr, c.over.get("n_tensors", len(ts)),
                      *adam_scalars(p), stream)
    raise KeyError(e)


def run(r, f, **over):
    """One guarded call of row r in form f.  Every destination and the workspace - exactly the bytes
    the query asks for - lie between sentinel bands, pre-filled with the sentinel NaN (Adam's p / m / v
    and an aliased trace: with their values).  Returns the status, the outputs (CPU), whether every
    band survived, whether every destination and the workspace still hold their fill bit for bit,
    whether an entry the call must write kept the sentinel, whether the entries it must not write
    (deta without dhebb_out) kept it, the workspace as the call left it, and whether the checked
    inputs (hebb, Adam's g) are unchanged.  over: what the rejected calls change."""
    from punet import kernels as K
    c = _Call(over)
    rc = _launch(r, f, c, K._stream())
    torch.cuda.synchronize()
    intact = all(g.intact() for g in c.guards)
    untouched = all(torch.equal(g.inner.view(g.word), b.view(g.word)) for g, b in zip(c.guards, c.before))
    outs, kept, extra = {}, False, True
    for name, (g, written) in c.outs.items():
        words = g.inner.view(g.word)
        n = g.numel if written is None else written
        kept = kept or bool((words[:n] == g.sent).any())
        extra = extra and bool((words[n:] == g.sent).all())
        if n:
            outs[name] = g.inner[:n].cpu()
    if r.entry == "adam":
        outs = {k: torch.cat([outs["%s%d" % (k, i)] for i, n in enumerate(r.p.numels) if n]) for k in "pmv"}
    if r.entry == "trace":
        outs = {"Hn": outs["hebb_out"]}
    same = all(torch.equal(d.cpu().view(torch.int16 if d.dtype == BF else torch.int32),
                           t.view(torch.int16 if t.dtype == BF else torch.int32)) for d, t in c.checked)
    return Result(rc, outs, intact, untouched, kept, extra, None if c.ws is None else c.ws.inner.cpu(), same)


def serial_child(out_dir):
    """what the PU_HEAD_PIPE=0 child process of test_head_matrix_gpu.py runs: the N = 128, C = 64 / 96
    fused rows in their training form (the serial kernel under that switch), outputs saved to out_dir"""
    import os
    for i, name in enumerate(PIPE_AB):
        r = CASE[name]
        res = run(r, FORMS["head"]["train"])
        assert res.rc == OK and res.intact and not res.kept
        torch.save(res.outs, os.path.join(out_dir, "%d.pt" % i))


PIPE_AB = ("head f32 B 1 N 128 C 64 hebb", "head f32 B 1 N 128 C 96 hebb", "head bf16 B 1 N 128 C 64 oja",
           "head bf16 B 1 N 128 C 96 oja")
