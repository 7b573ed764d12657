"""Every weight-gradient GEMM kernel the plan can pick against fp64: the case table, the reference,
the derived bounds and the guarded device runner shared by test_wgrad_matrix.py (CPU) and
test_wgrad_matrix_gpu.py.

pu_wgrad / pu_wgrad_bf16 (csrc/wgrad.hip) run in two phases: phase 1, one of about sixty GEMM kernel
instantiations, leaves `splits` partial [Nr][Kcp] tiles in the workspace; phase 2 sums them in fp64
and stores dweight[n][c][kh][kw] (+ dbias).  Phase 2 has its own tests (test_wgrad_reduce_gpu.py,
test_wgrad_rows_reduce_gpu.py); this matrix is about phase 1.  CASES has one row per kernel
instantiation the launcher's switch on the plan's kind can reach (wgrad_launch), steered only by what a call passes (math, the grid, the
channel counts, kernel / stride / pad, alignment) - never by a process-wide switch - with the plan
the library's queries report for it (PLANS) and the kernel instantiation that plan launches
(kernel_of: the launcher's rule, which adds math, FQ, nt, the column form and the instantiated
(C, N) to what the query reports).  FORMS lists bias_mode x accumulate x a dweight view one float
off 16-byte alignment; excluded() holds the rules that leave a (case, form) pair out.

Reference: dweight[n][c][r][s] = sum_m P[m][n] X[pix(m, r, s)][c] (+ the two bias forms of
include/plastic_unet.h) in fp64, as one matrix product per tap over the zero-padded source; for the
bf16 entry and the bf16 rows of math 2 on the bf16-rounded operands widened exactly.  Each reference
comes with its magnitude A: the same sums over |P| and |X|.

Bounds (derived, not measured):  |got - ref| <= c * 2^-24 * A  for every entry, u = 2^-24.
L is the most pixels one split covers, from the plan the query reports (split_len: the largest
stage multiple that still gives the reported split count, and never more than M).
  fp32 chains   (math 0, the register-staged, stem, pointwise and small-channel kernels)
                a slab entry is an fp32 sum of at most L products in some order: each product is
                rounded once (not at all inside an fma) and then passes at most L - 1 additions, so
                any order is within L u A_split of the exact sum.  The fp64 sum over the splits
                (< 2^-42 A) and the second-order terms (L u <= 2^-13 of the first) take less than
                one u A, the final fp32 store one more:            c = L + 2
  math 1        each product is six exact bf16 x bf16 products accumulated in fp32 (6 L additions
                per entry), over operands whose pieces sum to at most (1 + 2^-7)^2 < 1.02 of
                |P| |X|; the dropped terms are < 2^-23 = 2 u relative (include/plastic_unet.h):
                                                                   c = 1.02 * 6 L + 2 + 2
  Winograd      dW = G^T [sum_tiles (A e A^T) (.) (B^T d B)] G: A is that expression with the
                absolute values of G, A, B, e and d.  Both input transforms are two passes of one
                addition (4 roundings on a product), the transformed operands split exactly, the
                16 position GEMMs are math-1 chains over at most Lt tiles per split, the output
                transform is two passes of two additions (4) on the fp32 partial, then the store
                and the slack as above:              c = 4 + 1.02 * 6 Lt + 2 + 4 + 2
  bf16 entry    products of bf16 values are exact in fp32, so only the L - 1 additions count,
                then the slack and the store:                      c = L + 1
  bias          dbias is a plain fp32 sum over the same pixels in every kernel (mode 2: the fp64
                finisher adds the taps): the row's c with L in pixels, against sum |P| or sum |X|.
  accumulate    one fp32 addition per entry: torch.equal(accumulated, seed + plain) in fp32.
No constant here is fitted to a kernel's output; test_wgrad_matrix.py checks on the CPU that the
bounds are sharp enough to reject a dropped pixel row, a pixel counted twice, a tap shifted by a
column, a dropped src1 channel and an omitted bias.
"""
import collections
import ctypes
import functools
import re

import torch

from punet import _lib
from conv_epilogue import SENT32, Guarded, _dev    # the shared sentinel idiom

BF = torch.bfloat16
U = 2.0 ** -24

# --------------------------------------------------------------------------------------------- forms
# (bias_mode, accumulate, dweight one float off 16-byte alignment: a view into a flat gradient)
Form = collections.namedtuple("Form", "bias acc view")
FORMS = {
    "conv": collections.OrderedDict([
        ("b1", Form(1, 0, 0)), ("b0", Form(0, 0, 0)), ("b1+acc", Form(1, 1, 0)), ("b0+acc", Form(0, 1, 0)),
        ("b1+view", Form(1, 0, 1)), ("b0+view+acc", Form(0, 1, 1)),
    ]),
    "convT": collections.OrderedDict([
        ("b2", Form(2, 0, 0)), ("b0", Form(0, 0, 0)), ("b2+acc", Form(2, 1, 0)), ("b0+acc", Form(0, 1, 0)),
        ("b2+view", Form(2, 0, 1)), ("b0+view+acc", Form(0, 1, 1)),
    ]),
}

Case = collections.namedtuple("Case", "name entry kernel B H W c0 c1 n op math")

WR_WIDE_MAX = 16384           # csrc/wgrad.hip: slabs of at most this many entries take the wide reducer


def reducer(c, bias, view):
    """csrc/wgrad.hip plan_reducer: the phase-2 kernel a call takes"""
    bn, bk, kind, _, _ = PLANS[c.name][bias]
    C = c.c0 + c.c1
    k = geometry(c)[2]
    if c.entry == "f32" and kind == 5 and bn == 128:
        return "cols vec" if not view else "cols scalar"
    Nr, Kc = c.n + (bias == 2), k * k * C + (bias == 1)
    direct = c.entry == "f32" and kind in (2, 4, 6)
    wino = c.entry == "f32" and kind == 5
    if (direct or (not wino and Nr * ((Kc + 3) // 4 * 4) <= WR_WIDE_MAX)) and bias != 2:
        return "wide"
    return "transposed" if bias != 2 and k * k <= 9 and C % 4 == 0 and not view else "quad"


def bias_excluded(c, bias):
    """the rules that leave a bias_mode out of a row"""
    if c.kernel.startswith("wgrad_stem_kernel") and bias != 1:
        return "the stem kernel takes bias_mode 1 only (stem_wgrad_ok); bias 0 is the small kernel's C = 1 row"
    if c.kernel.startswith("wgrad_small_kernel<1,") and c.n >= 8 and bias == 1:
        return "C = 1, n >= 8 with bias_mode 1 is the stem kernel's call"
    if c.op.startswith("T3") and bias == 2:
        return "bias_mode 2 is the ConvT bias only when every source pixel is read once (k == stride)"
    return None


def excluded(c, f):
    """The explicit rules that leave a (case, form) pair out."""
    why = bias_excluded(c, f.bias)
    if why:
        return why
    if f.view and reducer(c, f.bias, 0) == reducer(c, f.bias, 1):
        return "the reducer has one path whatever dweight's alignment"
    return None


# ---------------------------------------------------------------------------------------- case table
def stem(n, bf16rows=False):
    return "wgrad_stem_kernel<%d,%d>" % (n, bf16rows)


def pw(C, N):
    return "wgrad_pw_kernel<%d,%d>" % (C, N)


def small(C, N):
    return "wgrad_small_kernel<%d,%d>" % (C, N)


_WAVES = {(64, 64): (2, 2), (64, 128): (2, 2), (32, 128): (1, 4), (64, 192): (2, 2), (128, 128): (2, 2),
          (128, 256): (2, 2), (64, 256): (1, 4)}


def dma(bn, bk, math, fq=False):
    """wgrad_dma_kernel<BN, BK, WN, WK, NBUF 3, X6, NW 4, FQ>; FQ is an X6 form"""
    return "wgrad_dma_kernel<%d,%d,%d,%d,3,%d,4,%d>" % ((bn, bk) + _WAVES[bn, bk] + (math == 1, math == 1 and fq))


def reg(bn, bk):
    return "wgrad_kernel<%d,%d,%d,%d,0>" % ((bn, bk) + _WAVES[bn, bk])


WINO, COLS, BF16 = "wgrad_wino_x6_kernel", "wgrad_wino_cols_x6_kernel", "wgrad_bf16_kernel"


def halo(nt):
    return "wgrad_halo_x6_kernel<%d>" % nt


def halo16(nt):
    return "wgrad_halo_bf16_kernel<%d>" % nt


def _case(name, kernel, shape, op="conv", math=1, entry="f32"):
    """shape = (B, H, W, c0, c1, n): the grid of `rows` (conv: dZ, and the source's grid; ConvT: the
    low-res input x, the source dU on the 2x grid), the two sources' channels and the GEMM rows n."""
    return Case(name, entry, kernel, *shape, op, math)


def _b16(name, kernel, shape, op="conv"):
    return _case(name, kernel, shape, op, 0, "bf16")


G = (2, 9, 13)        # the default grid: 234 pixels, a partial last 16-pixel stage
G3 = (3, 9, 13)       # 351 pixels: two splits of 176, the last one partial

CASES = [
    # ---- single-channel stem (bias_mode 1 only); 17 x 65: more than one 16 x 64 tile in each direction
    _case("stem 1->8", stem(8), G + (1, 0, 8)),
    _case("stem 1->16 2x2 tiles m0", stem(16), (1, 17, 65, 1, 0, 16), math=0),
    _case("stem 1->32", stem(32), G + (1, 0, 32)),
    _case("stem 1->64 m0", stem(64), G + (1, 0, 64), math=0),
    _case("stem bf16 rows 1->8", stem(8, True), G + (1, 0, 8), math=2),
    _case("stem bf16 rows 1->16", stem(16, True), G + (1, 0, 16), math=2),
    _case("stem bf16 rows 1->32", stem(32, True), G + (1, 0, 32), math=2),
    _case("stem bf16 rows 1->64 2x2 tiles", stem(64, True), (1, 17, 65, 1, 0, 64), math=2),
    # ---- pointwise 1x1
    _case("pw 3->4", pw(3, 4), G3 + (3, 0, 4), "conv1"),
    _case("pw 3->8", pw(3, 8), G3 + (3, 0, 8), "conv1"),
    _case("pw 3->16", pw(3, 16), G + (3, 0, 16), "conv1"),
    _case("pw 4->4", pw(4, 4), G + (4, 0, 4), "conv1"),
    _case("pw 4->8", pw(4, 8), G3 + (4, 0, 8), "conv1", math=0),
    _case("pw 4->16", pw(4, 16), G3 + (4, 0, 16), "conv1"),
    # ---- small-channel direct: C through one source and through two
    _case("small 1->4", small(1, 4), G + (1, 0, 4)),
    _case("small 1->8", small(1, 8), G + (1, 0, 8)),
    _case("small 1->16 2x2 tiles", small(1, 16), (2, 17, 33, 1, 0, 16)),
    _case("small 4->4", small(4, 4), G + (4, 0, 4)),
    _case("small 4->8", small(4, 8), G + (4, 0, 8), math=0),
    _case("small 4->16 2x2 tiles", small(4, 16), (2, 17, 33, 4, 0, 16)),
    _case("small 8->4", small(8, 4), G + (8, 0, 4)),
    _case("small 4+4->8", small(8, 8), G + (4, 4, 8)),
    _case("small 8->16", small(8, 16), G + (8, 0, 16)),
    _case("small 8+4->4", small(12, 4), G + (8, 4, 4)),
    _case("small 12->8", small(12, 8), G + (12, 0, 8)),
    _case("small 8+4->16", small(12, 16), G + (8, 4, 16)),
    _case("small 16->4", small(16, 4), G + (16, 0, 4)),
    _case("small 8+8->8", small(16, 8), G + (8, 8, 8)),
    _case("small 12+4->16 2x2 tiles", small(16, 16), (1, 17, 33, 12, 4, 16)),
    # ---- Winograd-domain kernel (even grid, 64-multiples, math 1)
    _case("wino one tile", WINO, (1, 2, 2, 64, 0, 64)),
    _case("wino 64+64->128, 30 tiles", WINO, (2, 6, 10, 64, 64, 128)),
    _case("wino 128->64, 3 splits", WINO, (3, 8, 8, 128, 0, 64)),
    # ---- its column form: the gate shape (512 tiles, whole 128-channel blocks)
    _case("wino cols gate 128->128", COLS, (2, 32, 32, 128, 0, 128)),
    _case("wino cols 128+128->128", COLS, (2, 32, 32, 128, 128, 128)),
    # ---- halo kernels: odd height with W a multiple of 16
    _case("halo<1> 64->64", halo(1), (1, 5, 16, 64, 0, 64)),
    _case("halo<1> 64+64->192", halo(1), (1, 3, 16, 64, 64, 192)),
    _case("halo<1> 256->192 ring wrap", halo(1), (1, 21, 128, 256, 0, 192)),     # 42 splits of 4 stages
    _case("halo<2> 64+64->128", halo(2), (1, 3, 16, 64, 64, 128)),
    _case("halo<2> 128->256", halo(2), (1, 5, 16, 128, 0, 256)),
    # ---- direct-to-LDS GEMM tiles: math 0, math 1 with FQ, math 1 without (ConvT, out_w < 4)
    _case("dma 64x64 m0", dma(64, 64, 0), G3 + (4, 0, 32), math=0),
    _case("dma 64x64 fq", dma(64, 64, 1, True), G3 + (4, 0, 32)),
    _case("dma 64x64 out_w 3", dma(64, 64, 1), (2, 9, 3, 4, 0, 32)),
    _case("dma 64x64 ConvT2", dma(64, 64, 1), (2, 5, 7, 16, 0, 40), "T2"),
    _case("dma 64x64 ConvT2 m0", dma(64, 64, 0), (2, 5, 7, 16, 0, 40), "T2", math=0),
    _case("dma 64x128 m0", dma(64, 128, 0), G3 + (48, 0, 64), math=0),
    _case("dma 64x128 fq 32+16", dma(64, 128, 1, True), G3 + (32, 16, 64)),
    _case("dma 64x128 ConvT3 crop 0", dma(64, 128, 1), (2, 5, 7, 48, 0, 64), "T3c0"),
    _case("dma 32x128 fq", dma(32, 128, 1, True), G3 + (20, 0, 32)),
    _case("dma 32x128 ConvT3 crop 1", dma(32, 128, 1), (2, 5, 7, 20, 0, 32), "T3c1"),
    _case("dma 64x192 m0", dma(64, 192, 0), G3 + (64, 0, 64), math=0),
    _case("dma 64x192 m0 20->32", dma(64, 192, 0), G3 + (20, 0, 32), math=0),
    _case("dma 64x192 fq", dma(64, 192, 1, True), G3 + (64, 0, 64)),
    _case("dma 64x192 ConvT2 144->64", dma(64, 192, 1), (2, 5, 7, 144, 0, 64), "T2"),
    _case("dma 128x128 m0", dma(128, 128, 0), G3 + (36, 0, 72), math=0),
    _case("dma 128x128 fq", dma(128, 128, 1, True), G3 + (36, 0, 72)),
    _case("dma 128x128 out_w 3", dma(128, 128, 1), (2, 9, 3, 36, 0, 72)),
    _case("dma 128x128 ConvT3 crop 1", dma(128, 128, 1), (2, 5, 7, 36, 0, 72), "T3c1"),
    _case("dma 128x256 fq 256->128", dma(128, 256, 1, True), G + (256, 0, 128)),
    _case("dma 128x256 fq 128+128->136", dma(128, 256, 1, True), G + (128, 128, 136)),
    _case("dma 128x256 ConvT2 64->128", dma(128, 256, 1), (2, 5, 5, 64, 0, 128), "T2"),
    # ---- register-staged scalar kernel: a channel count that is no multiple of 4
    _case("reg 64x64 3->16", reg(64, 64), G3 + (3, 0, 16)),
    _case("reg 64x64 4+3->16", reg(64, 64), G + (4, 3, 16)),
    _case("reg 64x64 ConvT2 6->64", reg(64, 64), (2, 5, 7, 6, 0, 64), "T2"),          # bias 2: Nr = n + 1
    _case("reg 64x256 10->32", reg(64, 256), G3 + (10, 0, 32)),
    _case("reg 64x256 8+6->40 m0", reg(64, 256), G + (8, 6, 40), math=0),
    _case("reg 64x256 ConvT3 crop 1", reg(64, 256), (2, 5, 7, 10, 0, 64), "T3c1"),
    _case("reg 128x128 10->72", reg(128, 128), G3 + (10, 0, 72)),
    # ---- bf16 entry
    _b16("bf16 40->72, 2 splits", BF16, (5, 9, 13, 40, 0, 72)),
    _b16("bf16 32+24->40", BF16, G + (32, 24, 40)),
    _b16("bf16 ConvT2 32->64", BF16, (2, 5, 7, 32, 0, 64), "T2"),
    _b16("bf16 ConvT3 crop 1", BF16, (2, 5, 7, 32, 0, 64), "T3c1"),
    _b16("bf16 halo<1> 64->64", halo16(1), (1, 4, 16, 64, 0, 64)),
    _b16("bf16 halo<1> 256->192 ring wrap", halo16(1), (1, 21, 128, 256, 0, 192)),
    _b16("bf16 halo<2> 64+64->128", halo16(2), (1, 4, 16, 64, 64, 128)),
    _b16("bf16 halo<2> 128->256 odd height", halo16(2), (1, 5, 16, 128, 0, 256)),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# the phase-2 kernels, which test_wgrad_reduce_gpu.py and test_wgrad_rows_reduce_gpu.py own
REDUCERS = {"wgrad_sum_splits4_kernel", "wgrad_finish4_kernel<d>", "wgrad_finish4_kernel<f>", "wgrad_finish_t_kernel<d>",
            "wgrad_finish_t_kernel<f>", "wgrad_finish_cols_kernel", "wgrad_reduce_wide_kernel"}

# name -> bias_mode -> (bn, bk, kind, splits, workspace bytes) as pu_wgrad_tile / pu_wgrad_bf16_tile
# and the workspace queries report them (kind: the loader kind, or the bf16 entry's halo flag)
PLANS = {
    "stem 1->8": {1: (8, 9, 4, 2, 768)},
    "stem 1->16 2x2 tiles m0": {1: (16, 9, 4, 4, 3072)},
    "stem 1->32": {1: (32, 9, 4, 2, 3072)},
    "stem 1->64 m0": {1: (64, 9, 4, 2, 6144)},
    "stem bf16 rows 1->8": {1: (8, 9, 4, 2, 768)},
    "stem bf16 rows 1->16": {1: (16, 9, 4, 2, 1536)},
    "stem bf16 rows 1->32": {1: (32, 9, 4, 2, 3072)},
    "stem bf16 rows 1->64 2x2 tiles": {1: (64, 9, 4, 4, 12288)},
    "pw 3->4": {1: (4, 3, 6, 2, 256), 0: (4, 3, 6, 2, 256)},
    "pw 3->8": {1: (8, 3, 6, 2, 256), 0: (8, 3, 6, 2, 256)},
    "pw 3->16": {1: (16, 3, 6, 1, 256), 0: (16, 3, 6, 1, 256)},
    "pw 4->4": {1: (4, 4, 6, 1, 256), 0: (4, 4, 6, 1, 256)},
    "pw 4->8": {1: (8, 4, 6, 2, 512), 0: (8, 4, 6, 2, 256)},
    "pw 4->16": {1: (16, 4, 6, 2, 1024), 0: (16, 4, 6, 2, 512)},
    "small 1->4": {1: (4, 9, 2, 2, 512), 0: (4, 9, 2, 2, 512)},
    "small 1->8": {0: (8, 9, 2, 2, 768)},
    "small 1->16 2x2 tiles": {0: (16, 9, 2, 8, 6144)},
    "small 4->4": {1: (4, 36, 2, 2, 1280), 0: (4, 36, 2, 2, 1280)},
    "small 4->8": {1: (8, 36, 2, 2, 2560), 0: (8, 36, 2, 2, 2304)},
    "small 4->16 2x2 tiles": {1: (16, 36, 2, 8, 20480), 0: (16, 36, 2, 8, 18432)},
    "small 8->4": {1: (4, 72, 2, 2, 2560), 0: (4, 72, 2, 2, 2304)},
    "small 4+4->8": {1: (8, 72, 2, 2, 4864), 0: (8, 72, 2, 2, 4608)},
    "small 8->16": {1: (16, 72, 2, 2, 9728), 0: (16, 72, 2, 2, 9216)},
    "small 8+4->4": {1: (4, 108, 2, 2, 3584), 0: (4, 108, 2, 2, 3584)},
    "small 12->8": {1: (8, 108, 2, 2, 7168), 0: (8, 108, 2, 2, 6912)},
    "small 8+4->16": {1: (16, 108, 2, 2, 14336), 0: (16, 108, 2, 2, 13824)},
    "small 16->4": {1: (4, 144, 2, 2, 4864), 0: (4, 144, 2, 2, 4608)},
    "small 8+8->8": {1: (8, 144, 2, 2, 9472), 0: (8, 144, 2, 2, 9216)},
    "small 12+4->16 2x2 tiles": {1: (16, 144, 2, 4, 37888), 0: (16, 144, 2, 4, 36864)},
    "wino one tile": {1: (64, 576, 5, 1, 148480), 0: (64, 576, 5, 1, 147456)},
    "wino 64+64->128, 30 tiles": {1: (64, 576, 5, 2, 1183744), 0: (64, 576, 5, 2, 1179648)},
    "wino 128->64, 3 splits": {1: (64, 576, 5, 3, 887808), 0: (64, 576, 5, 3, 884736)},
    "wino cols gate 128->128": {1: (128, 384, 5, 128, 25427968), 0: (128, 384, 5, 128, 25165824)},
    "wino cols 128+128->128": {1: (128, 384, 5, 128, 50593792), 0: (128, 384, 5, 128, 50331648)},
    "halo<1> 64->64": {1: (64, 576, 3, 5, 742400), 0: (64, 576, 3, 5, 737280)},
    "halo<1> 64+64->192": {1: (64, 576, 3, 3, 2663424), 0: (64, 576, 3, 3, 2654208)},
    "halo<1> 256->192 ring wrap": {1: (64, 576, 3, 42, 74446848), 0: (64, 576, 3, 42, 74317824)},
    "halo<2> 64+64->128": {1: (128, 576, 3, 3, 1775616), 0: (128, 576, 3, 3, 1769472)},
    "halo<2> 128->256": {1: (128, 576, 3, 5, 5918720), 0: (128, 576, 3, 5, 5898240)},
    "dma 64x64 m0": {1: (64, 64, 1, 2, 10240), 0: (64, 64, 1, 2, 9216)},
    "dma 64x64 fq": {1: (64, 64, 1, 2, 10240), 0: (64, 64, 1, 2, 9216)},
    "dma 64x64 out_w 3": {1: (64, 64, 1, 1, 5120), 0: (64, 64, 1, 1, 4608)},
    "dma 64x64 ConvT2": {2: (64, 64, 1, 1, 10496), 0: (64, 64, 1, 1, 10240)},
    "dma 64x64 ConvT2 m0": {2: (64, 64, 1, 1, 10496), 0: (64, 64, 1, 1, 10240)},
    "dma 64x128 m0": {1: (64, 128, 1, 2, 223232), 0: (64, 128, 1, 2, 221184)},
    "dma 64x128 fq 32+16": {1: (64, 128, 1, 2, 223232), 0: (64, 128, 1, 2, 221184)},
    "dma 64x128 ConvT3 crop 0": {0: (64, 128, 1, 1, 110592)},
    "dma 32x128 fq": {1: (32, 128, 1, 2, 47104), 0: (32, 128, 1, 2, 46080)},
    "dma 32x128 ConvT3 crop 1": {0: (32, 128, 1, 1, 23040)},
    "dma 64x192 m0": {1: (64, 192, 1, 2, 296960), 0: (64, 192, 1, 2, 294912)},
    "dma 64x192 m0 20->32": {1: (64, 192, 1, 2, 47104), 0: (64, 192, 1, 2, 46080)},
    "dma 64x192 fq": {1: (64, 192, 1, 2, 296960), 0: (64, 192, 1, 2, 294912)},
    "dma 64x192 ConvT2 144->64": {2: (64, 192, 1, 1, 149760), 0: (64, 192, 1, 1, 147456)},
    "dma 128x128 m0": {1: (128, 128, 1, 2, 188928), 0: (128, 128, 1, 2, 186624)},
    "dma 128x128 fq": {1: (128, 128, 1, 2, 188928), 0: (128, 128, 1, 2, 186624)},
    "dma 128x128 out_w 3": {1: (128, 128, 1, 1, 94464), 0: (128, 128, 1, 1, 93440)},
    "dma 128x128 ConvT3 crop 1": {0: (128, 128, 1, 1, 93440)},
    "dma 128x256 fq 256->128": {1: (128, 256, 1, 1, 1181696), 0: (128, 256, 1, 1, 1179648)},
    "dma 128x256 fq 128+128->136": {1: (128, 256, 1, 1, 1255680), 0: (128, 256, 1, 1, 1253376)},
    "dma 128x256 ConvT2 64->128": {2: (128, 256, 1, 1, 132096), 0: (128, 256, 1, 1, 131072)},
    "reg 64x64 3->16": {1: (64, 64, 0, 2, 3584), 0: (64, 64, 0, 2, 3584)},
    "reg 64x64 4+3->16": {1: (64, 64, 0, 1, 4096), 0: (64, 64, 0, 1, 4096)},
    "reg 64x64 ConvT2 6->64": {2: (64, 64, 0, 1, 6400), 0: (64, 64, 0, 1, 6144)},
    "reg 64x256 10->32": {1: (64, 256, 0, 2, 23552), 0: (64, 256, 0, 2, 23552)},
    "reg 64x256 8+6->40 m0": {1: (64, 256, 0, 1, 20480), 0: (64, 256, 0, 1, 20480)},
    "reg 64x256 ConvT3 crop 1": {0: (64, 256, 0, 1, 23552)},
    "reg 128x128 10->72": {1: (128, 128, 0, 2, 52992), 0: (128, 128, 0, 2, 52992)},
    "bf16 40->72, 2 splits": {1: (128, 128, 0, 2, 209664), 0: (128, 128, 0, 2, 207360)},
    "bf16 32+24->40": {1: (128, 128, 0, 1, 81408), 0: (128, 128, 0, 1, 80640)},
    "bf16 ConvT2 32->64": {2: (128, 128, 0, 1, 33280), 0: (128, 128, 0, 1, 32768)},
    "bf16 ConvT3 crop 1": {0: (128, 128, 0, 1, 73728)},
    "bf16 halo<1> 64->64": {1: (64, 576, 1, 4, 593920), 0: (64, 576, 1, 4, 589824)},
    "bf16 halo<1> 256->192 ring wrap": {1: (64, 576, 1, 42, 74446848), 0: (64, 576, 1, 42, 74317824)},
    "bf16 halo<2> 64+64->128": {1: (128, 576, 1, 4, 2367488), 0: (128, 576, 1, 4, 2359296)},
    "bf16 halo<2> 128->256 odd height": {1: (128, 576, 1, 5, 5918720), 0: (128, 576, 1, 5, 5898240)},
}


def layout(c):
    return "conv" if c.op.startswith("conv") else "convT"


Case.layout = property(layout)


def geometry(c):
    """(in_h, in_w), (out_h, out_w), k, stride, pad of the call"""
    H, W = c.H, c.W
    return {"conv": ((H, W), (H, W), 3, 1, 1),
            "conv1": ((H, W), (H, W), 1, 1, 0),
            "T2": ((2 * H, 2 * W), (H, W), 2, 2, 0),                      # ConvTranspose2d 2x2 / s2
            "T3c0": ((2 * H + 1, 2 * W + 1), (H, W), 3, 2, 0),            # ConvTranspose2d 3x3 / s2, crop 0
            "T3c1": ((2 * H, 2 * W), (H, W), 3, 2, 1)}[c.op]              # ... cropped by one row and column


def pixels(c):
    (_, _), (oh, ow), _, _, _ = geometry(c)
    return c.B * oh * ow


def fq(c):
    """the planner's rule for the FQ forms of the math-1 kernels"""
    (ih, iw), (oh, ow), _, st, _ = geometry(c)
    return st == 1 and (ih, iw) == (oh, ow) and ow >= 4


def kernel_of(c, bias):
    """The instantiation the launcher (csrc/wgrad.hip wgrad_launch) starts for the row's pinned plan."""
    bn, bk, kind, _, _ = PLANS[c.name][bias]
    C = c.c0 + c.c1
    if c.entry == "bf16":
        return halo16(bn // 64) if kind else BF16
    if kind == 4:
        return stem(c.n, c.math == 2)
    if kind == 6:
        return pw(C, c.n)
    if kind == 2:
        return small(C, c.n)
    if kind == 5:
        return COLS if bn == 128 else WINO
    if kind == 3:
        return halo(bn // 64)
    if kind == 1:
        return dma(bn, bk, c.math, fq(c))
    return reg(bn, bk)


def forms(c):
    return [(nm, f) for nm, f in FORMS[c.layout].items() if excluded(c, f) is None]


PAIR_COUNT = 325            # pinned: test_wgrad_matrix.py derives it from the table and the exclusion rules


def pairs():
    """every (case name, form name) the GPU file runs"""
    return [(c.name, nm) for c in CASES for nm, _ in forms(c)]


def demangle(sym):
    """'wgrad_dma_kernel<64,128,2,2,3,1,4,1>' from the Itanium name of a pu:: kernel template over
    ints, bools and float / double / __bf16 ('b') (None: not a pu:: function)"""
    m = re.match(r"_ZN2pu(\d+)", sym)
    if not m:
        return None
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while not rest.startswith("E"):
        m = re.match(r"L[ib](\d+)E|([df])|DF16(b)", rest)
        assert m, sym
        args.append(m.group(1) or m.group(2) or m.group(3))
        rest = rest[m.end():]
    return "%s<%s>" % (name, ",".join(args))


# ------------------------------------------------------------------------------------ plans and bounds
STANDIN = 0x10000


def wgrad_args(c, f, ptr, **over):
    """pu_wgrad_args of case c in form f; ptr: name -> device address.  over: fields replaced after
    that (the rejected calls)."""
    (ih, iw), (oh, ow), k, st, pad = geometry(c)
    a = _lib.WgradArgs(c.B, ih, iw, oh, ow, k, k, st, pad, ptr["rows"], c.n, ptr["src0"], c.c0,
                       ptr["src1"] if c.c1 else None, c.c1, f.bias, ptr["dweight"], ptr["dbias"] if f.bias else None,
                       f.acc, c.math)
    for key, val in over.items():
        setattr(a, key, val)
    return a


def standin_ptrs(f):
    names = ("rows", "src0", "src1", "dweight", "dbias")
    return {nm: STANDIN * (i + 1) + (4 if nm == "dweight" and f.view else 0) for i, nm in enumerate(names)}


def _fns(entry):
    L = _lib.load()
    if entry == "f32":
        return L.pu_wgrad, L.pu_wgrad_phase, L.pu_wgrad_workspace_bytes, L.pu_wgrad_tile
    return L.pu_wgrad_bf16, L.pu_wgrad_bf16_phase, L.pu_wgrad_bf16_workspace_bytes, L.pu_wgrad_bf16_tile


def plan_of(c, a):
    """(bn, bk, kind, splits, workspace bytes) the library reports for args a; an int status when the
    query refuses them"""
    _, _, ws_fn, tile_fn = _fns(c.entry)
    v = [ctypes.c_int(0) for _ in range(4)]
    rc = tile_fn(ctypes.byref(a), *(ctypes.byref(x) for x in v))
    if rc != 0:
        return rc
    return tuple(x.value for x in v) + (ws_fn(ctypes.byref(a)),)


def _most(total, stage, splits):
    """the largest multiple of `stage` that cuts `total` into `splits` ranges, at most total"""
    if splits <= 1:
        return total
    return min(total, (total - 1) // (splits - 1) // stage * stage)


def split_len(c, bias):
    """(L, Lt): the most pixels, and for the Winograd kernels the most 2x2 tiles, one split covers"""
    bn, bk, kind, splits, _ = PLANS[c.name][bias]
    M = pixels(c)
    (_, _), (oh, ow), _, _, _ = geometry(c)
    if c.entry == "bf16":
        return _most(M, 16 if kind else 32, splits), None
    if kind in (2, 4):                   # grid-stride over 16 x 32 (stem: 16 x 64) pixel tiles
        th, tw = 16, 64 if kind == 4 else 32
        ntiles = c.B * -(-oh // th) * -(-ow // tw)
        return min(M, -(-ntiles // splits) * min(th, oh) * min(tw, ow)), None
    if kind == 5:
        tiles = M // 4
        Lt = _most(tiles, 16, splits // 4 if bn == 128 else splits)
        return min(M, 4 * Lt), Lt
    return _most(M, 1 if kind == 6 else 16, splits), None


def bound_c(c, bias):
    """c of |got - ref| <= c * 2^-24 * A (module docstring)"""
    L, Lt = split_len(c, bias)
    kind = PLANS[c.name][bias][2]
    if c.entry == "bf16":
        return L + 1
    if kind == 5:
        return 4 + 1.02 * 6 * Lt + 2 + 4 + 2
    if c.math == 1 and kind in (1, 3):
        return 1.02 * 6 * L + 2 + 2
    return L + 2


def bias_c(c, bias):
    """the same for dbias: a plain sum over the split's pixels in the row's arithmetic"""
    L, _ = split_len(c, bias)
    kind = PLANS[c.name][bias][2]
    if c.entry == "bf16":
        return L + 1
    return 1.02 * 6 * L + 4 if (c.math == 1 and kind in (1, 3, 5)) else L + 2


def ratio(got, ref, mag, cc):
    """max over entries of |got - ref| / (cc * 2^-24 * mag); an entry with mag == 0 must be exact; a
    NaN fails"""
    err = (got.double().reshape(-1) - ref.reshape(-1)).abs().nan_to_num(nan=float("inf"))
    bound = cc * U * mag.reshape(-1)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r


# ------------------------------------------------------------------------------ values and reference
def _round(t, bf16):
    return t.to(BF).float() if bf16 else t


@functools.lru_cache(maxsize=None)
def values(name):
    """The operands of a case (CPU fp32 tensors, NHWC; the bf16 entry's, and the rows of math 2,
    rounded to bf16 first) and the seeds of the accumulate forms."""
    c = CASE[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    (ih, iw), (oh, ow), k, _, _ = geometry(c)
    C = c.c0 + c.c1
    b16 = c.entry == "bf16"
    v = dict(rows=_round(torch.randn(c.B, oh, ow, c.n, generator=g), b16 or c.math == 2),
             src0=_round(torch.randn(c.B, ih, iw, c.c0, generator=g), b16),
             src1=_round(torch.randn(c.B, ih, iw, c.c1, generator=g), b16) if c.c1 else None)
    v["seed_w"] = torch.randn(c.n * C * k * k, generator=g)
    v["seed_b"] = {1: torch.randn(c.n, generator=g), 2: torch.randn(C, generator=g)}
    return v


MUTANTS = ("drop_row", "double_pixel", "shift_tap", "drop_src1", "no_bias")
Ref = collections.namedtuple("Ref", "dw db mag_w mag_b")


def _grads(c, rows, src, bias, mutant=None, at=0):
    """dweight [n][C][k][k] and dbias of the call in fp64 from NHWC fp64 operands: one matrix product
    per tap over the zero-padded source.  mutant: one of MUTANTS (at: the pixel counted twice)."""
    (ih, iw), (oh, ow), k, st, pad = geometry(c)
    B, n, C = c.B, c.n, c.c0 + c.c1
    M = B * oh * ow
    P = rows.reshape(M, n)
    if mutant == "drop_row":
        P = P.clone()
        P[M - ow:] = 0
    elif mutant == "double_pixel":
        P = P.clone()
        P[at] *= 2
    elif mutant == "drop_src1":
        src = src.clone()
        src[..., C - 1] = 0
    hp = max(ih + pad, (oh - 1) * st + k) + 1          # one spare column and row for the shifted tap
    wp = max(iw + pad, (ow - 1) * st + k) + 1
    xp = torch.zeros(B, hp, wp, C, dtype=torch.float64)
    xp[:, pad:pad + ih, pad:pad + iw] = src
    dw = torch.empty(n, C, k, k, dtype=torch.float64)
    colsum = torch.zeros(C, dtype=torch.float64)
    for r in range(k):
        for s in range(k):
            s2 = s + 1 if (mutant == "shift_tap" and (r, s) == (k // 2, k // 2)) else s
            X = xp[:, r:r + st * (oh - 1) + 1:st, s2:s2 + st * (ow - 1) + 1:st].reshape(M, C)
            dw[:, :, r, s] = P.t() @ X
            colsum += X.sum(0)
    db = None if bias == 0 or mutant == "no_bias" else P.sum(0) if bias == 1 else colsum
    if bias and db is None:
        db = torch.zeros(n if bias == 1 else C, dtype=torch.float64)
    return dw, db


_A = torch.tensor([[1., 0.], [1., 1.], [1., -1.], [0., -1.]], dtype=torch.float64)                                # A    4 x 2
_BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]], dtype=torch.float64)  # B^T  4 x 4
_G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)                     # G    4 x 3


def _wino(c, rows, src, A, BT, Gm):
    """G^T [sum_tiles (A e A^T) (.) (B^T d B)] G per (n, c) over the 2x2 output tiles of a 3x3 / s1 / p1
    layer on an even grid (e: the tile of rows, d: its 4x4 source window)"""
    B, H, W, n, C = c.B, c.H, c.W, c.n, c.c0 + c.c1
    th, tw = H // 2, W // 2
    e = rows.reshape(B, th, 2, tw, 2, n).permute(0, 1, 3, 5, 2, 4).reshape(-1, n, 2, 2)
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = src
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2).reshape(-1, C, 4, 4)          # [B, th, tw, C, 4, 4]
    E = torch.einsum("ia,tnab,jb->tnij", A, e, A)
    D = torch.einsum("ia,tcab,jb->tcij", BT, d, BT)
    S = torch.einsum("tnij,tcij->ncij", E, D)
    return torch.einsum("ir,ncij,js->ncrs", Gm, S, Gm)


def _wino_signed(c, rows, src):
    """the Winograd-domain expression itself: equals the direct gradient"""
    return _wino(c, rows, src, _A, _BT, _G)


def _wino_magnitude(c, rows, src):
    """the same with the absolute values of G, A, B, e and d: the running-error magnitude of the
    Winograd-domain weight gradient"""
    return _wino(c, rows.abs(), src.abs(), _A.abs(), _BT.abs(), _G.abs())


def operands64(c):
    v = values(c.name)
    src = v["src0"] if v["src1"] is None else torch.cat([v["src0"], v["src1"]], 3)
    return v["rows"].double(), src.double()


@functools.lru_cache(maxsize=None)
def reference(name, bias):
    """Ref(dweight flat [n][c][kh][kw], dbias, their magnitudes) of a row in fp64; computed once"""
    c = CASE[name]
    rows, src = operands64(c)
    dw, db = _grads(c, rows, src, bias)
    mw, mb = _grads(c, rows.abs(), src.abs(), bias)
    if PLANS[name][bias][2] == 5 and c.entry == "f32":
        mw = _wino_magnitude(c, rows, src)
    return Ref(dw.reshape(-1), db, mw.reshape(-1), mb)


def mutated(name, bias, mutant):
    """the reference with one of MUTANTS applied (double_pixel: the first pixel of the second split,
    or the last pixel of a plan with one split)"""
    c = CASE[name]
    rows, src = operands64(c)
    L, _ = split_len(c, bias)
    dw, db = _grads(c, rows, src, bias, mutant, at=min(L, pixels(c) - 1))
    return dw.reshape(-1), db


# ------------------------------------------------------------------------------------- device runner
@functools.lru_cache(maxsize=None)
def device_inputs(name, rows_off=0, src0_off=0):
    """rows and sources of a case on the device, 16-byte aligned or the given floats past that"""
    c = CASE[name]
    v = values(name)
    dt = BF if c.entry == "bf16" else torch.float32
    return dict(rows=_dev(v["rows"], BF if c.math == 2 else dt, rows_off), src0=_dev(v["src0"], dt, src0_off),
                src1=_dev(v["src1"], dt) if c.c1 else None)


Result = collections.namedtuple("Result", "rc dw db plan intact untouched")


def run(c, f, phases=False, ws_short=0, ws_null=False, dbias_null=False, rows_off=0, src0_off=0, **over):
    """One guarded call of case c in form f (phases: phase 1 then phase 2 instead of the single
    call).  dweight, dbias and the workspace - exactly the bytes the query asks for, pre-filled with
    the sentinel NaN - each lie between sentinel bands; the outputs start as NaN, or as the seeds
    under accumulate.  Returns the status, dweight and dbias (CPU fp32), the plan the query reports
    for these very arguments, whether every band survived and whether outputs and workspace still
    hold their fill bit for bit.  The remaining keywords shape the rejected calls."""
    from punet import kernels as K
    single, phase_fn, _, _ = _fns(c.entry)
    v = values(c.name)
    d = device_inputs(c.name, rows_off, src0_off)
    (_, _), (_, _), k, _, _ = geometry(c)
    C = c.c0 + c.c1
    gw = Guarded(c.n * C * k * k, torch.float32, off=f.view)
    if f.acc:
        gw.inner.copy_(v["seed_w"])
    else:
        gw.inner.fill_(float("nan"))
    gb = None
    if f.bias:
        gb = Guarded(c.n if f.bias == 1 else C, torch.float32)
        if f.acc:
            gb.inner.copy_(v["seed_b"][f.bias])
        else:
            gb.inner.fill_(float("nan"))
    ptr = dict(rows=d["rows"].data_ptr(), src0=d["src0"].data_ptr(), src1=d["src1"].data_ptr() if c.c1 else None,
               dweight=gw.ptr(), dbias=gb.ptr() if gb is not None else None)
    # the workspace is sized by the well-formed call; the plan reported is that of the call made
    need = plan_of(c, wgrad_args(c, f, dict(standin_ptrs(f))))[4]
    assert need > 0 and need % 4 == 0, need
    a = wgrad_args(c, f, ptr, **over)
    if dbias_null:
        a.dbias = None
    plan = plan_of(c, a)
    gs = Guarded(need // 4, torch.float32)
    gs.inner.view(torch.int32).fill_(SENT32)
    guards = [g for g in (gw, gb, gs) if g is not None]
    before = [g.inner.clone() for g in guards]
    ws = (None, 0) if ws_null else (gs.ptr(), need - ws_short)
    stream = K._stream()
    if phases:
        rc = phase_fn(ctypes.byref(a), ws[0], ws[1], 1, stream)
        if rc == 0:
            rc = phase_fn(ctypes.byref(a), ws[0], ws[1], 2, stream)
    else:
        rc = single(ctypes.byref(a), ws[0], ws[1], stream)
    torch.cuda.synchronize()
    intact = all(g.intact() for g in guards)
    untouched = all(torch.equal(g.inner.view(torch.int32), b.view(torch.int32)) for g, b in zip(guards, before))
    return Result(rc, gw.inner.cpu(), gb.inner.cpu() if gb is not None else None, plan, intact, untouched)


@functools.lru_cache(maxsize=None)
def plain(name, bias, view):
    """the plain (accumulate = 0) result of a row, run once: what the accumulate forms add to a seed"""
    return run(CASE[name], Form(bias, 0, view))
