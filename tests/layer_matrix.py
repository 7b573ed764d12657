"""Every layer kernel outside the convolutions against fp64, launch branch by launch branch: the case
table, the references, the derived bounds and the guarded device runner shared by
test_layer_matrix.py (CPU) and test_layer_matrix_gpu.py.

csrc/norm.hip (BatchNorm forward / backward, the bilinear 2x upsample) and csrc/elementwise.hip (the
max-pools, the 1x1 head conv, the Dropout2d scale, the column sum, AddCoords, the layout change, the
bf16 converts) compile to 42 kernel instantiations besides the weight packers.  CASES has one row or
more per launch branch of their entry points, steered only by what a call passes (shape, dtype, NULL
operands, a pointer four bytes off 16-byte alignment); kernel_of applies the launcher's own rule to
the row and names the instantiations the call launches; FORMS lists, per entry point, the operand
forms every row of it is run in; excluded() holds the rules that leave a (row, form) pair out.

References are written plainly in fp64 (BatchNorm per slot with two-pass variance; the upsample with
ATen's float32 source index and weights - they are part of the specification - and the interpolation
and its transpose in fp64; the max-pool as ATen's row-major scan  val > max || isnan(val)).  Each
reference returns, per output, the value and the absolute bound of every entry.

Bounds (derived, not measured), u = 2^-24, e = 2^-53, M the sum of the absolute values of the terms
of the entry:
  bit-exact      max-pool forward / backward (an output is one of the inputs, or one correctly
                 rounded fp32 product with the Dropout2d scale; bf16 rows hold bf16 values),
                 nchw_to_nhwc, channel_scale and the outconv dx (one correctly rounded product; bf16:
                 that product rounded once more to bf16), both converts (round to nearest even),
                 AddCoords against the same float32 expressions evaluated op by op in numpy (the file
                 disables contraction):                                             bound 0
  accumulate     fp32: one addition, torch.equal(accumulated, seed + plain); the bf16 max-pool
                 against bf16(float(seed) + plain):                                 bound 0
  fp64 sums      (BatchNorm mean, dgamma / dbeta, the column sum) n terms summed in fp64 in some
                 order, stored once in fp32:                              u |ref| + (n + 2) e M
  BN rstd        var = s1 / n - mu^2 in fp64 carries dvar <= (2n + 6) e (E x^2 + mu^2);
                 d rstd / d var = -rstd^3 / 2; one fp32 store:            u rstd + rstd^3 dvar / 2
  BN running     B in-order updates, each computed in fp64 and rounded to fp32, the last stored:
                 (B + 1) u M with M the same recurrence over absolute values (+ the statistic's
                 own fp64 error, weighted by the momentum)
  bn_apply       y = v a + (beta - mu a) [+ resid], a = rstd gamma: five operations as written, six
                 with the residual, one unit of slack for the second-order terms, on
                 M = (|v| + |mu|) |a| + |beta| + |resid|; plus the fp32 rounding (and fp64 error)
                 of mean and rstd, which the bounds above already hold:
                 (6 [+ 1]) u M + (bound_rstd / rstd) (|v| + |mu|) |a| + bound_mean |a|
  bn_bwd_apply   dz = (g - gm - (z - mean) k) rstd gamma [+ add]: six operations, seven with add,
                 the fp32 rounding of the two coefficients gm and k, one unit of slack, on
                 M = (|g| + |gm| + |z - mean| |k|) rstd |gamma| + |add|:    (9 [+ 1]) u M
                 (+ the (n + 2) e error of the two fp64 sums); a masked entry is exactly 0
  upsample fwd   l0h (l0w x00 + l1w x01) + l1h (l0w x10 + l1w x11): every term passes a product, a
                 sum, a product and a sum, plus one unit of slack:                  5 u M
  upsample bwd   dx = sum over the T outputs that read the pixel of (wh ww) dy: the weight product,
                 the term's product, at most T - 1 additions; wh and ww are each l0 + l1 in fp32
                 where both taps of an output coincide (one rounding per axis); slack:
                 (T + 4) u M with T counted per entry (at most 16)
  exact coords   the same upsample against rational coordinates: the float32 coordinate scale * o
                 carries two roundings of a value below max(h, w) and 1 - l1 one more, so a weight
                 is off by at most (2 max(h, w) + 1) u and the two weights of an axis by twice that:
                 the bound above + 4 (2 max(h, w) + 1) u (max |x| of the image and channel) per axis;
                 backward: four outputs per axis read a pixel and the other axis's weights onto it
                 sum to at most 3, 24 taken as 32 (2 max(h, w) + 1) u max |dy| per axis
  outconv fwd    16 lanes, each an fma chain over its channels (4 per 64-channel round, then one
                 addition per round), four shuffle additions, the bias, slack:
                 (ceil(C / 64) + 10) u M; the scalar kernel: C products in one chain, the bias,
                 slack: (C + 2) u M;  M = sum |x| |w| + |b|
  outconv dw/db  a thread sums its n_t = ceil(rows / (blocks P)) pixels in fp32 (one rounding per
                 product, n_t - 1 additions), the block adds its P pixel groups in fp32 (P - 1), the
                 partials are summed in fp64 and stored once; slack:
                 (n_t + P + 1) u M with blocks from the launcher's rule, pinned per row
No constant here is fitted to a kernel's output; test_layer_matrix.py checks on the CPU that every
bound rejects the mutants of MUTANTS on every row they apply to.
"""
import collections
import functools

import numpy as np
import torch

from punet import _lib
from conv_epilogue import Guarded, _dev    # the shared sentinel idiom

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U, E53 = 2.0 ** -24, 2.0 ** -53
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))      # the values the kernels see, widened
OK, INVALID, WORKSPACE = 0, -1, -4

Row = collections.namedtuple("Row", "name entry kernels p")


class P(dict):
    """a row's parameters, readable as attributes; absent ones are None"""
    def __getattr__(self, k):
        return self.get(k)

    def __hash__(self):
        return hash(tuple(sorted(self.items())))


def _r(name, entry, kernels, **p):
    return Row(name, entry, frozenset([kernels] if isinstance(kernels, str) else kernels), P(p))


# ------------------------------------------------------------------------------------------- forms
def _forms(*items):
    return collections.OrderedDict((nm, P(opts)) for nm, opts in items)


FORMS = {
    # affine: gamma and beta passed; running: the two running buffers passed
    "bn_fwd": _forms(("relu", dict(relu=1, affine=1, running=1)), ("plain", dict(affine=1, running=1)),
                     ("resid+relu", dict(relu=1, affine=1, running=1, resid=1)), ("no affine", dict(relu=1, running=1)),
                     ("no running", dict(relu=1, affine=1))),
    "bn_eval": _forms(("relu", dict(relu=1, affine=1, running=1)), ("resid", dict(affine=1, running=1, resid=1)),
                      ("no affine", dict(running=1))),
    "bn_bwd": _forms(("plain", dict(affine=1, dparams=1)), ("add", dict(affine=1, dparams=1, add=1)),
                     ("mask", dict(affine=1, dparams=1, mask=1)), ("add+mask", dict(affine=1, dparams=1, add=1, mask=1)),
                     ("no gamma", dict(dparams=1)), ("no dgamma", dict(affine=1, mask=1))),
    "up_fwd": _forms(("plain", {})),
    "up_bwd": _forms(("plain", {}), ("mask", dict(mask=1))),
    "pool_fwd": _forms(("plain", {}), ("scaled", dict(scaled=1))),
    "pool_bwd": _forms(("plain", {}), ("relu", dict(relu=1)), ("acc", dict(acc=1)), ("relu+acc", dict(relu=1, acc=1)),
                       ("scaled", dict(scaled=1)), ("scaled+relu+acc", dict(scaled=1, relu=1, acc=1))),
    "oc_fwd": _forms(("bias", dict(bias=1)), ("no bias", {})),
    "oc_bwd": _forms(("relu", dict(relu=1)), ("no relu", {})),
    "scale": _forms(("plain", {})),
    "colsum": _forms(("plain", {}), ("acc", dict(acc=1))),
    "coords": _forms(("plain", {})),
    "nchw": _forms(("plain", {})),
    "cvt": _forms(("plain", {})),
}


def excluded(r, f):
    """The explicit rules that leave a (row, form) pair out."""
    if f.scaled and r.p.dt == "bf16":
        return "the Dropout2d scale is an fp32-entry operand"
    if r.p.mis == "scale" and not f.scaled:
        return "the misaligned operand is absent"
    return None


# ---------------------------------------------------------------------------------------- case table
BN_TRAIN = {"bn_partial_kernel<0>", "bn_stats_finalize_kernel", "bn_apply_kernel"}
BN_EVAL = {"bn_eval_stats_kernel", "bn_apply_kernel"}
BN_BWD = {"bn_partial_kernel<1>", "bn_bwd_finalize_kernel", "bn_bwd_apply_kernel"}
OC_BLOCKS = 1024                 # csrc/elementwise.hip
OCN_U = 4


def _bn(name, B, hw, C, S, ws, data="normal", bwd=True):
    rows = [_r("bn fwd " + name, "bn_fwd", BN_TRAIN, B=B, hw=hw, C=C, S=S, ws=ws, data=data)]
    if bwd:
        rows.append(_r("bn bwd " + name, "bn_bwd", BN_BWD, B=B, hw=hw, C=C, S=S, ws=ws, data=data))
    return rows


def _pool(name, dt, shape, fwd, bwd, **kw):
    B, H, W, C = shape
    t = {"f32": "f", "bf16": "b"}[dt]
    out = []
    if fwd:
        out.append(_r("pool fwd %s %s" % (dt, name), "pool_fwd", fwd % t if "%s" in fwd else fwd, dt=dt, B=B, H=H, W=W, C=C,
                      **kw))
    if bwd:
        out.append(_r("pool bwd %s %s" % (dt, name), "pool_bwd", bwd % t if "%s" in bwd else bwd, dt=dt, B=B, H=H, W=W, C=C,
                      **kw))
    return out


FW, F1, F0 = "maxpool_fwd_win_kernel<%s>", "maxpool_fwd_kernel<1,%s>", "maxpool_fwd_kernel<0,f>"
BW, B1, B0 = "maxpool_bwd_win_kernel<%s>", "maxpool_bwd_kernel<1,%s>", "maxpool_bwd_kernel<0,f>"


def _ocf(name, dt, rows, C, kernel, blocks, **kw):
    return _r("outconv fwd %s %s" % (dt, name), "oc_fwd", kernel, dt=dt, rows=rows, C=C, blocks=blocks, **kw)


def _ocb(name, dt, rows, C, blocks):
    t = {"f32": "f", "bf16": "b"}[dt]
    L = C // 4
    k = "outconv_bwd_narrow_kernel<%s,%d>" % (t, L) if L in (2, 4, 8) else "outconv_bwd_kernel<%s>" % t
    return _r("outconv bwd %s %s" % (dt, name), "oc_bwd", {k, "column_sum_kernel"}, dt=dt, rows=rows, C=C, blocks=blocks,
              ws=OC_BLOCKS * (C + 1) * 4)


COLSUM_V = {"colsum_partial_kernel<1>", "colsum_final_kernel"}
COLSUM_S = {"colsum_partial_kernel<0>", "colsum_final_kernel"}

CASES = (
    # ---- BatchNorm (B, hw, C; the split count S and the workspace are pinned to the query)
    _bn("C 12: idle tail threads", 2, 35, 12, 1, 576)
    + _bn("C 24", 2, 35, 24, 1, 1152)
    + _bn("C 48", 3, 35, 48, 1, 3456)
    + _bn("C 96: partial second block", 2, 35, 96, 1, 4608)
    + _bn("S 64 cap", 1, 16384, 4, 64, 4128)
    + _bn("S 3, hw 1000 % 3", 1, 1000, 8, 3, 448)
    + _bn("hw 1", 2, 1, 4, 1, 192)
    + _bn("constant channel, mean 1000 x spread", 2, 35, 8, 1, 384, data="edge")
    + [_r("bn eval C 12", "bn_eval", BN_EVAL, B=2, hw=35, C=12, data="normal"),
       _r("bn eval C 96", "bn_eval", BN_EVAL, B=3, hw=35, C=96, data="normal")]
    # ---- bilinear 2x upsample (B, h, w, C)
    + [_r("up %s %s" % (d, nm), "up_" + d, "upsample_bilinear2x_%s_kernel" % d, B=s[0], h=s[1], w=s[2], C=s[3])
       for nm, s in (("3x5", (2, 3, 5, 4)), ("1x1", (2, 1, 1, 4)), ("h 1", (1, 1, 5, 4)), ("w 1", (1, 5, 1, 8)),
                     ("h 2", (2, 2, 3, 8)), ("9x13, 4 blocks", (1, 9, 13, 8))) for d in ("fwd", "bwd")]
    # ---- max-pool (B, H, W, C)
    + _pool("even", "f32", (2, 6, 10, 8), FW, BW)
    + _pool("odd H", "f32", (2, 7, 10, 8), F1, B1)
    + _pool("odd W", "f32", (1, 6, 9, 4), F1, B1)
    + _pool("C 6", "f32", (2, 6, 10, 6), F0, B0)
    + _pool("C 5 odd", "f32", (1, 7, 9, 5), F0, B0)
    + _pool("x + 4 B", "f32", (2, 6, 10, 8), F0, B1, mis="x")
    + _pool("y + 4 B", "f32", (2, 6, 10, 8), F0, None, mis="y")
    + _pool("dy + 4 B", "f32", (2, 6, 10, 8), None, B1, mis="dy")
    + _pool("dx + 4 B", "f32", (2, 6, 10, 8), None, B1, mis="dx")
    + _pool("odd H, scale + 4 B", "f32", (2, 7, 10, 8), F0, None, mis="scale")
    + _pool("NaN and -inf windows", "f32", (1, 4, 6, 4), FW, BW, special=1)
    + _pool("NaN and -inf windows, odd", "f32", (1, 5, 7, 4), F1, B1, special=1)
    + _pool("NaN and -inf windows, C 3", "f32", (1, 4, 6, 3), F0, B0, special=1)
    + _pool("even", "bf16", (2, 6, 10, 8), FW, BW)
    + _pool("C 12", "bf16", (2, 6, 10, 12), F1, B1)
    + _pool("odd", "bf16", (2, 7, 9, 8), F1, B1)
    + _pool("NaN and -inf windows", "bf16", (1, 4, 6, 8), FW, BW, special=1)
    + _pool("NaN and -inf windows, odd", "bf16", (1, 5, 7, 8), F1, B1, special=1)
    # ---- head conv forward (rows, C; blocks of 16 pixel groups, or of 256 pixels on the scalar kernel)
    + [_ocf("C 64", "f32", 37, 64, "outconv_fwd_kernel<f>", 3),
       _ocf("C 96", "f32", 37, 96, "outconv_fwd_kernel<f>", 3),
       _ocf("C 8, 2 blocks", "f32", 300, 8, "outconv_fwd_kernel<f>", 19),
       _ocf("C 6", "f32", 300, 6, "outconv_fwd_scalar_kernel", 2),
       _ocf("C 8, x + 4 B", "f32", 300, 8, "outconv_fwd_scalar_kernel", 2, mis="x"),
       _ocf("C 8, w + 4 B", "f32", 300, 8, "outconv_fwd_scalar_kernel", 2, mis="w"),
       _ocf("C 64", "bf16", 37, 64, "outconv_fwd_kernel<b>", 3),
       _ocf("C 96", "bf16", 37, 96, "outconv_fwd_kernel<b>", 3),
       _ocf("C 8", "bf16", 300, 8, "outconv_fwd_kernel<b>", 19)]
    # ---- head conv backward (rows, C; pinned block count)
    + [_ocb("C 8", "f32", 300, 8, 3), _ocb("C 16", "f32", 300, 16, 5), _ocb("C 32", "f32", 300, 32, 10),
       _ocb("C 8 second trip of the unroll", "f32", 4 * 1024 * 128 + 77, 8, 1024),
       _ocb("C 16 one sweep and a tail", "f32", 1024 * 64 + 37, 16, 1024),
       _ocb("C 32 second trip of the unroll", "f32", 4 * 1024 * 32 + 21, 32, 1024),
       _ocb("C 64", "f32", 37, 64, 3), _ocb("C 96", "f32", 37, 96, 3),
       _ocb("C 4 past the block cap", "f32", 16384 + 21, 4, 1024),
       _ocb("C 8", "bf16", 300, 8, 3), _ocb("C 16", "bf16", 300, 16, 5), _ocb("C 32", "bf16", 300, 32, 10),
       _ocb("C 8 one sweep and a tail", "bf16", 1024 * 128 + 37, 8, 1024),
       _ocb("C 16 one sweep and a tail", "bf16", 1024 * 64 + 37, 16, 1024),
       _ocb("C 32 one sweep and a tail", "bf16", 1024 * 32 + 37, 32, 1024),
       _ocb("C 64", "bf16", 37, 64, 3), _ocb("C 96", "bf16", 37, 96, 3), _ocb("C 12", "bf16", 300, 12, 19)]
    # ---- Dropout2d scale (B, hw, C)
    + [_r("scale quads", "scale", "channel_scale4_kernel", B=2, hw=35, C=8),
       _r("scale batch 65536", "scale", "channel_scale_kernel<1>", B=65536, hw=1, C=4),
       _r("scale C 6", "scale", "channel_scale_kernel<0>", B=2, hw=35, C=6),
       _r("scale x + 4 B", "scale", "channel_scale_kernel<0>", B=2, hw=35, C=8, mis="x")]
    # ---- column sum (rows, cols; pinned partial blocks and workspace)
    + [_r("colsum 300x8", "colsum", COLSUM_V, rows=300, cols=8, nb=1, ws=64),
       _r("colsum 5000x8: four rows in flight", "colsum", COLSUM_V, rows=5000, cols=8, nb=5, ws=320),
       _r("colsum 300x12: idle lane", "colsum", COLSUM_V, rows=300, cols=12, nb=1, ws=96),
       _r("colsum 40x1028: second chunk", "colsum", COLSUM_V, rows=40, cols=1028, nb=1, ws=8224),
       _r("colsum 40x258: second chunk", "colsum", COLSUM_S, rows=40, cols=258, nb=1, ws=2064),
       _r("colsum 300x8, x + 4 B", "colsum", COLSUM_S, rows=300, cols=8, nb=1, ws=64, mis="x"),
       _r("colsum block cap", "colsum", COLSUM_S, rows=(1 << 20) + 5, cols=1, nb=1024, ws=8192)]
    # ---- AddCoords (B, c, h, w, with_r), the layout change, the converts
    + [_r("coords c 1 + r", "coords", "add_coords4_kernel", B=2, c=1, h=5, w=7, with_r=1),
       _r("coords c 1 + r, out + 4 B", "coords", "add_coords_kernel", B=2, c=1, h=5, w=7, with_r=1, mis="out"),
       _r("coords c 1", "coords", "add_coords_kernel", B=2, c=1, h=5, w=7, with_r=0),
       _r("coords c 3 + r", "coords", "add_coords_kernel", B=2, c=3, h=7, w=5, with_r=1),
       _r("nchw 3x5x7", "nchw", "nchw_to_nhwc_kernel", B=2, c=3, h=5, w=7),
       _r("f32 to bf16", "cvt", "f32_to_bf16_kernel", n=4004, to="bf16"),
       _r("bf16 to f32", "cvt", "bf16_to_f32_kernel", n=4004, to="f32")]
)
CASE = {r.name: r for r in CASES}
assert len(CASE) == len(CASES)

# kernels of the two files that the conv matrices exercise on every call
PACKERS = {"pack_weight_kernel<f>", "pack_weight_kernel<b>", "pack_multi_kernel"}
SOURCES = ("norm.hip", "elementwise.hip")
PAIR_COUNT = 303          # pinned: test_layer_matrix.py derives it from the table and the exclusion rules


def forms(r):
    return [(nm, f) for nm, f in FORMS[r.entry].items() if excluded(r, f) is None]


def pairs():
    return [(r.name, nm) for r in CASES for nm, _ in forms(r)]


# ------------------------------------------------------------------------------- the launchers' rules
def bn_plan(B, hw, C):
    """csrc/norm.hip bn_plan: (CC, S)"""
    CC = min(C, 64)
    cblocks = -(-C // CC)
    return CC, max(1, min(1024 // (cblocks * B), hw // 256, 64))


def oc_fwd_blocks(r):
    p = r.p
    vec = p.C % 4 == 0 and (p.dt == "bf16" or p.mis not in ("x", "w"))
    return min(-(-p.rows // 16), 8192) if vec else min(-(-p.rows // 256), 8192)


def oc_bwd_blocks(r):
    L = r.p.C // 4
    per = 256 // L if L in (2, 4, 8) else 16
    return min(-(-r.p.rows // per), OC_BLOCKS)


def colsum_blocks(rows):
    return max(1, min(1024, -(-rows // 1024)))


def kernel_of(r):
    """The instantiations the row's call launches: the launcher's rule applied to its arguments."""
    p, e = r.p, r.entry
    mis = p.mis
    if e == "bn_fwd":
        return frozenset(BN_TRAIN)
    if e == "bn_eval":
        return frozenset(BN_EVAL)
    if e == "bn_bwd":
        return frozenset(BN_BWD)
    if e in ("up_fwd", "up_bwd"):
        return frozenset(["upsample_bilinear2x_%s_kernel" % e[3:]])
    if e == "pool_fwd":
        even = p.H % 2 == 0 and p.W % 2 == 0
        if p.dt == "bf16":
            return frozenset([FW % "b" if p.C % 8 == 0 and even else F1 % "b"])
        vec = p.C % 4 == 0 and mis not in ("x", "y")
        if vec and even:
            return frozenset([FW % "f"])
        return frozenset([F1 % "f" if vec and mis != "scale" else F0])
    if e == "pool_bwd":
        even = p.H % 2 == 0 and p.W % 2 == 0
        if p.dt == "bf16":
            return frozenset([BW % "b" if p.C % 8 == 0 and even else B1 % "b"])
        vec = p.C % 4 == 0
        if vec and even and mis not in ("x", "dy", "dx"):
            return frozenset([BW % "f"])
        return frozenset([B1 % "f" if vec else B0])
    if e == "oc_fwd":
        if p.dt == "bf16":
            return frozenset(["outconv_fwd_kernel<b>"])
        return frozenset(["outconv_fwd_kernel<f>" if p.C % 4 == 0 and mis not in ("x", "w") else "outconv_fwd_scalar_kernel"])
    if e == "oc_bwd":
        t, L = {"f32": "f", "bf16": "b"}[p.dt], p.C // 4
        k = "outconv_bwd_narrow_kernel<%s,%d>" % (t, L) if L in (2, 4, 8) else "outconv_bwd_kernel<%s>" % t
        return frozenset([k, "column_sum_kernel"])
    if e == "scale":
        vec = p.C % 4 == 0 and mis is None
        if vec and p.hw * (p.C // 4) < (1 << 31) and p.B < 65536:
            return frozenset(["channel_scale4_kernel"])
        return frozenset(["channel_scale_kernel<%d>" % vec])
    if e == "colsum":
        return frozenset(COLSUM_V if p.cols % 4 == 0 and mis is None else COLSUM_S)
    if e == "coords":
        four = p.c == 1 and p.with_r and mis is None and p.B * p.h * p.w < (1 << 31)
        return frozenset(["add_coords4_kernel" if four else "add_coords_kernel"])
    if e == "nchw":
        return frozenset(["nchw_to_nhwc_kernel"])
    if e == "cvt":
        return frozenset(["f32_to_bf16_kernel" if p.to == "bf16" else "bf16_to_f32_kernel"])
    raise KeyError(e)


def plan_of(r):
    """what the library's queries report for the row (no GPU): BatchNorm (S, workspace bytes), outconv
    backward and the column sum (blocks by the launcher's rule, workspace bytes)"""
    L, p = _lib.load(), r.p
    if r.entry in ("bn_fwd", "bn_bwd"):
        ws = L.pu_bn_workspace_bytes(p.B, p.hw, p.C)
        return (ws - 8 * p.B * p.C) // (16 * p.B * p.C), ws
    if r.entry == "oc_bwd":
        return oc_bwd_blocks(r), L.pu_outconv_workspace_bytes(p.rows, p.C)
    if r.entry == "colsum":
        return colsum_blocks(p.rows), L.pu_column_sum_workspace_bytes(p.rows, p.cols)
    if r.entry == "oc_fwd":
        return oc_fwd_blocks(r), 0
    return None


def pinned(r):
    p = r.p
    if r.entry in ("bn_fwd", "bn_bwd"):
        return p.S, p.ws
    if r.entry == "oc_bwd":
        return p.blocks, p.ws
    if r.entry == "colsum":
        return p.nb, p.ws
    if r.entry == "oc_fwd":
        return p.blocks, 0
    return None


# --------------------------------------------------------------------------------------------- values
def _bf(t):
    return t.to(BF).float()


def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def values(name, p=None, entry=None):
    """The operands of a row (CPU fp32 tensors; bf16 rows hold bf16 values) and the seeds of its
    accumulate forms.  Rows of the same shape share nothing: the generator is seeded by the name."""
    if p is None:
        r = CASE[name]
        p, entry = r.p, r.entry
    g = _gen(name)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    v = {}
    if entry in ("bn_fwd", "bn_eval", "bn_bwd"):
        B, hw, C = p.B, p.hw, p.C
        z = rn(B, hw, C) * (0.5 + torch.rand(B, 1, C, generator=g)) + rn(B, 1, C)       # per-slot mean and spread
        if p.data == "edge":
            z[0, :, 0], z[1, :, 0] = 0.1, 0.3                 # a constant channel: var = 0 (and the var < 0 clamp)
            z[:, :, 1] = rn(B, hw) + 1000.0                   # mean 1000 x spread: E x^2 - mu^2 cancels six digits
        v.update(z=z, gamma=0.5 + torch.rand(C, generator=g), beta=rn(C), resid=rn(B, hw, C), rm=rn(C),
                 rv=0.5 + torch.rand(C, generator=g), g=rn(B, hw, C), add=rn(B, hw, C))
        m = rn(B, hw, C)
        m[torch.rand(B, hw, C, generator=g) < 0.25] = 0.0     # exact zeros: > 0, != 0 and >= 0 differ
        v["mask"] = m
    elif entry in ("up_fwd", "up_bwd"):
        v.update(x=rn(p.B, p.h, p.w, p.C), dy=rn(p.B, 2 * p.h, 2 * p.w, p.C))
        m = rn(p.B, p.h, p.w, p.C)
        m[torch.rand(p.B, p.h, p.w, p.C, generator=g) < 0.25] = 0.0
        v["mask"] = m
    elif entry in ("pool_fwd", "pool_bwd"):
        B, H, W, C = p.B, p.H, p.W, p.C
        # small integers: ties within a window, zeros under the ReLU mask, exact in bf16
        x = torch.randint(-2, 3, (B, H, W, C), generator=g).float()
        x[0, 0:2, 0:2, 0] = torch.tensor([[1., 1.], [0., 1.]])         # a three-way tie
        x[0, 0:2, 2:4, 0] = torch.tensor([[-1., 0.], [-2., 0.]])       # the maximum is 0, twice
        if p.special:
            nan, ninf = float("nan"), float("-inf")
            x[0, 0:2, 0:2, :] = nan                                     # a window of NaNs: the last one wins
            x[0, 0:2, 2:4, :] = ninf                                    # all -inf: the first element keeps the index
            x[0, 2:4, 0:2, 1] = torch.tensor([[2., nan], [3., 1.]])     # a NaN, then larger values: the NaN stays
            x[0, 2:4, 2:4, 1] = torch.tensor([[ninf, ninf], [ninf, -1.]])
            x[0, 2:4, 4:6, 0] = torch.tensor([[0., -1.], [-1., -2.]])   # the maximum is 0
            x[0, 2:4, 4:6, 2] = torch.tensor([[1., 1.], [0., 1.]])      # a three-way tie
        dy = rn(B, H // 2, W // 2, C)
        seed = rn(B, H, W, C)
        if p.dt == "bf16":
            dy, seed = _bf(dy), _bf(seed)
        scale = 2.0 * (torch.rand(B, C, generator=g) < 0.6).float() + 0.5 * torch.rand(B, C, generator=g)
        v.update(x=x, dy=dy, seed=seed, scale=scale)
    elif entry in ("oc_fwd", "oc_bwd"):
        rows, C = p.rows, p.C
        x = rn(rows, C)
        x[torch.rand(rows, C, generator=g) < 0.125] = 0.0
        dy = rn(rows) * (2.0 ** -4 if rows > 100000 else 1.0)
        # a last row that no bound can hide (the mutant that drops it)
        x[-1] = torch.where(x[-1] >= 0, 1.0 + x[-1].abs(), -1.0 - x[-1].abs())
        dy[-1] = 4.0
        if p.dt == "bf16":
            x = _bf(x)
        v.update(x=x, w=rn(C), b=rn(1) + 2.0, dy=dy)
    elif entry == "scale":
        v.update(x=rn(p.B, p.hw, p.C), scale=2.0 * (torch.rand(p.B, p.C, generator=g) < 0.5).float()
                 + torch.rand(p.B, p.C, generator=g))
    elif entry == "colsum":
        x = rn(p.rows, p.cols)
        x[-1] = 1.0 + x[-1].abs()
        v.update(x=x, seed=rn(p.cols) + 3.0)
    elif entry == "coords":
        v.update(x=rn(p.B, p.c, p.h, p.w))
    elif entry == "nchw":
        v.update(x=rn(p.B, p.c, p.h, p.w))
    elif entry == "cvt":
        x = rn(p.n) * torch.exp2(torch.randint(-20, 20, (p.n,), generator=g).float())
        x[:8] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                              float("inf"), -float("inf"), 3.0e38])          # ties to even, both ways; overflow
        v.update(x=_bf(x) if p.to == "f32" else x)
    else:
        raise KeyError(entry)
    return v


# ----------------------------------------------------------------------------------------- references
# every reference returns {output name: (value, bound)}: fp64 value (an exact class: the tensor in its
# own dtype) and the absolute bound of every entry; bound 0 = bit for bit (NaNs equal NaNs)
MUTANTS = ("bn whole batch", "bn biased running var", "bn one running update", "up align_corners false",
           "pool last max wins", "pool leak into the odd edge", "pool relu mask >=", "oc bias dropped",
           "oc last row dropped", "colsum last row dropped", "colsum accumulate ignored", "scale by channel only")


def _zero(t):
    return torch.zeros(t.shape, dtype=F64)


def bn_stats64(z, whole_batch=False):
    """per (slot, channel): mean, biased variance, mean |z|, mean z^2 in fp64 (two passes)"""
    dims = (0, 1) if whole_batch else (1,)
    mu = z.mean(dims, keepdim=True)
    var = ((z - mu) ** 2).mean(dims, keepdim=True)
    m1, m2 = z.abs().mean(dims, keepdim=True), (z * z).mean(dims, keepdim=True)
    ex = lambda t: t.expand(z.shape[0], 1, z.shape[2])[:, 0]          # noqa: E731
    return ex(mu), ex(var), ex(m1), ex(m2)


def _f32(t):
    return t.float().double()


def bn_fwd_ref(p, f, v, training, mutant=None, sum_unit=E53):
    """sum_unit: the unit roundoff of the statistics' sums (the kernels: fp64; ATen on the CPU may use fp32)"""
    B, hw, C = p.B, p.hw, p.C
    z = v["z"].double()
    gamma = v["gamma"].double() if f.affine else torch.ones(C, dtype=F64)
    beta = v["beta"].double() if f.affine else torch.zeros(C, dtype=F64)
    resid = v["resid"].double() if f.resid else None
    out = {}
    if training:
        mu, var, m1, m2 = bn_stats64(z, whole_batch=(mutant == "bn whole batch"))
        n = float(hw)
        b_mean = U * mu.abs() + (hw + 2) * sum_unit * m1
        dvar = (2 * hw + 6) * sum_unit * (m2 + mu * mu)
        rstd = (var + EPS) ** -0.5
        b_rstd = U * rstd + 0.5 * rstd ** 3 * dvar + 4 * E53 * rstd
        out["save_mean"], out["save_rstd"] = (mu, b_mean), (rstd, b_rstd)
        if f.running:
            unb = var if (hw == 1 or mutant == "bn biased running var") else var * n / (n - 1.0)
            rm, rv = v["rm"].double(), v["rv"].double()
            am, av = rm.abs(), rv.abs()
            em, ev = _zero(rm), _zero(rv)
            for b in range(1 if mutant == "bn one running update" else B):
                rm = _f32(MOM * mu[b] + (1.0 - MOM) * rm)
                rv = _f32(MOM * unb[b] + (1.0 - MOM) * rv)
                am = MOM * mu[b].abs() + (1.0 - MOM) * am
                av = MOM * unb[b].abs() + (1.0 - MOM) * av
                em = MOM * (hw + 2) * sum_unit * m1[b] + (1.0 - MOM) * em
                ev = MOM * dvar[b] * (1.0 if hw == 1 else n / (n - 1.0)) + (1.0 - MOM) * ev
            out["running_mean"], out["running_var"] = (rm, (B + 1) * U * am + em), (rv, (B + 1) * U * av + ev)
        mu, rstd, b_mean, b_rstd = (t[:, None, :] for t in (mu, rstd, b_mean, b_rstd))
    else:
        mu = v["rm"].double()
        rstd = (v["rv"].double() + EPS) ** -0.5
        b_rstd = U * rstd + 4 * E53 * rstd
        out["save_mean"], out["save_rstd"] = (mu, _zero(mu)), (rstd, b_rstd)
        b_mean = _zero(mu)
    a = rstd * gamma
    y = (z - mu) * a + beta
    M = (z.abs() + mu.abs()) * a.abs() + beta.abs()
    if resid is not None:
        y, M = y + resid, M + resid.abs()
    if f.relu:
        y = y.clamp_min(0.0)
    bound = (7 if f.resid else 6) * U * M + (b_rstd / rstd) * (z.abs() + mu.abs()) * a.abs() + b_mean * a.abs()
    out["y"] = (y, bound.expand_as(y))
    return out


def bn_saved(p, v):
    """save_mean / save_rstd as the forward stores them: the reference statistics rounded to fp32"""
    mu, var, _, _ = bn_stats64(v["z"].double())
    return mu.float(), ((var + EPS) ** -0.5).float()


def bn_bwd_ref(p, f, v, mutant=None, sum_unit=E53, stat_err=None):
    """sum_unit: the unit roundoff of the two sums (the kernels: fp64; ATen on the CPU may use fp32);
    stat_err = (dmean, drstd / rstd) per (slot, channel): the error of the saved statistics of an
    implementation that computes its own (the kernels are given the reference's)"""
    B, hw, C = p.B, p.hw, p.C
    z, g = v["z"].double(), v["g"].double()
    sm, sr = bn_saved(p, v)
    mean, r = sm.double()[:, None, :], sr.double()[:, None, :]
    gamma = v["gamma"].double() if f.affine else torch.ones(C, dtype=F64)
    n = float(hw)
    d = z - mean
    dims = (0, 1) if mutant == "bn whole batch" else (1,)
    nn = n * (B if mutant == "bn whole batch" else 1)
    s0, s1 = g.sum(dims, keepdim=True), (d * g).sum(dims, keepdim=True)
    A0, A1 = g.abs().sum(dims, keepdim=True), (d.abs() * g.abs()).sum(dims, keepdim=True)
    gm, k = s0 / nn, s1 * r * r / nn
    dz = (g - gm - d * k) * r * gamma
    M = (g.abs() + gm.abs() + d.abs() * k.abs()) * r * gamma.abs()
    sums = (hw + 2) * sum_unit * (A0 / n + d.abs() * A1 * r * r / n) * r * gamma.abs()
    if f.add:
        dz, M = dz + v["add"].double(), M + v["add"].double().abs()
    bound = (10 if f.add else 9) * U * M + sums
    if stat_err is not None:
        bound = bound + (k.abs() * stat_err[0][:, None, :] + 3 * stat_err[1][:, None, :] * M) * r * gamma.abs()
    if f.mask:
        on = v["mask"] > 0
        dz, bound = torch.where(on, dz, _zero(dz)), torch.where(on, bound, _zero(dz))
    out = {"dz": (dz, bound)}
    if f.dparams:
        s0, s1, A0, A1 = (t.expand(B, 1, C)[:, 0] if mutant == "bn whole batch" else t[:, 0] for t in (s0, s1, A0, A1))
        if mutant == "bn whole batch":
            s0, s1, A0, A1 = s0 / B, s1 / B, A0 / B, A1 / B
        rr = r[:, 0]
        dg, db = (s1 * rr).sum(0), s0.sum(0)
        out["dgamma"] = (dg, U * dg.abs() + (B * hw + B + 2) * E53 * (A1 * rr).sum(0))
        out["dbeta"] = (db, U * db.abs() + (B * hw + 2) * E53 * A0.sum(0))
    return out


def lin_f32(n_in):
    """ATen's area_pixel_compute_scale / source_index for align_corners=True, scale factor 2, in
    float32 op by op: (i0, i1, l0, l1) per output index"""
    f = np.float32
    out = 2 * n_in
    scale = f(n_in - 1) / f(out - 1) if out > 1 else f(0)
    real = (scale * np.arange(out, dtype=f)).astype(f)
    i0 = real.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (real - i0.astype(f)).astype(f)
    l0 = (f(1) - l1).astype(f)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def lin_exact(n_in):
    """the same with rational coordinates o (n - 1) / (2n - 1)"""
    out = 2 * n_in
    o = np.arange(out, dtype=np.int64)
    num, den = o * (n_in - 1), max(out - 1, 1)
    i0 = num // den
    i1 = i0 + (i0 < n_in - 1)
    l1 = (num - i0 * den).astype(np.float64) / den
    return i0, i1, 1.0 - l1, l1


def lin_half_pixel(n_in):
    """align_corners=False (the mutant): source (o + 0.5) / 2 - 0.5 clamped at 0"""
    out = 2 * n_in
    real = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * 0.5 - 0.5, 0.0)
    i0 = real.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = real - i0
    return i0, i1, 1.0 - l1, l1


def lin_matrix(n_in, rule):
    """[2n, n] interpolation matrix of one axis in fp64"""
    i0, i1, l0, l1 = rule(n_in)
    Wm = torch.zeros(2 * n_in, n_in, dtype=F64)
    for o in range(2 * n_in):
        Wm[o, i0[o]] += l0[o]
        Wm[o, i1[o]] += l1[o]
    return Wm


def up_ref(p, f, v, bwd, rule=lin_f32, mutant=None):
    if mutant == "up align_corners false":
        rule = lin_half_pixel
    Wh, Ww = lin_matrix(p.h, rule), lin_matrix(p.w, rule)
    if not bwd:
        x = v["x"].double()
        y = torch.einsum("oi,pj,bijc->bopc", Wh, Ww, x)
        M = torch.einsum("oi,pj,bijc->bopc", Wh.abs(), Ww.abs(), x.abs())
        return {"y": (y, 5 * U * M)}
    dy = v["dy"].double()
    dx = torch.einsum("oi,pj,bopc->bijc", Wh, Ww, dy)
    M = torch.einsum("oi,pj,bopc->bijc", Wh.abs(), Ww.abs(), dy.abs())
    T = torch.outer((Wh != 0).sum(0), (Ww != 0).sum(0)).double()[None, :, :, None]
    bound = (T + 4) * U * M
    if f.mask:
        on = v["mask"] > 0
        dx, bound = torch.where(on, dx, _zero(dx)), torch.where(on, bound, _zero(dx))
    return {"dx": (dx, bound)}


def up_coordinate_slack(p, v, bwd):
    """what the float32 coordinate formula may add to the bound against exact coordinates (module
    docstring): 4 (2 max(h, w) + 1) u per axis, times max |x| over the image and channel"""
    t = (v["dy"] if bwd else v["x"]).double().abs().amax((1, 2), keepdim=True)
    per_axis = 4 * (2 * max(p.h, p.w) + 1) * U
    # backward: four outputs per axis read a pixel, each weight off by up to twice that, and the other
    # axis's weights onto a pixel sum to at most 3: 24, taken as 32 (2 max(h, w) + 1) u per axis
    return 2 * per_axis * t * (8.0 if bwd else 1.0)


def pool_scan(x, last_wins=False):
    """ATen's max_pool2d scan of the 2x2 windows, row-major: take val if val > max || isnan(val)"""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    best = torch.full((B, Ho, Wo, C), float("-inf"))
    arg = torch.zeros((B, Ho, Wo, C), dtype=torch.long)
    for q in range(4):
        val = x[:, (q >> 1):2 * Ho:2, (q & 1):2 * Wo:2]
        take = ((val >= best) if last_wins else (val > best)) | val.isnan()
        best, arg = torch.where(take, val, best), torch.where(take, torch.full_like(arg, q), arg)
    return best, arg


def pool_ref(p, f, v, bwd, mutant=None):
    dt = BF if p.dt == "bf16" else F32
    x = v["x"]
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    best, arg = pool_scan(x, last_wins=(mutant == "pool last max wins"))
    scale = v["scale"][:, None, None, :] if f.scaled else None
    if not bwd:
        y = best * scale if f.scaled else best              # one fp32 product
        return {"y": (y.to(dt), _zero(y))}
    gs = v["dy"] * scale if f.scaled else v["dy"]
    dx = torch.zeros(B, H, W, C)
    for q in range(4):
        val = x[:, (q >> 1):2 * Ho:2, (q & 1):2 * Wo:2]
        sel = arg == q
        if f.relu:
            sel = sel & ((val >= 0) if mutant == "pool relu mask >=" else (val > 0))
        dx[:, (q >> 1):2 * Ho:2, (q & 1):2 * Wo:2] = torch.where(sel, gs, torch.zeros_like(gs))
    if mutant == "pool leak into the odd edge":
        if H % 2:
            dx[:, H - 1] = dx[:, H - 2]
        if W % 2:
            dx[:, :, W - 1] = dx[:, :, W - 2]
    if f.acc:
        dx = v["seed"] + dx                                  # one fp32 addition (then the bf16 store)
    return {"dx": (dx.to(dt), _zero(dx))}


def oc_fwd_ref(p, f, v, mutant=None):
    x, w = v["x"].double(), v["w"].double()
    b = v["b"].double() if f.bias and mutant != "oc bias dropped" else torch.zeros(1, dtype=F64)
    y = x @ w + b
    M = x.abs() @ w.abs() + (v["b"].double().abs() if f.bias else 0.0)
    scalar = kernel_of(Row("", "oc_fwd", None, p)) == frozenset(["outconv_fwd_scalar_kernel"])
    c = p.C + 2 if scalar else -(-p.C // 64) + 10
    return {"y": (y, c * U * M)}


def oc_bwd_ref(p, f, v, mutant=None):
    dt = BF if p.dt == "bf16" else F32
    x, w, g = v["x"], v["w"], v["dy"]
    dx = g[:, None] * w[None, :]                             # one fp32 product
    if f.relu:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    x64, g64 = x.double(), g.double()
    if mutant == "oc last row dropped":
        g64 = g64.clone()
        g64[-1] = 0.0
    dw, db = g64 @ x64, g64.sum().reshape(1)
    Mw, Mb = g.double().abs() @ x64.abs(), g.double().abs().sum().reshape(1)
    L = p.C // 4
    per = 256 // L if L in (2, 4, 8) else 16
    n_t = -(-p.rows // (p.blocks * per))
    c = n_t + per + 1
    return {"dx": (dx.to(dt), _zero(dx)), "dw": (dw, c * U * Mw), "db": (db, c * U * Mb)}


def scale_ref(p, f, v, mutant=None):
    s = v["scale"][0:1].expand_as(v["scale"]) if mutant == "scale by channel only" else v["scale"]
    y = v["x"] * s[:, None, :]
    return {"y": (y, _zero(y))}


def colsum_ref(p, f, v, mutant=None):
    x = v["x"].double()
    if mutant == "colsum last row dropped":
        x = x[:-1]
    s = x.sum(0)
    bound = U * s.abs() + (p.rows + 2) * E53 * v["x"].double().abs().sum(0)
    if f.acc and mutant != "colsum accumulate ignored":
        seed = v["seed"].double()
        return {"out": (seed + s, bound + U * (seed + s).abs())}
    return {"out": (s, bound)}


def coords_ref(p, f, v, mutant=None):
    """AddCoords + NCHW -> NHWC in numpy float32, one operation at a time (the layer's quirk included:
    xx runs over the columns but is scaled by h - 1, yy over the rows by w - 1)"""
    fl = np.float32
    B, c, h, w = p.B, p.c, p.h, p.w
    x = v["x"].numpy()
    j = np.broadcast_to(np.arange(w, dtype=fl)[None, :], (h, w))
    i = np.broadcast_to(np.arange(h, dtype=fl)[:, None], (h, w))
    xx = ((j / fl(h - 1)).astype(fl) * fl(2)).astype(fl) - fl(1)
    yy = ((i / fl(w - 1)).astype(fl) * fl(2)).astype(fl) - fl(1)
    chans = [x[:, k] for k in range(c)] + [np.broadcast_to(xx, (B, h, w)), np.broadcast_to(yy, (B, h, w))]
    if p.with_r:
        dx, dy = (xx - fl(0.5)).astype(fl), (yy - fl(0.5)).astype(fl)
        rr = np.sqrt(((dx * dx).astype(fl) + (dy * dy).astype(fl)).astype(fl)).astype(fl)
        chans.append(np.broadcast_to(rr, (B, h, w)))
    out = torch.from_numpy(np.stack(chans, axis=-1).astype(fl).copy())
    return {"out": (out, _zero(out))}


def nchw_ref(p, f, v, mutant=None):
    y = v["x"].permute(0, 2, 3, 1).contiguous()
    return {"out": (y, _zero(y))}


def cvt_ref(p, f, v, mutant=None):
    y = v["x"].to(BF) if p.to == "bf16" else v["x"]
    return {"out": (y, _zero(y))}


def _reference(entry, p, f, v, mutant=None):
    if entry == "bn_fwd":
        return bn_fwd_ref(p, f, v, True, mutant)
    if entry == "bn_eval":
        return bn_fwd_ref(p, f, v, False, mutant)
    if entry == "bn_bwd":
        return bn_bwd_ref(p, f, v, mutant)
    if entry in ("up_fwd", "up_bwd"):
        return up_ref(p, f, v, entry == "up_bwd", mutant=mutant)
    if entry in ("pool_fwd", "pool_bwd"):
        return pool_ref(p, f, v, entry == "pool_bwd", mutant)
    return {"oc_fwd": oc_fwd_ref, "oc_bwd": oc_bwd_ref, "scale": scale_ref, "colsum": colsum_ref, "coords": coords_ref,
            "nchw": nchw_ref, "cvt": cvt_ref}[entry](p, f, v, mutant)


@functools.lru_cache(maxsize=None)
def reference(name, form):
    """{output: (value, bound)} of a (row, form) pair; computed once and left unchanged"""
    r = CASE[name]
    return _reference(r.entry, r.p, FORMS[r.entry][form], values(name))


def mutated(name, form, mutant):
    r = CASE[name]
    return _reference(r.entry, r.p, FORMS[r.entry][form], values(name), mutant)


def applies(r, f, mutant):
    """whether a mutant changes what the (row, form) pair computes"""
    p, e = r.p, r.entry
    if mutant == "bn whole batch":
        return e in ("bn_fwd", "bn_bwd") and p.B > 1 and p.hw > 1
    if mutant == "bn biased running var":
        return e == "bn_fwd" and bool(f.running) and p.hw > 1
    if mutant == "bn one running update":
        return e == "bn_fwd" and bool(f.running) and p.B > 1
    if mutant == "up align_corners false":
        return e in ("up_fwd", "up_bwd") and (p.h > 1 or p.w > 1)
    if mutant == "pool last max wins":
        return e == "pool_bwd"
    if mutant == "pool leak into the odd edge":
        return e == "pool_bwd" and (p.H % 2 or p.W % 2) == 1
    if mutant == "pool relu mask >=":
        return e == "pool_bwd" and bool(f.relu)
    if mutant == "oc bias dropped":
        return e == "oc_fwd" and bool(f.bias)
    if mutant == "oc last row dropped":
        return e == "oc_bwd"
    if mutant == "colsum last row dropped":
        return e == "colsum"
    if mutant == "colsum accumulate ignored":
        return e == "colsum" and bool(f.acc)
    if mutant == "scale by channel only":
        return e == "scale" and p.B > 1
    raise KeyError(mutant)


def ratio(got, ref, bound):
    """per entry |got - ref| / bound; an entry with bound 0 must be exact (0 or inf); NaN equals NaN,
    and +-inf equals the same infinity"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    bound = bound.double().reshape(-1)
    same = (got == ref) | (got.isnan() & ref.isnan())
    err = torch.where(same, torch.zeros_like(got), (got - ref).abs()).nan_to_num(nan=float("inf"), posinf=float("inf"))
    return torch.where(bound > 0, err / bound.clamp_min(1e-300),
                       torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


# ------------------------------------------------------------------------------------- device runner
Result = collections.namedtuple("Result", "rc outs intact untouched kept extra")
_DT = {"f32": F32, "bf16": BF}


class _Call:
    """the guarded buffers and device operands of one call"""

    def __init__(self, over):
        self.over, self.guards, self.outs, self.keep, self.ws = over, [], {}, [], None
        self.mis = set(over.get("mis", ()))
        self.null = set(over.get("null", ()))

    def src(self, name, t, dtype=F32):
        if name in self.null:
            return None
        d = _dev(t, dtype, 1 if name in self.mis else 0)
        self.keep.append(d)
        return d.data_ptr()

    def dst(self, name, numel, dtype=F32, seed=None, written=None, out=True):
        """a destination between sentinel bands, filled with the sentinel NaN or the seed; written:
        the slice of it the call must write (default: all of it)"""
        g = Guarded(numel, dtype, off=1 if name in self.mis else 0)
        if seed is not None:
            g.inner.copy_(seed.reshape(-1).to(dtype))
        self.guards.append(g)
        if out:
            self.outs[name] = (g, written)
        return None if name in self.null else g.ptr()

    def call(self, fn, *args):
        self.before = [g.inner.clone() for g in self.guards]
        return fn(*args)

    def workspace(self, need):
        if self.over.get("ws_null"):
            return None, 0
        g = Guarded(max(need // 4, 1), F32)
        self.guards.append(g)
        self.ws = g
        return g.ptr(), need - self.over.get("ws_short", 0)


def _launch(r, f, c, stream):
    """builds the operands of the row's call in form f and makes it; returns the status"""
    L, p, e = _lib.load(), r.p, r.entry
    v = values(r.name, p if r.name not in CASE else None, e if r.name not in CASE else None)
    mis = p.mis
    if mis:
        c.mis.add(mis)
    if e in ("bn_fwd", "bn_eval"):
        B, hw, C = p.B, p.hw, p.C
        training = e == "bn_fwd"
        z = c.src("z", v["z"])
        gamma = c.src("gamma", v["gamma"]) if f.affine else None
        beta = c.src("beta", v["beta"]) if f.affine else None
        resid = c.src("resid", v["resid"]) if f.resid else None
        rm = rv = None
        if f.running:
            rm = c.dst("running_mean", C, seed=v["rm"], out=training)
            rv = c.dst("running_var", C, seed=v["rv"], out=training)
        y = c.dst("y", B * hw * C)
        sm = c.dst("save_mean", B * C, written=None if training else C)
        sr = c.dst("save_rstd", B * C, written=None if training else C)
        ws = c.workspace(L.pu_bn_workspace_bytes(B, hw, C)) if training or c.over.get("ws") else (None, 0)
        return c.call(L.pu_bn_fwd, z, gamma, beta, rm, rv, y, sm, sr, B, hw, C, EPS, MOM, int(training), int(bool(f.relu)), resid,
                           ws[0], ws[1], stream)
    if e == "bn_bwd":
        B, hw, C = p.B, p.hw, p.C
        sm, sr = bn_saved(p, v)
        a = [c.src("z", v["z"]), c.src("g", v["g"]), c.src("save_mean", sm), c.src("save_rstd", sr),
             c.src("gamma", v["gamma"]) if f.affine else None, c.dst("dz", B * hw * C)]
        a += [c.dst("dgamma", C), c.dst("dbeta", C)] if f.dparams else [None, None]
        add = c.src("add", v["add"]) if f.add else None
        mask = c.src("mask", v["mask"]) if f.mask else None
        ws = c.workspace(L.pu_bn_workspace_bytes(B, hw, C))
        return c.call(L.pu_bn_bwd, *a, B, hw, C, add, mask, ws[0], ws[1], stream)
    if e == "up_fwd":
        return c.call(L.pu_upsample_bilinear2x_fwd, c.src("x", v["x"]), c.dst("y", 4 * p.B * p.h * p.w * p.C), p.B, p.h, p.w, p.C,
                                            stream)
    if e == "up_bwd":
        return c.call(L.pu_upsample_bilinear2x_bwd, c.src("dy", v["dy"]), c.src("mask", v["mask"]) if f.mask else None,
                                            c.dst("dx", p.B * p.h * p.w * p.C), p.B, p.h, p.w, p.C, stream)
    if e == "pool_fwd":
        dt = _DT[p.dt]
        x = c.src("x", v["x"], dt)
        y = c.dst("y", p.B * (p.H // 2) * (p.W // 2) * p.C, dt)
        if p.dt == "bf16":
            return c.call(L.pu_maxpool2_fwd_bf16, x, y, p.B, p.H, p.W, p.C, stream)
        if f.scaled:
            return c.call(L.pu_maxpool2_fwd_scaled, x, c.src("scale", v["scale"]), y, p.B, p.H, p.W, p.C, stream)
        return c.call(L.pu_maxpool2_fwd, x, y, p.B, p.H, p.W, p.C, stream)
    if e == "pool_bwd":
        dt = _DT[p.dt]
        x, dy = c.src("x", v["x"], dt), c.src("dy", v["dy"], dt)
        dx = c.dst("dx", p.B * p.H * p.W * p.C, dt, seed=v["seed"] if f.acc else None)
        tail = (p.B, p.H, p.W, p.C, int(bool(f.relu)), int(bool(f.acc)), stream)
        if p.dt == "bf16":
            return c.call(L.pu_maxpool2_bwd_bf16, x, dy, dx, *tail)
        if f.scaled:
            return c.call(L.pu_maxpool2_bwd_scaled, x, dy, c.src("scale", v["scale"]), dx, *tail)
        return c.call(L.pu_maxpool2_bwd, x, dy, dx, *tail)
    if e == "oc_fwd":
        fn = L.pu_outconv_fwd_bf16 if p.dt == "bf16" else L.pu_outconv_fwd
        return c.call(fn, c.src("x", v["x"], _DT[p.dt]), c.src("w", v["w"]), c.src("b", v["b"]) if f.bias else None,
                  c.dst("y", p.rows), p.rows, p.C, stream)
    if e == "oc_bwd":
        fn = L.pu_outconv_bwd_bf16 if p.dt == "bf16" else L.pu_outconv_bwd
        a = [c.src("x", v["x"], _DT[p.dt]), c.src("w", v["w"]), c.src("dy", v["dy"]), c.dst("dx", p.rows * p.C, _DT[p.dt]),
             c.dst("dw", p.C), c.dst("db", 1)]
        ws = c.workspace(L.pu_outconv_workspace_bytes(p.rows, p.C))
        return c.call(fn, *a, p.rows, p.C, int(bool(f.relu)), ws[0], ws[1], stream)
    if e == "scale":
        return c.call(L.pu_channel_scale, c.src("x", v["x"]), c.src("scale", v["scale"]), c.dst("y", p.B * p.hw * p.C), p.B, p.hw, p.C,
                                  stream)
    if e == "colsum":
        a = [c.src("x", v["x"]), p.rows, p.cols, c.dst("out", p.cols, seed=v["seed"] if f.acc else None), int(bool(f.acc))]
        ws = c.workspace(L.pu_column_sum_workspace_bytes(p.rows, p.cols))
        return c.call(L.pu_column_sum, *a, ws[0], ws[1], stream)
    if e == "coords":
        return c.call(L.pu_add_coords, c.src("x", v["x"]), c.dst("out", p.B * p.h * p.w * (p.c + 2 + p.with_r)), p.B, p.c, p.h, p.w,
                               p.with_r, stream)
    if e == "nchw":
        return c.call(L.pu_nchw_to_nhwc, c.src("x", v["x"]), c.dst("out", p.B * p.c * p.h * p.w), p.B, p.c, p.h, p.w, stream)
    if e == "cvt":
        if p.to == "bf16":
            return c.call(L.pu_convert_f32_bf16, c.src("x", v["x"]), c.dst("out", p.n, BF), p.n, stream)
        return c.call(L.pu_convert_bf16_f32, c.src("x", v["x"], BF), c.dst("out", p.n), p.n, stream)
    raise KeyError(e)


def run(r, f, **over):
    """One guarded call of row r in form f.  Every destination and the workspace - exactly the bytes
    the query asks for - lie between sentinel bands, pre-filled with the sentinel NaN (a destination
    under accumulate, and the running statistics: with their seed).  Returns the status, the outputs
    (CPU, in their own dtype), whether every band survived, whether every destination and the
    workspace still hold their fill bit for bit, whether an entry the call must write kept the
    sentinel, and whether the entries it must not write (BatchNorm eval: [C, B C) of the statistics)
    kept it.  over: what the rejected calls change (mis / null: operand names; ws_short; ws_null)."""
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
        outs[name] = g.inner[:n].cpu()
    return Result(rc, outs, intact, untouched, kept, extra)
