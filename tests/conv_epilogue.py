"""Every convolution kernel against every epilogue form it can be given: the case table, the fp64
reference, the derived bounds and the guarded device runner shared by test_conv_epilogue.py (CPU)
and test_conv_epilogue_gpu.py.

One pu_conv_igemm / pu_conv_igemm_bf16 call can combine bias, residual, ReLU, mask0 / mask1, a
per-(image, channel) scale, accumulate, a split over two destinations and the ConvT shuffle, in the
order csrc/conv_common.h documents (bias, residual, ReLU, mask, channel scale, accumulate).  CASES
names one row per kernel the dispatch can pick - steered by what the call passes (weight6, wino,
cgroup, the two dispatch hints, the grid), never by process-wide switches - with the plan the
library reports for it; FORMS lists the epilogue forms of each layout class.

Reference: the convolution in fp64 (F.conv2d / F.conv_transpose2d + crop) and the epilogue in fp64.

Bounds (derived, not measured):
  fp32 GEMM level   the project's fp32 conv tolerance, rtol 1e-4 and atol 1e-5 * max|ref|.
  fp32 epilogue     the call with identity values (bias 0, resid 0, masks 1, scale 1, seed 0, no
                    ReLU; same pointers, so the same kernel instantiation) yields the raw
                    accumulators z.  The real call applies at most four fp32 roundings to z (bias,
                    residual, scale, accumulate), each at most 2^-24 of an intermediate bounded by
                    S = (|z| + |bias| + |resid|) * |scale| + |seed|; contraction into an fma only
                    removes roundings:  |got - epilogue64(z)| <= 4 * 2^-24 * S  per element.
  bf16              one round-to-nearest bf16 store on top of the fp32 GEMM tolerance:
                    |got - ref| <= 2^-8 |ref| + 1.01 d,  d = 1e-4 |ref| + 1e-5 max|ref|.
"""
import collections
import ctypes
import functools

import torch
import torch.nn.functional as F

from punet import _lib

RELU, ACCUM, SHUF, RESID, NO_HALO, NO_SMALLX6 = 1, 2, 4, 8, 16, 64
BF = torch.bfloat16
GUARD = 4096                    # sentinel floats before and after every destination and the workspace
SENT32, SENT16 = 0x7FC5A5A5, 0x7FC5     # a NaN with a payload no kernel produces (fp32 / bf16 words)

# ------------------------------------------------------------------------------------ epilogue forms
# the operands of a form; "relu" and "accum" are flags, the rest are pointers
_F = frozenset
FORMS = {
    "one": collections.OrderedDict([
        ("none", _F()),
        ("bias", _F({"bias"})),
        ("bias+relu", _F({"bias", "relu"})),
        ("mask0", _F({"mask0"})),
        ("relu+mask0", _F({"relu", "mask0"})),
        ("bias+relu+mask0", _F({"bias", "relu", "mask0"})),
        ("bias+resid+relu", _F({"bias", "resid", "relu"})),
        ("resid+mask0", _F({"resid", "mask0"})),
        ("cscale+mask0", _F({"cscale", "mask0"})),
        ("accum", _F({"accum"})),
        ("all", _F({"bias", "resid", "relu", "mask0", "cscale", "accum"})),
    ]),
    "split": collections.OrderedDict([
        ("none", _F()),
        ("bias", _F({"bias"})),
        ("masks", _F({"mask0", "mask1"})),
        ("mask0", _F({"mask0"})),
        ("mask1", _F({"mask1"})),
        ("bias+relu+masks", _F({"bias", "relu", "mask0", "mask1"})),
        ("cscale+mask1", _F({"cscale", "mask1"})),
        ("accum", _F({"accum"})),
        ("all", _F({"bias", "relu", "mask0", "mask1", "cscale", "accum"})),
    ]),
    "shuf": collections.OrderedDict([
        ("none", _F()),
        ("bias", _F({"bias"})),
        ("bias+relu", _F({"bias", "relu"})),
        ("bias+cscale", _F({"bias", "cscale"})),
        ("bias+mask0", _F({"bias", "mask0"})),
        ("bias+accum", _F({"bias", "accum"})),
        ("all", _F({"bias", "relu", "mask0", "cscale", "accum"})),
    ]),
}


def excluded(case, ops):
    """The explicit rules that leave a (case, form) pair out: what the API rejects, and - for a row
    whose point is one misaligned operand - the forms that do not pass that operand."""
    if "resid" in ops and case.layout != "one":
        return "RESID needs one destination and no SHUFFLE2"
    if "cscale" in ops and case.entry == "bf16":
        return "chan_scale is an fp32-entry epilogue"
    if case.mis in ("bias", "mask0") and case.mis not in ops:
        return "the misaligned operand is absent"
    return None


# ---------------------------------------------------------------------------------------- case table
Case = collections.namedtuple("Case", "name entry kernel B H W c0 c1 n n0 op k cg w6 wino flags crop mis plan")


def _case(name, entry, kernel, shape, plan, n0=None, op="conv", k=3, cg=0, w6=False, wino=False, flags=0, crop=0,
          mis=None):
    """shape = (B, H, W, c0, c1, n): the input grid, the two sources and the GEMM columns (ConvT: the
    output channels co, n = 4 co).  plan = (bm, bn, mode | kind, K splits with the scratch the
    workspace query asks for); without scratch every plan runs unsplit."""
    B, H, W, c0, c1, n = shape
    if op != "conv":
        n *= 4
    return Case(name, entry, kernel, B, H, W, c0, c1, n, n if n0 is None else n0, op, k, cg, w6, wino, flags, crop, mis,
                plan)


X6 = dict(w6=True)
LEAN = dict(w6=True, cg=32)
WINO = dict(w6=True, wino=True, cg=32)
T2 = dict(op="convT2", k=1)                 # ConvTranspose2d 2x2 / s2 forward: 1x1 GEMM + SHUFFLE2
T3 = dict(op="convT3", k=2, w6=True)        # ConvTranspose2d 3x3 / s2 forward: 2x2 / p1 sub-pixel conv + SHUFFLE2

CASES = [
    # ---- fp32 entry (mode: 0 chunk16 DMA, 1 vec4, 2 scalar, 3 direct, 4 x6, 5 stem, 6 wino, 7 smallx6)
    _case("stem 1->16", "f32", "stem", (2, 9, 13, 1, 0, 16), (1024, 16, 5, 1)),
    _case("1x1 small 4->8", "f32", "1x1", (2, 9, 13, 4, 0, 8), (256, 8, 3, 1), k=1),
    _case("1x1 small 4+4->16", "f32", "1x1", (2, 9, 13, 4, 4, 16), (256, 16, 3, 1), k=1),
    _case("smallx6 8->8", "f32", "smallx6", (2, 9, 13, 8, 0, 8), (512, 8, 7, 1), **X6),
    _case("smallx6 16->16 n0 8", "f32", "smallx6", (2, 9, 13, 16, 0, 16), (512, 16, 7, 1), n0=8, **X6),
    _case("direct 12->8", "f32", "direct", (2, 9, 13, 12, 0, 8), (512, 8, 3, 1)),
    _case("direct 16->16 (NO_SMALLX6)", "f32", "direct", (2, 9, 13, 16, 0, 16), (512, 16, 3, 1), flags=NO_SMALLX6, **X6),
    _case("direct 4+4->4", "f32", "direct", (1, 9, 13, 4, 4, 4), (512, 4, 3, 1)),
    _case("wino 64->64", "f32", "wino 64", (2, 12, 8, 64, 0, 64), (256, 64, 6, 1), **WINO),
    _case("wino 64+64->128 n0 64", "f32", "wino 64", (1, 8, 8, 64, 64, 128), (256, 64, 6, 1), n0=64, **WINO),
    _case("wino wide 64->128 n0 96", "f32", "wino wide", (1, 4, 4, 64, 0, 128), (128, 128, 6, 1), n0=96, **WINO),
    _case("wino split-K 256->64", "f32", "wino 64", (1, 8, 8, 256, 0, 64), (256, 64, 6, 2), **WINO),
    _case("x6 lean 128x32", "f32", "x6 lean 128x32", (2, 9, 13, 32, 0, 32), (128, 32, 4, 1), **LEAN),
    _case("x6 lean 128x64 64->64", "f32", "x6 lean 128x64", (2, 9, 13, 64, 0, 64), (128, 64, 4, 2), **LEAN),
    _case("x6 lean 128x64 32->48 n0 16", "f32", "x6 lean 128x64", (2, 9, 13, 32, 0, 48), (128, 64, 4, 1), n0=16, **LEAN),
    _case("x6 lean 128x128 64+64->96 n0 32", "f32", "x6 lean 128x128", (1, 9, 13, 64, 64, 96), (128, 128, 4, 4), n0=32,
          **LEAN),
    _case("x6 lean 128x128 48+48->96 n0 32 cg16", "f32", "x6 lean 128x128", (1, 9, 13, 48, 48, 96), (128, 128, 4, 6),
          n0=32, w6=True, cg=16),
    _case("x6 lean 256x128 256->160 n0 96", "f32", "x6 lean 256x128", (5, 7, 9, 256, 0, 160), (256, 128, 4, 8), n0=96,
          **LEAN),
    _case("x6 64->64 cg0", "f32", "x6", (2, 9, 13, 64, 0, 64), (128, 64, 4, 4), **X6),
    _case("x6 32+64->64", "f32", "x6", (1, 9, 13, 32, 64, 64), (128, 64, 4, 6), w6=True, cg=32),
    _case("x6 1x1 64->64", "f32", "x6", (2, 9, 13, 64, 0, 64), (128, 64, 4, 1), k=1, **X6),
    _case("x6 ConvT2 64->4x32", "f32", "x6", (2, 5, 7, 64, 0, 32), (128, 128, 4, 1), w6=True, **T2),
    _case("x6 ConvT2 64->4x48", "f32", "x6", (2, 5, 7, 64, 0, 48), (128, 128, 4, 1), w6=True, **T2),
    _case("x6 ConvT3 32->4x16 crop0", "f32", "x6", (2, 5, 5, 32, 0, 16), (128, 64, 4, 1), **T3),
    _case("x6 ConvT3 32->4x16 crop1", "f32", "x6", (2, 5, 5, 32, 0, 16), (128, 64, 4, 1), crop=1, **T3),
    _case("smallx6 ConvT3 16->4x8 crop0", "f32", "smallx6", (2, 5, 5, 16, 0, 8), (256, 32, 7, 1), **T3),
    _case("smallx6 ConvT3 16->4x8 crop1", "f32", "smallx6", (2, 5, 5, 16, 0, 8), (256, 32, 7, 1), crop=1, **T3),
    _case("dma 32->32", "f32", "dma", (2, 9, 13, 32, 0, 32), (64, 64, 0, 2)),
    _case("dma 64+64->64", "f32", "dma", (1, 4, 4, 64, 64, 64), (64, 64, 0, 9)),
    _case("dma ConvT2 128->4x32", "f32", "dma", (2, 4, 4, 128, 0, 32), (64, 64, 0, 1), **T2),
    _case("vec4 loader 20->32", "f32", "loader vec4", (2, 9, 13, 20, 0, 32), (64, 64, 1, 1)),
    _case("scalar loader 3->32", "f32", "loader scalar", (2, 9, 13, 3, 0, 32), (64, 64, 2, 1)),
    _case("scalar loader 3+3->6 n0 3", "f32", "loader scalar", (2, 9, 13, 3, 3, 6), (64, 64, 2, 1), n0=3),
    # one operand 4-byte but not 16-byte aligned: the MFMA kernels' per-element branch, and the
    # small kernels re-planned onto the tiled ones
    _case("x6 lean 64->64, bias + 4 B", "f32", "x6 lean 128x64 elem", (2, 9, 13, 64, 0, 64), (128, 64, 4, 1), mis="bias", **LEAN),
    _case("x6 lean 64->64, dst0 + 4 B", "f32", "x6 lean 128x64 elem", (2, 9, 13, 64, 0, 64), (128, 64, 4, 1), mis="dst0", **LEAN),
    _case("x6 lean 64->64, mask0 + 4 B", "f32", "x6 lean 128x64 elem", (2, 9, 13, 64, 0, 64), (128, 64, 4, 1), mis="mask0", **LEAN),
    _case("stem 1->16, bias + 4 B", "f32", "loader scalar elem", (2, 9, 13, 1, 0, 16), (64, 64, 2, 1), mis="bias"),
    _case("stem 1->16, dst0 + 4 B", "f32", "loader scalar elem", (2, 9, 13, 1, 0, 16), (64, 64, 2, 1), mis="dst0"),
    _case("stem 1->16, mask0 + 4 B", "f32", "loader scalar elem", (2, 9, 13, 1, 0, 16), (64, 64, 2, 1), mis="mask0"),
    _case("x6 64->64 n0 30", "f32", "x6 elem", (2, 9, 13, 64, 0, 64), (128, 64, 4, 1), n0=30, **X6),
    # ---- bf16 entry (kind: 0 tile, 1 lean, 2 halo, 3 rows)
    _case("bf16 tile 32->32", "bf16", "bf16 tile", (2, 9, 13, 32, 0, 32), (64, 64, 0, 2)),
    _case("bf16 tile 32+64->64", "bf16", "bf16 tile", (1, 9, 13, 32, 64, 64), (64, 64, 0, 6), cg=32),
    _case("bf16 tile 128+64->64", "bf16", "bf16 tile", (1, 4, 4, 128, 64, 64), (64, 64, 0, 11), cg=32),
    _case("bf16 lean 64->64", "bf16", "bf16 lean", (2, 9, 13, 64, 0, 64), (256, 64, 1, 2), cg=32),
    _case("bf16 lean 64+64->96 n0 32", "bf16", "bf16 lean", (1, 9, 13, 64, 64, 96), (128, 128, 1, 4), n0=32, cg=32),
    _case("bf16 lean 128+128->64", "bf16", "bf16 lean", (1, 4, 4, 128, 128, 64), (256, 64, 1, 8), cg=32),
    _case("bf16 halo 64->64", "bf16", "bf16 halo", (1, 8, 32, 64, 0, 64), (256, 64, 2, 1), cg=32),
    _case("bf16 halo 32+32->128 n0 64", "bf16", "bf16 halo", (1, 8, 32, 32, 32, 128), (256, 64, 2, 1), n0=64, cg=32),
    _case("bf16 rows 64->64", "bf16", "bf16 rows", (1, 16, 128, 64, 0, 64), (128, 64, 3, 1), cg=32),
    _case("bf16 ConvT2 64->4x32", "bf16", "bf16 tile", (2, 5, 7, 64, 0, 32), (64, 64, 0, 1), **T2),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# every kernel the tables of the epilogue matrix name; "elem": vec_epi == 0 by alignment or n0
KERNELS = {"stem", "1x1", "smallx6", "direct", "wino 64", "wino wide", "x6 lean 128x32", "x6 lean 128x64",
           "x6 lean 128x128", "x6 lean 256x128", "x6", "dma", "loader vec4", "loader scalar", "x6 lean 128x64 elem",
           "loader scalar elem", "x6 elem", "bf16 tile", "bf16 lean", "bf16 halo", "bf16 rows"}


def layout(c):
    return "shuf" if c.op != "conv" else "one" if c.n0 == c.n else "split"


Case.layout = property(layout)


def geometry(c):
    """(out grid of the GEMM, pad, k_pad, pack mode, (shuf_h, shuf_w, shuf_off), logical output shape)"""
    C = c.c0 + c.c1
    kpm = 16 if c.entry == "f32" else 32
    if c.op == "convT2":
        K, out, pad, mode, shuf = C, (c.H, c.W), 0, _lib.PU_PACK_CONVT_FWD, (0, 0, 0)
        shape = (c.B, 2 * c.H, 2 * c.W, c.n // 4)
    elif c.op == "convT3":
        K, out, pad, mode = 4 * C, (c.H + 1, c.W + 1), 1, _lib.PU_PACK_CONVT3_FWD
        shuf = (2 * c.H + 1 - c.crop, 2 * c.W + 1 - c.crop, c.crop)
        shape = (c.B, shuf[0], shuf[1], c.n // 4)
    else:
        K, out, pad, mode, shuf = c.k * c.k * C, (c.H, c.W), (c.k - 1) // 2, _lib.PU_PACK_CONV_FWD, (0, 0, 0)
        shape = (c.B, c.H, c.W, c.n)
    return out, pad, (K + kpm - 1) // kpm * kpm, mode, shuf, shape


def cs_ld(c):
    """chan_scale row stride: the scaled channels rounded up to 4, plus 4 (never the default)"""
    return (geometry(c)[5][3] + 3) // 4 * 4 + 4


def splits(c):
    """the scratch variants a row runs: unsplit only, or the split-K finish and the in-kernel epilogue"""
    return (False, True) if c.plan[3] > 1 else (False,)


def pairs():
    """every (case name, form name, scratch) the GPU file runs"""
    out = []
    for c in CASES:
        for fname, ops in FORMS[c.layout].items():
            if excluded(c, ops) is None:
                out += [(c.name, fname, s) for s in splits(c)]
    return out


def conv_args(c, ops, ptr, ws=(None, 0)):
    """pu_conv_args of case c with the operands of a form; ptr: name -> device address."""
    (oh, ow), pad, k_pad, _, shuf, _ = geometry(c)
    flags = c.flags | (RELU if "relu" in ops else 0) | (ACCUM if "accum" in ops else 0) | \
        (RESID if "resid" in ops else 0) | (SHUF if c.layout == "shuf" else 0)
    a = _lib.ConvArgs(c.B, c.H, c.W, oh, ow, c.k, c.k, 1, pad, ptr["src0"], c.c0, ptr["src1"] if c.c1 else None, c.c1,
                      ptr["weight"], k_pad, c.cg, c.n, ptr["bias"] if "bias" in ops else None, ptr["dst0"], c.n0,
                      ptr["dst1"] if c.layout == "split" else None, ptr["mask0"] if "mask0" in ops else None,
                      ptr["mask1"] if "mask1" in ops else None, flags, ws[0], ws[1],
                      ptr["resid"] if "resid" in ops else None, shuf[0], shuf[1], shuf[2])
    a.weight6 = ptr["weight6"] if c.w6 else None
    a.wino = ptr["wino"] if c.wino else None
    if "cscale" in ops:
        a.chan_scale, a.chan_scale_ld = ptr["cscale"], cs_ld(c)
    return a


def _fns(entry):
    L = _lib.load()
    if entry == "f32":
        return L.pu_conv_igemm, L.pu_conv_igemm_workspace_bytes, L.pu_conv_igemm_tile
    return L.pu_conv_igemm_bf16, L.pu_conv_igemm_bf16_workspace_bytes, L.pu_conv_igemm_bf16_tile


def plan_of(c, a):
    """(bm, bn, mode | kind, ksplit) the library reports for args a (None: the query refuses them),
    and the scratch it asks for"""
    _, ws_fn, tile_fn = _fns(c.entry)
    bm, bn, x, y = (ctypes.c_int(0) for _ in range(4))
    if tile_fn(ctypes.byref(a), *(ctypes.byref(v) for v in (bm, bn, x, y))) != 0:
        return None, ws_fn(ctypes.byref(a))
    mode, ks = (x.value, y.value) if c.entry == "f32" else (y.value, x.value)
    return (bm.value, bn.value, mode, ks), ws_fn(ctypes.byref(a))


STANDIN = 0x10000


def standin_ptrs(c):
    """16-byte aligned stand-in addresses that no planning query dereferences (the misaligned
    operand: 4 bytes further)"""
    names = ("src0", "src1", "weight", "weight6", "wino", "bias", "dst0", "dst1", "mask0", "mask1", "resid", "cscale")
    return {nm: STANDIN * (i + 1) + (4 if nm == c.mis else 0) for i, nm in enumerate(names)}


def expect_lean(c):
    """csrc/igemm.hip lean_ok for the table's shapes: the x6 kernel a mode-4 plan runs"""
    C = c.c0 + c.c1
    return c.w6 and c.op == "conv" and c.k == 3 and c.cg in (16, 32) and c.c1 in (0, c.c0) and geometry(c)[2] == 9 * C


# ------------------------------------------------------------------------------ values and reference
def _round(t, entry):
    return t.to(BF).float() if entry == "bf16" else t


@functools.lru_cache(maxsize=None)
def values(name):
    """The operands of a case (CPU fp32 tensors; the bf16 entry's rounded to bf16 first): sources and
    weight, and every epilogue operand in the logical output layout [B, Ho, Wo, channels]."""
    c = CASE[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    _, _, _, _, _, shape = geometry(c)
    C = c.c0 + c.c1
    ch = shape[3]
    r = lambda *s: _round(torch.randn(*s, generator=g), c.entry)      # noqa: E731
    v = dict(x0=r(c.B, c.H, c.W, c.c0), x1=r(c.B, c.H, c.W, c.c1) if c.c1 else None)
    taps = {"conv": c.k * c.k, "convT2": 4, "convT3": 9}[c.op]
    wshape = (c.n, C, c.k, c.k) if c.op == "conv" else (C, ch, 2, 2) if c.op == "convT2" else (C, ch, 3, 3)
    v["w"] = _round(torch.randn(*wshape, generator=g) * (taps * C) ** -0.5, c.entry)
    v["bias"] = r(ch)
    v["resid"] = r(*shape)
    mask = torch.randn(*shape, generator=g)
    mask[torch.rand(*shape, generator=g) < 0.125] = 0.0       # exact zeros: > 0, != 0 and >= 0 differ
    v["mask"] = _round(mask, c.entry)
    scale = torch.full((c.B, cs_ld(c)), 7.0)                   # the pad columns must never be read
    scale[:, :ch] = 2.0 * (torch.rand(c.B, ch, generator=g) < 0.5).float()
    v["cscale"] = scale
    v["seed"] = r(*shape)
    return v


def conv64(c, v):
    """The convolution of case c in fp64, in the logical output layout [B, Ho, Wo, channels]."""
    x = v["x0"] if v["x1"] is None else torch.cat([v["x0"], v["x1"]], 3)
    x = x.double().permute(0, 3, 1, 2)
    w = v["w"].double()
    if c.op == "conv":
        z = F.conv2d(x, w, padding=(c.k - 1) // 2)
    elif c.op == "convT2":
        z = F.conv_transpose2d(x, w, stride=2)
    else:
        z = F.conv_transpose2d(x, w, stride=2)[:, :, c.crop:, c.crop:]
    return z.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASE[name]
    z = conv64(c, values(name))
    assert tuple(z.shape) == geometry(c)[5], (z.shape, geometry(c)[5])
    return z


def operands(c, ops, neutral=False):
    """The logical fp64 epilogue operands of a call (None: absent).  mask: the mask over all
    channels, ones on a side whose pointer is absent; neutral: the identity values."""
    v = values(c.name)
    _, _, _, _, _, shape = geometry(c)
    ch = shape[3]
    o = dict(bias=None, resid=None, mask=None, scale=None, seed=None, relu="relu" in ops and not neutral)
    if "bias" in ops:
        o["bias"] = torch.zeros(ch, dtype=torch.float64) if neutral else v["bias"].double()
    if "resid" in ops:
        o["resid"] = torch.zeros(shape, dtype=torch.float64) if neutral else v["resid"].double()
    if "mask0" in ops or "mask1" in ops:
        m = torch.ones(shape, dtype=torch.float64)
        if not neutral:
            n0 = ch if c.layout != "split" else c.n0
            if "mask0" in ops:
                m[..., :n0] = v["mask"][..., :n0].double()
            if "mask1" in ops:
                m[..., n0:] = v["mask"][..., n0:].double()
        o["mask"] = m
    if "cscale" in ops:
        s = v["cscale"].double()
        o["scale_full"] = torch.ones_like(s) if neutral else s
        o["scale"] = o["scale_full"][:, None, None, :ch]
    if "accum" in ops:
        o["seed"] = torch.zeros(shape, dtype=torch.float64) if neutral else v["seed"].double()
    return o


def epilogue64(z, o):
    """The documented epilogue of accumulators z in fp64: bias, residual, ReLU, mask, channel scale,
    accumulate."""
    y = z.double()
    if o["bias"] is not None:
        y = y + o["bias"]
    if o["resid"] is not None:
        y = y + o["resid"]
    if o["relu"]:
        y = y.clamp_min(0.0)
    if o["mask"] is not None:
        y = torch.where(o["mask"] > 0, y, torch.zeros_like(y))
    if o["scale"] is not None:
        y = y * o["scale"]
    if o["seed"] is not None:
        y = y + o["seed"]
    return y


def magnitude(z, o):
    """S = (|z| + |bias| + |resid|) * |scale| + |seed|: bounds every intermediate of the epilogue"""
    s = z.double().abs()
    if o["bias"] is not None:
        s = s + o["bias"].abs()
    if o["resid"] is not None:
        s = s + o["resid"].abs()
    if o["scale"] is not None:
        s = s * o["scale"].abs()
    if o["seed"] is not None:
        s = s + o["seed"].abs()
    return s


def gemm_ratio(got, ref):
    """max over elements of |got - ref| / (1e-5 max|ref| + 1e-4 |ref|): the fp32 conv tolerance of
    test_kernels_gpu.assert_close (<= 1 passes; NaN fails)"""
    ref = ref.double()
    tol = 1e-5 * max(ref.abs().max().item(), 1e-30) + 1e-4 * ref.abs()
    return ((got.double() - ref).abs() / tol).nan_to_num(nan=float("inf")).max().item()


def epilogue_ratio(got, z, o):
    """max |got - epilogue64(z)| / (4 * 2^-24 * S); elements with S == 0 must be exact"""
    err = (got.double() - epilogue64(z, o)).abs().nan_to_num(nan=float("inf"))
    bound = 4 * 2.0 ** -24 * magnitude(z, o)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                            torch.zeros_like(err)))
    return r.max().item()


def bf16_ratio(got, ref):
    """max |got - ref| / (2^-8 |ref| + 1.01 (1e-4 |ref| + 1e-5 max|ref|))"""
    ref = ref.double()
    d = 1e-4 * ref.abs() + 1e-5 * max(ref.abs().max().item(), 1e-30)
    return ((got.double() - ref).abs() / (2.0 ** -8 * ref.abs() + 1.01 * d)).nan_to_num(nan=float("inf")).max().item()


def check_exact(got, o):
    """What holds bit for bit whatever the accumulation order: a masked-off output is 0, or the
    seed under ACCUM; an output under ReLU is >= 0 before the (non-negative) scale, so >= 0, or
    >= the seed under ACCUM (rounding is monotone)."""
    got = got.double()
    seed = o["seed"]
    if o["mask"] is not None:
        off = ~(o["mask"] > 0)
        want = torch.zeros_like(got) if seed is None else seed
        assert torch.equal(got[off], want[off]), "a masked-off output is not exactly %s" % ("0" if seed is None else "the seed")
    if o["relu"]:
        floor = torch.zeros_like(got) if seed is None else seed
        assert bool((got >= floor).all()), "an output under ReLU is below %s" % ("0" if seed is None else "the seed")


# ------------------------------------------------------------------------------------- device runner
class Guarded:
    """numel elements inside a larger device buffer: GUARD sentinel floats before and after, the
    inner buffer 16-byte aligned or (off = 1) one float past that."""

    def __init__(self, numel, dtype, off=0):
        self.per = 4 // torch.empty(0, dtype=dtype).element_size()        # elements per float
        self.word, self.sent = (torch.int32, SENT32) if self.per == 1 else (torch.int16, SENT16)
        self.lo = (GUARD + off) * self.per
        self.numel = numel
        total = self.lo + numel + GUARD * self.per
        self.buf = torch.empty(total, dtype=dtype, device="cuda")
        self.buf.view(self.word).fill_(self.sent)
        self.inner = self.buf[self.lo:self.lo + numel]
        assert self.inner.data_ptr() % 16 == 4 * off

    def ptr(self):
        return self.inner.data_ptr()

    def intact(self):
        w = self.buf.view(self.word)
        return bool((w[:self.lo] == self.sent).all()) and bool((w[self.lo + self.numel:] == self.sent).all())


def _dev(t, dtype, off=0):
    """a device copy of CPU tensor t, 16-byte aligned or off floats past that"""
    per = 4 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.empty(t.numel() + 8 * per, dtype=dtype, device="cuda")
    view = buf[off * per:off * per + t.numel()]
    view.copy_(t.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == 4 * off
    return view


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    """Sources and packed weights of a case on the device (shared by all its forms)."""
    from punet import kernels as K
    c = CASE[name]
    v = values(name)
    dt = BF if c.entry == "bf16" else torch.float32
    _, _, k_pad, mode, _, _ = geometry(c)
    d = dict(src0=_dev(v["x0"], dt), src1=_dev(v["x1"], dt) if c.c1 else None)
    w = v["w"].cuda()
    packed = K.pack_weight(w, mode, k_pad, cgroup=c.cg, dtype=dt)
    assert not c.w6 or packed.planes is not None
    d["weight"] = packed.direct
    d["weight6"] = packed.planes if c.w6 else None
    d["wino"] = None
    if c.wino:
        d["wino"] = torch.empty(K.lib().pu_wino_bytes(c.n, c.c0 + c.c1) // 2, dtype=BF, device="cuda")
        K.pack_wino([(w, d["wino"], False)])
    d["_w"] = w
    return d


Result = collections.namedtuple("Result", "rc out plan need intact untouched")


def run(c, ops, scratch=False, neutral=False):
    """One guarded call of case c with the operands `ops`.  Destinations and workspace sit between
    sentinels; without ACCUM the destination is NaN-filled.  Returns the status, the output in the
    logical layout (CPU fp32), the plan and scratch the queries report for these very arguments,
    whether every sentinel survived and whether the destination still holds its fill bit for bit."""
    from punet import kernels as K
    fn, _, _ = _fns(c.entry)
    dt = BF if c.entry == "bf16" else torch.float32
    d = device_inputs(c.name)
    o = operands(c, ops, neutral)
    _, _, _, _, _, shape = geometry(c)
    ch = shape[3]
    n0 = c.n0 if c.layout == "split" else ch

    def sides(t):          # a logical tensor as the one or two NHWC tensors the call sees
        return [t] if c.layout != "split" else [t[..., :n0].contiguous(), t[..., n0:].contiguous()]

    fill = sides(o["seed"] if o["seed"] is not None else torch.full(shape, float("nan"), dtype=torch.float64))
    dst = []
    for i, t in enumerate(fill):
        gd = Guarded(t.numel(), dt, off=1 if (c.mis == "dst0" and i == 0) else 0)
        gd.inner.copy_(t.reshape(-1).to(dt))
        dst.append(gd)
    before = [gd.inner.clone() for gd in dst]
    keep = [d]             # device operands stay referenced until the call has finished
    ptr = {k: (None if d[k] is None else d[k].data_ptr()) for k in ("src0", "src1", "weight", "weight6", "wino")}
    ptr.update(dst0=dst[0].ptr(), dst1=dst[1].ptr() if len(dst) > 1 else None, bias=None, mask0=None, mask1=None,
               resid=None, cscale=None)
    if o["bias"] is not None:
        keep.append(_dev(o["bias"], torch.float32, off=1 if c.mis == "bias" else 0))
        ptr["bias"] = keep[-1].data_ptr()
    if o["resid"] is not None:
        keep.append(_dev(o["resid"], dt))
        ptr["resid"] = keep[-1].data_ptr()
    if o["mask"] is not None:
        for i, m in enumerate(sides(o["mask"])):
            if "mask%d" % i in ops:
                keep.append(_dev(m, dt, off=1 if (c.mis == "mask0" and i == 0) else 0))
                ptr["mask%d" % i] = keep[-1].data_ptr()
    if o["scale"] is not None:
        keep.append(_dev(o["scale_full"], torch.float32))
        ptr["cscale"] = keep[-1].data_ptr()
    if neutral:
        ops = ops - {"relu"}
    a = conv_args(c, ops, ptr)
    _, need = plan_of(c, a)
    ws = None
    if scratch:
        assert need > 0 and need % 4 == 0, need
        ws = Guarded(need // 4, torch.float32)
        ws.inner.fill_(float("nan"))
        a = conv_args(c, ops, ptr, (ws.ptr(), need))
    plan, need2 = plan_of(c, a)
    assert need2 == need
    rc = fn(ctypes.byref(a), K._stream())
    torch.cuda.synchronize()
    intact = all(gd.intact() for gd in dst) and (ws is None or ws.intact())
    word = dst[0].word
    untouched = all(torch.equal(gd.inner.view(word), b.view(word)) for gd, b in zip(dst, before))
    parts = [gd.inner.float().cpu().reshape(t.shape) for gd, t in zip(dst, fill)]
    out = parts[0] if len(parts) == 1 else torch.cat(parts, 3)
    del keep
    return Result(rc, out, plan, need, intact, untouched)
