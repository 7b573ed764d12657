"""torch-tensor wrappers over the C-ABI kernels (one wrapper per entry point of plastic_unet.h).

Every wrapper enqueues on torch's *current* HIP stream and never synchronises.  Tensors must be
fp32, contiguous and resident on the ROCm device; activations are NHWC.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import packs     # PackedWeight, the operand pack_weight makes and igemm reads (packs calls back into here)
from ._lib import (ConvArgs, WgradArgs, PlasticArgs, PlasticHeadArgs, PlasticBwdArgs, PlasticBwdTraceArgs, AdamTensor,
                   PackJob, WinoJob, check,
                   PU_EPI_RELU, PU_EPI_ACCUM, PU_EPI_SHUFFLE2, PU_EPI_RESID, PU_CONV_NO_HALO, PU_CONV_HALO_V1,
                   PU_CONV_NO_SMALLX6, PU_EPI_OUT_BF16)

__all__ = ["KernelProfiler", "igemm", "wgrad", "pack_weight", "nchw_to_nhwc", "maxpool2_fwd", "maxpool2_bwd",
           "outconv_fwd", "outconv_bwd", "plastic_fwd", "trace_update", "plastic_bwd", "plastic_bwd_trace", "bce_fwd",
           "bce_bwd", "seg_metrics", "rle_encode", "augment", "flip_mean", "fit", "lovasz_fwd", "lovasz_bwd", "adam_multi", "grad_norm", "pack_weights", "round16", "cgroup_for", "device_info", "lib"]


def lib():
    return _lib.load()


# ------------------------------------------------------------------------------ launch profiler
_PROF = None
_MODES = {0: "chunk16", 1: "vec4", 2: "scalar", 3: "direct", 4: "x6", 5: "stem", 6: "wino", 7: "x6s"}

# fp32 GEMM arithmetic of the MFMA convolutions: "split6" (default) = each fp32 product as 6 exact
# bf16 products on the bf16 MFMA pipe (pu_split_weight6 / pu_conv_args.weight6, fp32-accurate);
# "native" = v_mfma_f32_32x32x2_f32.  Read when a weight is packed and when a conv launches.
_FP32_MATH = os.environ.get("PU_FP32_MATH", "split6")


# bf16 3x3/s1 convolutions of width 32/64/128: on = the halo and row-stream kernels (default, as
# at the C-ABI), off = the per-tap lean kernel (PU_CONV_HALO=0: A/B runs; tests flip it with
# set_conv_halo)
_CONV_HALO = os.environ.get("PU_CONV_HALO", "1") != "0"


def set_conv_halo(on):
    """Route eligible bf16 convolutions: 1 (or True) halo and row-stream kernels - the default, as
    at the C-ABI -, 0 (or False) per-tap kernel.  Returns the previous setting (1 or 0)."""
    global _CONV_HALO
    if isinstance(on, str) or on not in (0, 1):
        raise ValueError("set_conv_halo: 1 / True (halo and rows) or 0 / False (per-tap), not %r" % (on,))
    prev, _CONV_HALO = int(_CONV_HALO), bool(on)
    return prev


def _halo_flags():
    return 0 if _CONV_HALO else PU_CONV_NO_HALO


def fp32_math():
    return _FP32_MATH


# fp32 3x3/s1/p1 convolutions (forward and data gradient) on the Winograd F(2x2,3x3) kernel where
# the layer qualifies (PU_WINO=0: the direct 6-product kernels everywhere; A/B runs, tests flip it
# with set_wino)
_WINO = os.environ.get("PU_WINO", "1") != "0"


# fp32 8/16-channel 3x3 convolutions on the 16x16x32 MFMA kernel (csrc/smallconv.hip) or the VALU
# direct kernel (PU_SMALLX6=0; tests flip it with set_smallx6)
_SMALLX6 = os.environ.get("PU_SMALLX6", "1") != "0"


def set_smallx6(on):
    """Route 8/16-channel fp32 3x3 convolutions to the MFMA kernel (True) or the VALU direct one."""
    global _SMALLX6
    prev, _SMALLX6 = _SMALLX6, bool(on)
    return prev


def set_wino(on):
    """Route eligible fp32 3x3 convolutions to the Winograd kernel (True) or the direct kernels.
    Returns the previous setting."""
    global _WINO
    prev, _WINO = _WINO, bool(on)
    return prev


def wino_wanted(w, mode):
    """Whether a packed conv operand of parameter w (OIHW 3x3) should carry a Winograd operand:
    the reduced channel count a multiple of 32 and the produced one of 64 (the kernel's chunks
    and output blocks)."""
    if mode not in (0, 1) or w.dim() != 4 or w.shape[2:] != (3, 3) or _FP32_MATH != "split6":
        return False
    n, c = (w.shape[0], w.shape[1]) if mode == 0 else (w.shape[1], w.shape[0])
    # mirrors csrc/winograd.hip wino_ok / wino_wide_items: a short reduction (c < 128) into more
    # than 64 outputs runs only as wide 128-channel items
    return c % 32 == 0 and n % 64 == 0 and (c >= 128 or n <= 64 or n % 128 == 0)


def pack_wino(jobs):
    """pu_pack_wino: jobs = [(w, out, dgrad)] - U = G g G^T of each OIHW weight, exact bf16 planes."""
    if not jobs:
        return
    arr = (WinoJob * len(jobs))()
    nbytes = 0.0
    for i, (w, out, dgrad) in enumerate(jobs):
        _req(w, "w")
        arr[i] = WinoJob(w.data_ptr(), out.data_ptr(), w.shape[0], w.shape[1], int(dgrad))
        nbytes += 4.0 * w.numel() + 2.0 * out.numel()
    with _Rec("pack_wino", nbytes=nbytes):
        check(lib().pu_pack_wino(arr, len(jobs), _stream()), "pu_pack_wino")


def set_fp32_math(mode):
    """'split6' or 'native' (tests / ablations).  Returns the previous mode."""
    global _FP32_MATH
    if mode not in ("split6", "native"):
        raise ValueError("fp32 math must be 'split6' or 'native', got %r" % (mode,))
    prev, _FP32_MATH = _FP32_MATH, mode
    return prev


class KernelProfiler:
    """Brackets every wrapped launch with HIP events on the stream it is launched on, tagged with
    the kernel instantiation and its algorithmic FLOPs / bytes.  Use as a context manager."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _PROF
        self._prev, _PROF = _PROF, self
        return self

    def __exit__(self, *exc):
        global _PROF
        _PROF = self._prev
        return False

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(tag, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


class _Rec:
    __slots__ = ("tag", "flops", "nbytes", "e0")

    def __init__(self, tag, flops=0.0, nbytes=0.0):
        self.tag, self.flops, self.nbytes = tag, flops, nbytes
        self.e0 = None

    def __enter__(self):
        if _PROF is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _PROF is not None and self.e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _PROF.records.append((self.tag, self.flops, self.nbytes, self.e0, e1))
        return False


def _p(t):
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current stream's raw handle.  torch.cuda.current_stream() resolves the device through
    torch.cuda.is_available() and an environment lookup on every call (~2 us of host time, several
    hundred calls per training step); the raw accessor takes the device index directly."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


def round16(k):
    return (k + 15) // 16 * 16


def _req(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("%s must be on the ROCm device (got %s); the plastic U-Net path has no CPU "
                           "fallback" % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


BF16 = torch.bfloat16


def _act_dtype(t):
    """Activation dtype of a call: float32, or bfloat16 for the bf16 (C3) entry points."""
    return BF16 if t.dtype == BF16 else torch.float32


def device_info(device=0):
    L = lib()
    cu, clk, mem = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    check(L.pu_device_info(device, ctypes.byref(cu), ctypes.byref(clk), ctypes.byref(mem)), "pu_device_info")
    return cu.value, clk.value, mem.value


def cgroup_for(c0, c1=0):
    """K order for a packed conv operand: 32-channel groups when both sources allow it."""
    if c0 % 32 == 0 and c1 % 32 == 0:
        return 32
    if c0 % 16 == 0 and c1 % 16 == 0:
        return 16
    return 0


_WINO_TAKES = {}    # call signature -> does pu_conv_igemm take the Winograd kernel for it


def direct_call(weight):
    """A call on this operand is about to take a direct kernel: its direct operand is repacked
    first if the last repack skipped it, and refreshed with every repack from now on."""
    if weight.take_direct():
        pack_weights([weight], wino=False)


def igemm(*, batch, in_hw, out_hw, k, stride, pad, src0, c0, weight, k_pad, n, dst0, n0=None,
          src1=None, c1=0, bias=None, dst1=None, mask0=None, mask1=None, relu=False, accum=False,
          shuffle=False, cgroup=0, resid=None, shuf=(0, 0, 0), chan_scale=None):
    """pu_conv_igemm: implicit-GEMM conv (3x3 fwd/dgrad, ConvT fwd with shuffle, ConvT dgrad).
    resid: residual tensor added before ReLU/mask; shuf = (out_h, out_w, crop) of a SHUFFLE2 grid;
    chan_scale: [batch, ld] per-(image, column) factors applied after the mask (the Dropout2d scale
    of the tensor being produced; SHUFFLE2: per output channel).  A bf16 dst0 with fp32 operands
    is the single-channel stem writing the bf16 trunk's first activation (PU_EPI_OUT_BF16).
    weight: the packs.PackedWeight of the parameter (pack_weight, or the trunk's Packs cache)."""
    if not isinstance(weight, packs.PackedWeight):
        raise TypeError("weight must be a PackedWeight (pack_weight or Packs.get), not %s" % type(weight).__name__)
    dt = _act_dtype(src0)
    out_bf16 = dt == torch.float32 and dst0 is not None and dst0.dtype == BF16
    for t, nm in ((src0, "src0"), (src1, "src1"), (weight.direct, "weight"), (dst0, "dst0"),
                  (dst1, "dst1"), (mask0, "mask0"), (mask1, "mask1"), (resid, "resid")):
        _req(t, nm, BF16 if (out_bf16 and nm == "dst0") else dt)
    _req(bias, "bias")
    _req(chan_scale, "chan_scale")
    flags = (PU_EPI_RELU if relu else 0) | (PU_EPI_ACCUM if accum else 0) | (PU_EPI_SHUFFLE2 if shuffle else 0) \
        | (PU_EPI_RESID if resid is not None else 0) | _halo_flags() | (0 if _SMALLX6 else PU_CONV_NO_SMALLX6) \
        | (PU_EPI_OUT_BF16 if out_bf16 else 0)
    a = ConvArgs(batch, in_hw[0], in_hw[1], out_hw[0], out_hw[1], k, k, stride, pad,
                 _p(src0), c0, _p(src1), c1, weight.data_ptr(), k_pad, cgroup, n, _p(bias),
                 _p(dst0), n if n0 is None else n0, _p(dst1), _p(mask0), _p(mask1), flags, None, 0,
                 _p(resid), shuf[0], shuf[1], shuf[2])
    if chan_scale is not None:
        if chan_scale.dim() != 2 or chan_scale.shape[0] != batch:
            raise RuntimeError("chan_scale must be [batch, channels]")
        a.chan_scale, a.chan_scale_ld = chan_scale.data_ptr(), chan_scale.shape[1]
    w6 = weight.planes if (dt != BF16 and _FP32_MATH == "split6") else None
    wn = weight.wino if (w6 is not None and _WINO) else None
    if w6 is not None:
        a.weight6 = w6.data_ptr()
    if wn is not None:
        a.wino = wn.data_ptr()
    L = lib()
    if weight.state != packs.KEPT:
        # an operand that has only ever run on the Winograd kernel, so the last repack may have
        # skipped its direct operand: does this call take the Winograd kernel too?
        takes = False       # not without U (Winograd switched off, native fp32 math)
        if wn is not None:
            # the signature wino_ok reads: shapes, flags, which operands exist, their alignment
            key = (batch, tuple(in_hw), tuple(out_hw), k, stride, pad, c0, c1, n, a.n0, k_pad, cgroup, flags,
                   tuple(None if t is None else t.data_ptr() % 16 for t in
                         (src0, src1, bias, dst0, dst1, mask0, mask1, resid, chan_scale, weight.direct, w6, wn)))
            takes = _WINO_TAKES.get(key)
            if takes is None:       # the library's answer, cached per signature
                bm, bn, mode, ks = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                check(L.pu_conv_igemm_tile(ctypes.byref(a), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(mode),
                                           ctypes.byref(ks)), "pu_conv_igemm_tile")
                takes = _WINO_TAKES[key] = mode.value == 6
        if not takes:
            direct_call(weight)
    if dt == BF16:
        _igemm_bf16(L, a, batch, out_hw, k, c0, c1, n, dst0)
        return
    nbytes = L.pu_conv_igemm_workspace_bytes(ctypes.byref(a))
    if nbytes:     # split-K scratch from the caching allocator (stream-ordered reuse)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dst0.device)
        a.workspace, a.ws_bytes = ws.data_ptr(), nbytes
    if _PROF is None:
        check(L.pu_conv_igemm(ctypes.byref(a), _stream()), "pu_conv_igemm")
        return
    bm, bn, mode, ks = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.pu_conv_igemm_tile(ctypes.byref(a), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(mode), ctypes.byref(ks))
    M = batch * out_hw[0] * out_hw[1]
    tag = "igemm<%dx%d,%s%s>" % (bm.value, bn.value, _MODES[mode.value], ",k%d" % ks.value if ks.value > 1 else "")
    nb = 0.0
    if mode.value in (3, 5, 7):    # small-channel / stem kernels: HBM-bound, report algorithmic bytes
        per = (c0 + c1) + n * (1 + int(accum) + int(resid is not None)) + n0_mask(n, n0, mask0, mask1)
        nb = 4.0 * M * per
    with _Rec(tag, flops=2.0 * M * n * k * k * (c0 + c1), nbytes=nb):
        check(L.pu_conv_igemm(ctypes.byref(a), _stream()), "pu_conv_igemm")


def n0_mask(n, n0, mask0, mask1):
    """channels of the ReLU masks an igemm epilogue reads"""
    n0 = n if n0 is None else n0
    return (n0 if mask0 is not None else 0) + (n - n0 if mask1 is not None else 0)


def _igemm_bf16(L, a, batch, out_hw, k, c0, c1, n, dst0):
    nbytes = L.pu_conv_igemm_bf16_workspace_bytes(ctypes.byref(a))
    if nbytes:
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dst0.device)
        a.workspace, a.ws_bytes = ws.data_ptr(), nbytes
    if _PROF is None:
        check(L.pu_conv_igemm_bf16(ctypes.byref(a), _stream()), "pu_conv_igemm_bf16")
        return
    bm, bn, ks, kind = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.pu_conv_igemm_bf16_tile(ctypes.byref(a), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(ks), ctypes.byref(kind))
    M = batch * out_hw[0] * out_hw[1]
    tag = "igemm_bf16<%dx%d%s%s>" % (bm.value, bn.value, ("", ",lean", ",halo", ",rows")[kind.value],
                                     ",k%d" % ks.value if ks.value > 1 else "")
    with _Rec(tag, flops=2.0 * M * n * k * k * (c0 + c1)):
        check(L.pu_conv_igemm_bf16(ctypes.byref(a), _stream()), "pu_conv_igemm_bf16")


def wgrad_args(*, batch, in_hw, out_hw, k, stride, pad, rows, n, src0, c0, dweight, src1=None, c1=0,
               bias_mode=0, dbias=None, accumulate=False, math=None):
    """The pu_wgrad_args of one kxk weight gradient.  rows, src0, src1, dweight and dbias are device
    addresses (None: absent); math None is the fp32 arithmetic PU_FP32_MATH selects."""
    if math is None:
        math = 1 if _FP32_MATH == "split6" else 0
    return WgradArgs(batch, in_hw[0], in_hw[1], out_hw[0], out_hw[1], k, k, stride, pad,
                     rows, n, src0, c0, src1, c1, bias_mode, dweight, dbias, 1 if accumulate else 0, math)


def wgrad(*, batch, in_hw, out_hw, k, stride, pad, rows, n, src0, c0, dweight, src1=None, c1=0,
          bias_mode=0, dbias=None, accumulate=False):
    """pu_wgrad: split-K weight (+bias) gradient into PyTorch's [n][c][k][k] layout (fp32, or
    bf16 rows/sources with fp32 gradients)."""
    # bf16 dZ with an fp32 single-channel source: the bf16 trunk's stem (pu_wgrad math 2)
    stem_bf16 = rows.dtype == BF16 and src0.dtype == torch.float32 and c0 == 1 and src1 is None
    dt = torch.float32 if stem_bf16 else _act_dtype(rows)
    for t, nm in ((rows, "rows"), (src0, "src0"), (src1, "src1")):
        _req(t, nm, BF16 if (stem_bf16 and nm == "rows") else dt)
    _req(dweight, "dweight"); _req(dbias, "dbias")
    a = wgrad_args(batch=batch, in_hw=in_hw, out_hw=out_hw, k=k, stride=stride, pad=pad, rows=_p(rows), n=n,
                   src0=_p(src0), c0=c0, src1=_p(src1), c1=c1, bias_mode=bias_mode, dweight=_p(dweight),
                   dbias=_p(dbias), accumulate=accumulate, math=2 if stem_bf16 else 0 if dt == BF16 else None)
    name = "pu_wgrad_bf16" if dt == BF16 else "pu_wgrad"
    run, phase, tile, ws_bytes = (getattr(lib(), name + sfx) for sfx in ("", "_phase", "_tile", "_workspace_bytes"))
    nbytes = ws_bytes(ctypes.byref(a))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=rows.device)
    if nbytes == 0 or _PROF is None:          # (0: the arguments were refused, and run says why)
        check(run(ctypes.byref(a), ws.data_ptr(), nbytes, _stream()), name)
        return
    bn, bk, kind = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(tile(ctypes.byref(a), ctypes.byref(bn), ctypes.byref(bk), ctypes.byref(kind), None), name + "_tile")
    if dt == BF16:
        tag = "wgrad_bf16<%dx%d%s>" % (bn.value, bk.value, ",halo" if kind.value else "")
    else:
        tag = "wgrad<%dx%d,%s>" % (bn.value, bk.value,
                                   ("scalar", "vec4", "direct", "halo", "stem", "wino", "pointwise")[kind.value])
        if a.math == 1 and kind.value in (1, 3, 5):
            tag = tag[:-1] + ",x6>"
    M = batch * out_hw[0] * out_hw[1]
    # the GEMM and the split reduction timed apart (they are separate kernels in rocprof too)
    with _Rec(tag, flops=2.0 * M * n * k * k * (c0 + c1)):
        check(phase(ctypes.byref(a), ws.data_ptr(), nbytes, 1, _stream()), name + "_phase")
    with _Rec("wgrad_reduce", nbytes=float(nbytes)):
        check(phase(ctypes.byref(a), ws.data_ptr(), nbytes, 2, _stream()), name + "_phase")


def wgrad_kind(*, batch, hw, n, c0, c1=0, k=3):
    """Which kernel pu_wgrad takes for an fp32 kxk/s1 same-size ('same' padding) weight gradient
    (pu_wgrad_tile's loader kind: 1 float4 GEMM, 2 small-channel direct, 3 halo, 4 stem,
    5 Winograd-domain, 6 pointwise)."""
    a = wgrad_args(batch=batch, in_hw=hw, out_hw=hw, k=k, stride=1, pad=(k - 1) // 2, rows=16, n=n, src0=16, c0=c0,
                   src1=16 if c1 else None, c1=c1, bias_mode=1, dweight=16, dbias=16)
    bn, bk, qv, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().pu_wgrad_tile(ctypes.byref(a), ctypes.byref(bn), ctypes.byref(bk), ctypes.byref(qv), ctypes.byref(sp)),
          "pu_wgrad_tile")
    return qv.value


def pack_weight(w, mode, k_pad, cgroup=0, dtype=torch.float32):
    """Pack an fp32 parameter into its GEMM operands (fp32, or bf16 for the C3 kernels): a
    packs.PackedWeight holding the direct operand and, for fp32 split6 math, its bf16 planes and
    the Winograd operand of a 3x3 conv that qualifies."""
    _req(w, "w")
    d0, d1, kh, kw = w.shape
    taps = kh * kw
    rows = {0: d0, 1: d1, 2: taps * d1, 3: d0, 4: 4 * d1}[mode]
    direct = torch.empty(rows, k_pad, dtype=dtype, device=w.device)
    fn = lib().pu_pack_weight_bf16 if dtype == BF16 else lib().pu_pack_weight
    with _Rec("pack_weight", nbytes=4.0 * w.numel() + direct.element_size() * direct.numel()):
        check(fn(w.data_ptr(), direct.data_ptr(), mode, d0, d1, kh, kw, k_pad, cgroup, _stream()), "pu_pack_weight")
    planes = wino = None
    if dtype == torch.float32 and _FP32_MATH == "split6" and k_pad % 16 == 0:
        planes = split_weight6(direct)
        # U only while Winograd dispatch is on, so a PU_WINO=0 run neither holds nor refreshes it
        # (set_wino before packing to switch)
        if _WINO and wino_wanted(w, mode):
            n, c = (d0, d1) if mode == 0 else (d1, d0)
            wino = torch.empty(lib().pu_wino_bytes(n, c) // 2, dtype=BF16, device=w.device)
            pack_wino([(w, wino, mode == 1)])
    return packs.PackedWeight(w, mode, k_pad, cgroup, direct, planes, wino)


def pack_weights(jobs, wino=True):
    """Refresh many packed operands (PackedWeight) from their parameters in one launch
    (pu_pack_weights: direct and planes).  wino: also refresh the Winograd operands they carry (one
    more launch)."""
    if not jobs:
        return
    arr = (PackJob * len(jobs))()
    nbytes = 0.0
    for i, p in enumerate(jobs):
        w, packed, planes = p.src, p.direct, p.planes
        _req(w, "w")
        d0, d1, kh, kw = w.shape
        bf = p.dtype == BF16
        arr[i] = PackJob(w.data_ptr(), None if bf else packed.data_ptr(), packed.data_ptr() if bf else None,
                         None if planes is None else planes.data_ptr(), p.mode, d0, d1, kh, kw, p.k_pad, p.cgroup)
        nbytes += 4.0 * w.numel() + packed.element_size() * packed.numel() + (0 if planes is None else 2.0 * planes.numel())
    with _Rec("pack_weight", nbytes=nbytes):
        check(lib().pu_pack_weights(arr, len(jobs), _stream()), "pu_pack_weights")
    for p in jobs:
        p.direct_repacked()
    if wino:
        pack_wino([(p.src, p.wino, p.mode == 1) for p in jobs if p.wino is not None])


def split_weight6(packed):
    """packed fp32 [n][k_pad] (or the PackedWeight holding it as direct) -> bf16 planes
    [k_pad/16][6][n][8] (hi/mid/lo, exact split)."""
    if isinstance(packed, packs.PackedWeight):
        packed = packed.direct
    _req(packed, "packed")
    n, k_pad = packed.shape
    out = torch.empty(k_pad // 16, 6, n, 8, dtype=BF16, device=packed.device)
    with _Rec("pack_weight", nbytes=4.0 * packed.numel() + 6.0 * packed.numel()):
        check(lib().pu_split_weight6(packed.data_ptr(), out.data_ptr(), n, k_pad, _stream()), "pu_split_weight6")
    return out


def to_bf16(x):
    _req(x, "x")
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    with _Rec("convert", nbytes=6.0 * x.numel()):
        check(lib().pu_convert_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "pu_convert_f32_bf16")
    return y


def to_f32(x):
    _req(x, "x", BF16)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with _Rec("convert", nbytes=6.0 * x.numel()):
        check(lib().pu_convert_bf16_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "pu_convert_bf16_f32")
    return y


def nchw_to_nhwc(x):
    _req(x, "x")
    B, C, H, W = x.shape
    out = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
    check(lib().pu_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), B, C, H, W, _stream()), "pu_nchw_to_nhwc")
    return out


def channel_scale(x, scale, out=None):
    """Dropout2d on NHWC x [B,H,W,C] with per-(sample, channel) scale [B,C]; out may be x."""
    _req(x, "x"); _req(scale, "scale")
    B, H, W, C = x.shape
    y = torch.empty_like(x) if out is None else out
    with _Rec("channel_scale", nbytes=8.0 * x.numel()):
        check(lib().pu_channel_scale(x.data_ptr(), scale.data_ptr(), y.data_ptr(), B, H * W, C, _stream()),
              "pu_channel_scale")
    return y


def add_coords(x, with_r):
    """NCHW input [B,C,H,W] -> NHWC [B,H,W,C+2(+1)] with the AddCoords channels appended."""
    _req(x, "x")
    B, C, H, W = x.shape
    out = torch.empty(B, H, W, C + 2 + int(with_r), dtype=torch.float32, device=x.device)
    with _Rec("add_coords", nbytes=4.0 * (x.numel() + out.numel())):
        check(lib().pu_add_coords(x.data_ptr(), out.data_ptr(), B, C, H, W, int(with_r), _stream()), "pu_add_coords")
    return out


def column_sum(x2d, out=None, accumulate=False):
    """Deterministic fp64 column sums of a row-major [rows, cols] tensor."""
    _req(x2d, "x")
    rows, cols = x2d.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x2d.device)
    L = lib()
    nbytes = L.pu_column_sum_workspace_bytes(rows, cols)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x2d.device)
    with _Rec("column_sum", nbytes=4.0 * x2d.numel()):
        check(L.pu_column_sum(x2d.data_ptr(), rows, cols, out.data_ptr(), int(accumulate), ws.data_ptr(), nbytes,
                              _stream()), "pu_column_sum")
    return out


def maxpool2_fwd(x, scale=None):
    """MaxPool2d(2); scale [B, C] (fp32 only): the Dropout2d that follows the pool, fused."""
    dt = _act_dtype(x)
    _req(x, "x", dt)
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, C, dtype=dt, device=x.device)
    with _Rec("maxpool_fwd", nbytes=x.element_size() * (x.numel() + y.numel())):
        if scale is not None:
            _req(x, "x"); _req(scale, "scale")       # fp32 entry point
            check(lib().pu_maxpool2_fwd_scaled(x.data_ptr(), scale.data_ptr(), y.data_ptr(), B, H, W, C, _stream()),
                  "pu_maxpool2_fwd_scaled")
        else:
            fn = lib().pu_maxpool2_fwd_bf16 if dt == BF16 else lib().pu_maxpool2_fwd
            check(fn(x.data_ptr(), y.data_ptr(), B, H, W, C, _stream()), "pu_maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy, dx, relu_mask=True, accumulate=True, scale=None):
    """MaxPool2d(2) backward; scale [B, C] (fp32 only): dy * scale routed (the Dropout2d backward)."""
    dt = _act_dtype(x)
    _req(x, "x", dt); _req(dy, "dy", dt); _req(dx, "dx", dt)
    B, H, W, C = x.shape
    with _Rec("maxpool_bwd", nbytes=x.element_size() * (x.numel() * (3 if accumulate else 2) + dy.numel())):
        if scale is not None:
            _req(x, "x"); _req(scale, "scale")       # fp32 entry point
            check(lib().pu_maxpool2_bwd_scaled(x.data_ptr(), dy.data_ptr(), scale.data_ptr(), dx.data_ptr(), B, H, W,
                                               C, int(relu_mask), int(accumulate), _stream()), "pu_maxpool2_bwd_scaled")
        else:
            fn = lib().pu_maxpool2_bwd_bf16 if dt == BF16 else lib().pu_maxpool2_bwd
            check(fn(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, C, int(relu_mask), int(accumulate),
                     _stream()), "pu_maxpool2_bwd")
    return dx


def outconv_fwd(x, w, b):
    """x [B,H,W,C] NHWC, w [C] (flattened [1,C,1,1]), b [1] -> logits [B,H,W]."""
    dt = _act_dtype(x)
    _req(x, "x", dt); _req(w, "w"); _req(b, "b")
    B, H, W, C = x.shape
    y = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    fn = lib().pu_outconv_fwd_bf16 if dt == BF16 else lib().pu_outconv_fwd
    with _Rec("outconv_fwd", nbytes=x.element_size() * x.numel() + 4.0 * y.numel()):
        check(fn(x.data_ptr(), w.data_ptr(), _p(b), y.data_ptr(), B * H * W, C, _stream()), "pu_outconv_fwd")
    return y


def outconv_bwd(x, w, dy, relu_mask=True, out=None):
    dt = _act_dtype(x)
    _req(x, "x", dt); _req(w, "w"); _req(dy, "dy")
    B, H, W, C = x.shape
    rows = B * H * W
    dx = torch.empty_like(x)
    if out is None:
        dw = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(1, dtype=torch.float32, device=x.device)
    else:
        dw, db = out
    L = lib()
    nbytes = L.pu_outconv_workspace_bytes(rows, C)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x.device)
    fn = L.pu_outconv_bwd_bf16 if dt == BF16 else L.pu_outconv_bwd
    with _Rec("outconv_bwd", nbytes=x.element_size() * 2.0 * x.numel() + 4.0 * rows):
        check(fn(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                 rows, C, int(relu_mask), ws.data_ptr(), nbytes, _stream()), "pu_outconv_bwd")
    return dx, dw, db


def plastic_fwd(x, hebb, w, alpha, eta, rule, update_trace=True):
    """x, hebb [B,N,N] -> (y [B,N,N], hebb' [B,N,N] or None)."""
    for t, nm in ((x, "x"), (hebb, "hebb"), (w, "w"), (alpha, "alpha"), (eta, "eta")):
        _req(t, nm)
    B, N, _ = x.shape
    y = torch.empty_like(x)
    hn = torch.empty_like(hebb) if update_trace else None
    a = PlasticArgs(B, N, x.data_ptr(), hebb.data_ptr(), w.data_ptr(), alpha.data_ptr(), eta.data_ptr(),
                    y.data_ptr(), _p(hn), rule)
    with _Rec("plastic_fwd", flops=2.0 * B * N ** 3, nbytes=4.0 * (4 * B * N * N + 2 * N * N)):
        check(lib().pu_plastic_fwd(ctypes.byref(a), _stream()), "pu_plastic_fwd")
    return y, hn


def plastic_head_fwd(feat, wo, bo, hebb, w, alpha, eta, rule, update_trace=True):
    """The fused head (pu_plastic_head_fwd): feat [B,N,N,C] NHWC (fp32 / bf16), wo [C], bo [1] ->
    (X [B,N,N] logits, Y [B,N,N], hebb' [B,N,N] or None)."""
    dt = _act_dtype(feat)
    _req(feat, "feat", dt)
    for t, nm in ((wo, "wo"), (bo, "bo"), (hebb, "hebb"), (w, "w"), (alpha, "alpha"), (eta, "eta")):
        _req(t, nm)
    B, N, _, C = feat.shape
    X = torch.empty(B, N, N, dtype=torch.float32, device=feat.device)
    y = torch.empty_like(X)
    hn = torch.empty_like(hebb) if update_trace else None
    a = PlasticHeadArgs(B, N, C, feat.data_ptr(), int(dt == BF16), wo.data_ptr(), bo.data_ptr(), hebb.data_ptr(),
                        w.data_ptr(), alpha.data_ptr(), eta.data_ptr(), X.data_ptr(), y.data_ptr(), _p(hn), rule)
    nbytes = feat.element_size() * feat.numel() + 4.0 * (4 * B * N * N + 2 * N * N)
    with _Rec("plastic_head_fwd", flops=2.0 * B * N ** 3 + 2.0 * B * N * N * C, nbytes=nbytes):
        check(lib().pu_plastic_head_fwd(ctypes.byref(a), _stream()), "pu_plastic_head_fwd")
    return X, y, hn


def trace_update(hebb, x, y, eta, rule, out=None):
    for t, nm in ((hebb, "hebb"), (x, "x"), (y, "y"), (eta, "eta")):
        _req(t, nm)
    B, N, _ = hebb.shape
    out = torch.empty_like(hebb) if out is None else out
    with _Rec("trace_update", nbytes=8.0 * B * N * N + 8.0 * B * N):
        _trace(hebb, x, y, eta, out, B, N, rule)
    return out


def _trace(hebb, x, y, eta, out, B, N, rule):
    check(lib().pu_trace_update(hebb.data_ptr(), x.data_ptr(), y.data_ptr(), eta.data_ptr(), out.data_ptr(), B, N,
                                rule, _stream()), "pu_trace_update")


def plastic_bwd(x, hebb, w, alpha, y, dy, need_dx=True, need_dw=True, out=None):
    for t, nm in ((x, "x"), (hebb, "hebb"), (w, "w"), (alpha, "alpha"), (y, "y"), (dy, "dy")):
        _req(t, nm)
    B, N, _ = x.shape
    dx = torch.empty_like(x) if need_dx else None
    if out is not None and need_dw:
        dw, da = out
    else:
        dw = torch.empty_like(w) if need_dw else None
        da = torch.empty_like(alpha) if need_dw else None
    L = lib()
    nbytes = L.pu_plastic_bwd_workspace_bytes(B, N)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x.device) if need_dw else None
    a = PlasticBwdArgs(B, N, x.data_ptr(), hebb.data_ptr(), w.data_ptr(), alpha.data_ptr(), y.data_ptr(),
                       dy.data_ptr(), _p(dx), _p(dw), _p(da))
    with _Rec("plastic_bwd", flops=4.0 * B * N ** 3):
        check(L.pu_plastic_bwd(ctypes.byref(a), _p(ws), nbytes if need_dw else 0, _stream()), "pu_plastic_bwd")
    return dx, dw, da


def plastic_bwd_trace_bytes(B, N, has_p=True, need_dh=True):
    """HBM floor of pu_plastic_bwd_trace beyond the head backward: P and H read once by the trace
    backward (8 B N^2), P, T_b, alpha in and dH out for the dH finish (16 B N^2)."""
    return (8.0 * B * N * N if has_p else 0.0) + (16.0 * B * N * N if need_dh else 0.0)


def plastic_bwd_trace(x, hebb, w, alpha, eta, y, dy, dhebb_out, rule, need_dx=True, need_dw=True, need_dh=True):
    """The head backward with the gradient of the updated trace (pu_plastic_bwd_trace).

    dy [B,N,N] or None (zeros), dhebb_out = dL/dH' [B,N,N] or None -> (dx, dw, dalpha, dhebb, deta);
    outputs not asked for are None, deta [1] is None without dhebb_out."""
    for t, nm in ((x, "x"), (hebb, "hebb"), (w, "w"), (alpha, "alpha"), (eta, "eta"), (y, "y"), (dy, "dy"),
                  (dhebb_out, "dhebb_out")):
        _req(t, nm)
    if dy is None and dhebb_out is None:
        raise ValueError("plastic_bwd_trace: neither dy nor dhebb_out")
    B, N, _ = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dw else None
    da = torch.empty_like(alpha) if need_dw else None
    dh = torch.empty_like(hebb) if need_dh else None
    deta = torch.empty_like(eta) if dhebb_out is not None else None
    L = lib()
    nbytes = L.pu_plastic_bwd_trace_workspace_bytes(B, N)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x.device)
    a = PlasticBwdTraceArgs(B, N, rule, x.data_ptr(), hebb.data_ptr(), w.data_ptr(), alpha.data_ptr(), eta.data_ptr(),
                            y.data_ptr(), _p(dy), _p(dhebb_out), _p(dx), _p(dw), _p(da), _p(dh), _p(deta))
    head = 4.0 * (5 * B * N * N + 2 * N * N) + (8.0 * B * N * N + 8.0 * N * N if need_dw or need_dh else 0.0)
    with _Rec("plastic_bwd_trace", flops=4.0 * B * N ** 3 + 8.0 * B * N * N,
              nbytes=head + plastic_bwd_trace_bytes(B, N, dhebb_out is not None, need_dh)):
        check(L.pu_plastic_bwd_trace(ctypes.byref(a), ws.data_ptr(), nbytes, _stream()), "pu_plastic_bwd_trace")
    return dx, dw, da, dh, deta


def bce_fwd(y, t):
    _req(y, "y"); _req(t, "t")
    n = y.numel()
    if t.numel() != n:
        raise ValueError("Target size (%s) must be the same as input size (%s)" % (tuple(t.shape), tuple(y.shape)))
    L = lib()
    nbytes = L.pu_bce_workspace_bytes(n)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    check(L.pu_bce_fwd(y.data_ptr(), t.data_ptr(), n, loss.data_ptr(), ws.data_ptr(), nbytes, _stream()), "pu_bce_fwd")
    return loss


def bce_bwd(y, t, grad_loss):
    _req(y, "y"); _req(t, "t")
    dy = torch.empty_like(y)
    g = grad_loss.contiguous() if grad_loss is not None else None
    check(lib().pu_bce_bwd(y.data_ptr(), t.data_ptr(), y.numel(), _p(g), dy.data_ptr(), _stream()), "pu_bce_bwd")
    return dy


def seg_metrics(y, t, thresholds=()):
    """Validation metrics of a batch in one pass (pu_seg_metrics): y and t of one size with a leading
    batch axis B -> (loss [B] float32, counts [B, 2 + 2 T] int64) on the device.  loss[b] has the
    bits of bce_fwd(y[b], t[b]); a counts row is agree, tcount, pcount[0..T), icount[0..T) - see
    plastic_unet.h.  thresholds: up to 32 ascending host floats, compared as NumPy compares an fp32
    array with a float64 scalar."""
    _req(y, "y"); _req(t, "t")
    if y.dim() < 1 or y.shape[0] == 0:
        raise ValueError("seg_metrics: y needs a leading batch axis (got shape %s)" % (tuple(y.shape),))
    if t.numel() != y.numel():
        raise ValueError("Target size (%s) must be the same as input size (%s)" % (tuple(t.shape), tuple(y.shape)))
    B = y.shape[0]
    n = y.numel() // B
    T = len(thresholds)
    th = (ctypes.c_double * max(T, 1))(*[float(v) for v in thresholds])
    L = lib()
    nbytes = L.pu_seg_metrics_workspace_bytes(B, n, T)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=y.device)
    loss = torch.empty(B, dtype=torch.float32, device=y.device)
    counts = torch.empty((B, 2 + 2 * T), dtype=torch.int64, device=y.device)
    with _Rec("seg_metrics", nbytes=8.0 * y.numel() + float(nbytes)):
        check(L.pu_seg_metrics(y.data_ptr(), t.data_ptr(), B, n, th if T else None, T, loss.data_ptr(), counts.data_ptr(),
                               ws.data_ptr(), nbytes, _stream()), "pu_seg_metrics")
    return loss, counts


def rle_encode(y, threshold, cap=None):
    """Threshold and column-major run-length encoding of a batch of maps (pu_rle_encode): y [B, H, W]
    -> (offsets [B + 1] int32, runs [cap, 2] int32) on the device.  The (start, length) pairs of image
    b are runs[offsets[b]:offsets[b + 1]], the numbers utils.encode prints for y[b] > threshold.
    threshold: a host float compared as (double)y > threshold - a compare value, see punet.rle.compare_value.
    cap: room for that many pairs (default: the worst case, B * ceil(H W / 2)); the offsets are the true
    ones whatever it is, and pairs from index cap on are not stored."""
    _req(y, "y")
    if y.dim() != 3 or y.numel() == 0:
        raise ValueError("rle_encode: y must be [B, H, W] with no empty axis (got shape %s)" % (tuple(y.shape),))
    B, H, W = y.shape
    if cap is None:
        cap = B * ((H * W + 1) // 2)
    L = lib()
    nbytes = L.pu_rle_encode_workspace_bytes(B, H, W)
    ws = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=y.device)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=y.device)
    runs = torch.empty((max(cap, 0), 2), dtype=torch.int32, device=y.device)
    with _Rec("rle_encode", nbytes=4.0 * y.numel() + 2.0 * float(nbytes)):
        check(L.pu_rle_encode(y.data_ptr(), B, H, W, float(threshold), offsets.data_ptr(), runs.data_ptr() or None, cap,
                              ws.data_ptr(), nbytes, _stream()), "pu_rle_encode")
    return offsets, runs


def check_augment_table(table, batch, max_shift):
    """A host table of augment rows -> int32 numpy [batch, 4], or ValueError: rows {flip, dy, dx, 0} with
    flip in {0, 1} and |dy|, |dx| <= max_shift (the kernel would clamp them; a host table says what it
    means)."""
    rows = table.numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if rows.shape != (batch, 4):
        raise ValueError("augment: the table must be [%d, 4] {flip, dy, dx, 0} rows (got shape %s)" % (batch, rows.shape))
    if rows.dtype.kind not in "iu":
        raise ValueError("augment: the table must hold integers (got %s)" % rows.dtype)
    if rows.size and not np.isin(rows[:, 0], (0, 1)).all():
        raise ValueError("augment: a flip outside {0, 1}")
    if rows.size and (np.abs(rows[:, 1:3].astype(np.int64)) > max_shift).any():
        raise ValueError("augment: a shift outside +-%d (max_shift)" % max_shift)
    return np.ascontiguousarray(rows, dtype=np.int32)


def augment(x, t, table, max_shift, out=None):
    """Flip and reflected shift of a batch (pu_augment): x [B, Cx, H, W] and t [B, Ct, H, W] or None ->
    (x_out, t_out) (t_out None with t); slot b's planes, image and mask alike, transformed by table row
    b = {flip, dy, dx, 0} - see plastic_unet.h.  table: a device int32 tensor [B, 4], used as it is (the
    kernel clamps its shifts to +-max_shift), or a host array / CPU tensor, checked here (ValueError) and
    uploaded.  out: None (new tensors) or the pair (x_out, t_out) to write, neither overlapping an input."""
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("augment: x must be [B, C, H, W] with no empty axis (got shape %s)" % (tuple(x.shape),))
    B, cx, H, W = x.shape
    ct = 0
    if t is not None:
        if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (H, W) or t.numel() == 0:
            raise ValueError("augment: t must be [%d, C, %d, %d] like x (got shape %s)" % (B, H, W, tuple(t.shape)))
        ct = t.shape[1]
    max_shift = int(max_shift)
    if not 0 <= max_shift <= min(H, W) - 1:
        raise ValueError("augment: max_shift %d outside 0 .. min(H, W) - 1 = %d" % (max_shift, min(H, W) - 1))
    on_device = isinstance(table, torch.Tensor) and table.is_cuda
    if on_device:
        _req(table, "table", torch.int32)
        if tuple(table.shape) != (B, 4):
            raise ValueError("augment: the table must be [%d, 4] (got shape %s)" % (B, tuple(table.shape)))
    else:
        rows = check_augment_table(table, B, max_shift)      # before the images are looked at: a host-only check
    _req(x, "x"); _req(t, "t")
    if not on_device:
        table = torch.from_numpy(rows).to(x.device)
    if out is None:
        x_out = torch.empty_like(x)
        t_out = torch.empty_like(t) if t is not None else None
    else:
        x_out, t_out = out
        _req(x_out, "x_out"); _req(t_out, "t_out")
        if x_out.shape != x.shape or (t is None) != (t_out is None) or (t is not None and t_out.shape != t.shape):
            raise ValueError("augment: out must be (x_out, t_out) shaped like (x, t)")
    with _Rec("augment", nbytes=8.0 * (x.numel() + (t.numel() if t is not None else 0))):
        check(lib().pu_augment(x.data_ptr(), _p(t), x_out.data_ptr(), _p(t_out), B, cx, ct, H, W, table.data_ptr(),
                               max_shift, _stream()), "pu_augment")
    return x_out, t_out


def flip_mean(y, y_mirror, out=None):
    """out = 0.5 * (y + y_mirror mirrored left-right) (pu_flip_mean): y and y_mirror [..., H, W] of one
    shape, the prediction of a batch and of its mirrored images.  out: None (a new tensor) or y itself."""
    _req(y, "y"); _req(y_mirror, "y_mirror"); _req(out, "out")
    if y.dim() < 2 or y.numel() == 0:
        raise ValueError("flip_mean: y must be [..., H, W] with no empty axis (got shape %s)" % (tuple(y.shape),))
    if y_mirror.shape != y.shape or (out is not None and out.shape != y.shape):
        raise ValueError("flip_mean: y %s, y_mirror %s and out must have one shape" % (tuple(y.shape), tuple(y_mirror.shape)))
    if out is None:
        out = torch.empty_like(y)
    H, W = y.shape[-2:]
    with _Rec("flip_mean", nbytes=12.0 * y.numel()):
        check(lib().pu_flip_mean(y.data_ptr(), y_mirror.data_ptr(), out.data_ptr(), y.numel() // (H * W), H, W, _stream()),
              "pu_flip_mean")
    return out


FIT_MODES = {"pad": 0, "crop": 1, "resize": 2}     # PU_FIT_PAD, PU_FIT_CROP, PU_FIT_RESIZE


def fit(x, size, mode, top=0, left=0, out=None):
    """Planes of one size gathered into planes of another (pu_fit): x [..., h, w] -> [..., H, W], size = (H, W)
    or one side S.  mode 'pad': reflected borders (the edge pixel not repeated), `top` rows above and `left`
    columns before the data - numpy.pad(mode='reflect'); 'crop': the H x W window at (top, left); both are bit
    copies.  'resize': bilinear with zeros outside, skimage's resize(order=1, mode='constant') as
    utils.data_set.resize_bilinear_constant restates it - see plastic_unet.h for the order of its arithmetic.
    out: None (a new tensor) or the tensor to write, not overlapping x."""
    if mode not in FIT_MODES:
        raise ValueError("fit: mode must be 'pad', 'crop' or 'resize', not %r" % (mode,))
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError("fit: x must be [..., h, w] with no empty axis (got shape %s)" % (tuple(x.shape),))
    H, W = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
    h, w = x.shape[-2:]
    top, left = int(top), int(left)
    if H < 1 or W < 1 or h * w > 1 << 30 or H * W > 1 << 30:
        raise ValueError("fit: planes of %d x %d to %d x %d (1 .. 2^30 pixels each)" % (h, w, H, W))
    if mode == "pad":
        if H < h or W < w:
            raise ValueError("fit: pad of %d x %d to a smaller %d x %d" % (h, w, H, W))
        if not (0 <= top <= h - 1 and 0 <= H - h - top <= h - 1):
            raise ValueError("fit: pad rows: top %d and bottom %d outside 0 .. h - 1 = %d" % (top, H - h - top, h - 1))
        if not (0 <= left <= w - 1 and 0 <= W - w - left <= w - 1):
            raise ValueError("fit: pad columns: left %d and right %d outside 0 .. w - 1 = %d" % (left, W - w - left, w - 1))
    elif mode == "crop":
        if H > h or W > w:
            raise ValueError("fit: crop of %d x %d to a larger %d x %d" % (h, w, H, W))
        if not (0 <= top <= h - H and 0 <= left <= w - W):
            raise ValueError("fit: crop window at top %d, left %d of %d x %d leaves the plane %d x %d" % (top, left, H, W, h, w))
    elif top or left:
        raise ValueError("fit: resize takes top = left = 0 (got %d, %d)" % (top, left))
    _req(x, "x"); _req(out, "out")
    shape = tuple(x.shape[:-2]) + (H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape:
        raise ValueError("fit: out must be %s (got shape %s)" % (shape, tuple(out.shape)))
    with _Rec("fit", nbytes=4.0 * (x.numel() + out.numel())):
        check(lib().pu_fit(x.data_ptr(), out.data_ptr(), x.numel() // (h * w), h, w, H, W, FIT_MODES[mode], top, left,
                           _stream()), "pu_fit")
    return out


LOVASZ_MAX_N = 16384    # pixels per image one workgroup sorts in LDS (csrc/lovasz.hip)


def lovasz_fwd(y, t):
    """Lovasz loss on probabilities, per image (pu_lovasz_fwd): y and t [B, n] -> (loss 0-d, loss_per_image
    [B], D [B, n]) on the device.  loss is the mean of the image losses; D[b][i] is d loss_b / d y[b][i],
    the table lovasz_bwd scales - see plastic_unet.h for the order of the sort and of every sum."""
    _req(y, "y"); _req(t, "t")
    if y.dim() != 2 or y.numel() == 0:
        raise ValueError("lovasz_fwd: y must be [B, n] with no empty axis (got shape %s)" % (tuple(y.shape),))
    if t.shape != y.shape:
        raise ValueError("Target size (%s) must be the same as input size (%s)" % (tuple(t.shape), tuple(y.shape)))
    B, n = y.shape
    if n > LOVASZ_MAX_N:
        raise ValueError("lovasz_fwd: %d pixels per image; one workgroup sorts an image in LDS, up to %d (128 x 128)"
                         % (n, LOVASZ_MAX_N))
    L = lib()
    nbytes = L.pu_lovasz_workspace_bytes(B, n)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    per_image = torch.empty(B, dtype=torch.float32, device=y.device)
    dtab = torch.empty_like(y)
    with _Rec("lovasz_fwd", nbytes=12.0 * y.numel()):
        check(L.pu_lovasz_fwd(y.data_ptr(), t.data_ptr(), B, n, loss.data_ptr(), per_image.data_ptr(), dtab.data_ptr(),
                              ws.data_ptr(), nbytes, _stream()), "pu_lovasz_fwd")
    return loss, per_image, dtab


def lovasz_bwd(dtab, grad_loss):
    """dy = D * (grad_loss / B) (pu_lovasz_bwd): D [B, n] from lovasz_fwd, grad_loss a device scalar
    (None: 1)."""
    _req(dtab, "dtab")
    if dtab.dim() != 2 or dtab.numel() == 0:
        raise ValueError("lovasz_bwd: dtab must be [B, n] with no empty axis (got shape %s)" % (tuple(dtab.shape),))
    g = grad_loss.contiguous() if grad_loss is not None else None
    _req(g, "grad_loss")
    dy = torch.empty_like(dtab)
    B, n = dtab.shape
    with _Rec("lovasz_bwd", nbytes=8.0 * dtab.numel()):
        check(lib().pu_lovasz_bwd(dtab.data_ptr(), _p(g), B, n, dy.data_ptr(), _stream()), "pu_lovasz_bwd")
    return dy


def grad_norm(grads, max_norm):
    """Global 2-norm of the gradient tensors and its clipping coefficient (pu_grad_norm) ->
    float32 [2] on the device: [norm, min(1, max_norm / (norm + 1e-6))].  The sum runs in fp64 in a
    fixed order: the same bits for the same values wherever the tensors lie.  float('inf') as
    max_norm measures without clipping."""
    n = len(grads)
    if n == 0:
        raise ValueError("grad_norm: no gradients")
    arr = (AdamTensor * n)()
    for i, g in enumerate(grads):
        _req(g, "grads[%d]" % i)
        arr[i] = AdamTensor(None, g.data_ptr(), None, None, g.numel())
    L = lib()
    nbytes = L.pu_grad_norm_workspace_bytes(arr, n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=grads[0].device)
    out = torch.empty(2, dtype=torch.float32, device=grads[0].device)
    with _Rec("grad_norm", nbytes=4.0 * sum(g.numel() for g in grads) + float(nbytes)):
        check(L.pu_grad_norm(arr, n, max_norm, out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "pu_grad_norm")
    return out


def adam_multi(params, grads, exp_avgs, exp_avg_sqs, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt,
               grad_scale=None):
    """grad_scale: a float32 device tensor whose first element multiplies every gradient as it is
    read (pu_adam_multi_clipped; the gradients themselves stay as they are); None: pu_adam_multi."""
    n = len(params)
    arr = (AdamTensor * max(n, 1))()
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        arr[i] = AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    with _Rec("adam", nbytes=28.0 * sum(p.numel() for p in params)):
        if grad_scale is None:
            check(lib().pu_adam_multi(arr, n, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt, _stream()),
                  "pu_adam_multi")
        else:
            _req(grad_scale, "grad_scale")
            check(lib().pu_adam_multi_clipped(arr, n, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt,
                                              grad_scale.data_ptr(), _stream()), "pu_adam_multi_clipped")


# --------------------------------------------------------------------- BatchNorm2d / bilinear 2x
def bn_fwd(z, gamma, beta, running_mean, running_var, eps, momentum, training, relu=True, resid=None):
    """BatchNorm2d (+ReLU) over NHWC z [B,H,W,C].  training: per-slot statistics over H x W (the
    reference's bs=1 BatchNorm, slot by slot) and B in-order running-statistic updates; else the
    running statistics; resid is added before the ReLU.  Returns (y, save_mean [B,C] or [C], save_rstd)."""
    _req(z, "z"); _req(resid, "resid")
    B, H, W, C = z.shape
    y = torch.empty_like(z)
    shape = (B, C) if training else (C,)
    mean = torch.empty(shape, dtype=torch.float32, device=z.device)
    rstd = torch.empty(shape, dtype=torch.float32, device=z.device)
    L = lib()
    nbytes = L.pu_bn_workspace_bytes(B, H * W, C)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=z.device)
    with _Rec("batchnorm_fwd", nbytes=4.0 * (3 if training else 2) * z.numel()):
        check(L.pu_bn_fwd(z.data_ptr(), _p(gamma), _p(beta), _p(running_mean), _p(running_var), y.data_ptr(),
                          mean.data_ptr(), rstd.data_ptr(), B, H * W, C, float(eps), float(momentum),
                          1 if training else 0, 1 if relu else 0, _p(resid), ws.data_ptr(), nbytes, _stream()),
              "pu_bn_fwd")
    return y, mean, rstd


def bn_bwd(z, g, mean, rstd, gamma, dgamma=None, dbeta=None, add=None, mask=None):
    """Backward of the training-mode BatchNorm2d given g = dL/d(BN output) (ReLU mask already
    applied): returns dz (+ add, times (mask > 0) when given); writes dgamma / dbeta [C]."""
    _req(z, "z"); _req(g, "g"); _req(add, "add"); _req(mask, "mask")
    B, H, W, C = z.shape
    dz = torch.empty_like(z)
    L = lib()
    nbytes = L.pu_bn_workspace_bytes(B, H * W, C)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=z.device)
    with _Rec("batchnorm_bwd", nbytes=4.0 * 5 * z.numel()):
        check(L.pu_bn_bwd(z.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(gamma), dz.data_ptr(),
                          _p(dgamma), _p(dbeta), B, H * W, C, _p(add), _p(mask), ws.data_ptr(), nbytes, _stream()),
              "pu_bn_bwd")
    return dz


def upsample_bilinear2x(x):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) on NHWC x."""
    _req(x, "x")
    B, h, w, C = x.shape
    y = torch.empty(B, 2 * h, 2 * w, C, dtype=torch.float32, device=x.device)
    with _Rec("upsample_fwd", nbytes=4.0 * (x.numel() + y.numel())):
        check(lib().pu_upsample_bilinear2x_fwd(x.data_ptr(), y.data_ptr(), B, h, w, C, _stream()),
              "pu_upsample_bilinear2x_fwd")
    return y


def upsample_bilinear2x_bwd(dy, mask=None):
    """Gradient of upsample_bilinear2x w.r.t. its input, times (mask > 0) when given."""
    _req(dy, "dy"); _req(mask, "mask")
    B, H2, W2, C = dy.shape
    dx = torch.empty(B, H2 // 2, W2 // 2, C, dtype=torch.float32, device=dy.device)
    with _Rec("upsample_bwd", nbytes=4.0 * (dy.numel() + 2 * dx.numel())):
        check(lib().pu_upsample_bilinear2x_bwd(dy.data_ptr(), _p(mask), dx.data_ptr(), B, H2 // 2, W2 // 2, C,
                                               _stream()), "pu_upsample_bilinear2x_bwd")
    return dx
