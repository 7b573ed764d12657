"""The U-Net trunk of UNetp as one autograd node whose forward and backward are sequences of
HIP kernel launches (no ATen compute ops).

Reference: yaricom/Plastic-UNet src/unet/unet_p.py:54-67 (forward) and the blocks at :179-260;
the backward is what ``loss.backward()`` (src/train.py:110) runs through ATen on the CPU.

The layer ops live in punet.layers and the plumbing shared with the residual trunk (gradient
sinks, side-stream weight gradients, BatchNorm and outconv blocks, the autograd node) in
punet.trunk_base; this module is UNetp's parameter order and its two schedules.

Forward (NHWC, fp32), per stage:
  inc     : conv3x3+ReLU, conv3x3+ReLU
  down_i  : MaxPool2d(2) -> conv3x3+ReLU -> conv3x3+ReLU
  up_j    : ConvT2x2s2 (GEMM + pixel-shuffle epilogue) -> conv3x3+ReLU over [skip | upsampled]
            read from two buffers (no concat copy) -> conv3x3+ReLU
  outc    : 1x1 conv C -> 1 (logits)
The CoordConv U-Net of src/coord_conv_script.py:146-200 (config C4) is the same schedule with a
stem - AddCoords fused into the input transpose (pu_add_coords) + 1x1 conv + ReLU - and Keras-style
up stages: ConvT2x2s2 halving the channels and the concat [upsampled | skip] (upsampled FIRST).
Backward fuses every ReLU mask into the producing kernel's epilogue (dgrad / maxpool-bwd /
outconv-bwd multiply by (activation > 0)), writes skip gradients once and lets the max-pool
backward accumulate into them, and gets bias gradients from the weight-gradient GEMM (a ones
column / ones row), so no separate elementwise or reduction passes run.
"""
import os

import torch

from . import kernels as K
from .layers import (conv3x3, conv3x3_dgrad, conv3x3_wgrad, conv1x1, conv1x1_wgrad,            # noqa: F401
                     convT2x2, convT2x2_dgrad, convT2x2_wgrad, as_nhwc_input, _kp, _cg)
from .packs import Packs as _Packs                                                              # noqa: F401
from .trunk_base import TrunkBase, TrunkFunction, _OnStream                                     # noqa: F401


# Weight-gradient side stream: the backward enqueues every weight gradient (and its split
# reduction) on a second stream, ordered after the kernel that produced its dZ, so they overlap the
# data-gradient chain.  PU_WSTREAM=1 always, 0 never, unset: bf16 trunks only - measured
# (profiles/r05_experiments/side_stream_ab.txt): C3 (bf16) 8822 -> 8952 img/s, C2 (fp32) 4370 ->
# 4317: the fp32 Winograd kernels hold a whole CU per block (LDS + 2 x 256 VGPRs per SIMD), so
# concurrent launches only queue behind each other and slow both.
_SIDE = {"1": True, "0": False}.get(os.environ.get("PU_WSTREAM", ""), "bf16")


# PU_STEM_BF16=0: the bf16 trunk's stem writes fp32 and converts (A/B runs)
_STEM_BF16 = os.environ.get("PU_STEM_BF16", "1") != "0"


def set_side_stream(on):
    """Switch the weight-gradient side stream for backward passes started after this call:
    True / False, or "bf16" (the default: bf16 trunks only)."""
    global _SIDE
    _SIDE = on if on == "bf16" else bool(on)


class UNetpTrunk(TrunkBase):
    """Parameter order and kernel schedule of the generalised UNetp trunk (depth D).  Models with a
    ``coord`` stem (CoordConvUNetp) get its w,b appended after outc and ``up_first`` concats.

    Variants of the reference's constructor flags (unet_p.py:9-52):
      batch_norm=True         (:186-193) each conv is Conv -> BatchNorm2d -> ReLU: the conv epilogue
                              keeps bias only, punet.kernels.bn_fwd normalises slot by slot (the
                              reference's batch size 1) and applies the ReLU; backward runs bn_bwd
                              on the masked gradient before the conv's wgrad / dgrad
      bilinear_upsample=True  (:235-236) nn.Upsample(2, bilinear, align_corners=True) in place of
                              the ConvTranspose2d: no parameters, gather-form backward
    """

    def __init__(self, model):
        super().__init__()
        self.depth = model.depth
        self.coord = getattr(model, "coord", None)
        self.with_r = bool(getattr(model, "with_r", False))
        self.up_first = bool(getattr(model, "up_first", False))
        # activations dtype: float32, or bfloat16 (config C3; fp32 accumulation, fp32 parameters
        # and gradients; the 1-channel stem conv runs in fp32 and its output is rounded once)
        self.dtype = getattr(model, "compute_dtype", torch.float32)
        self.bilinear = bool(getattr(model, "bilinear_upsample", False))
        seqs = {"inc": model.inc.conv.conv}
        for i in range(1, self.depth):
            seqs["down%d" % i] = getattr(model, "down%d" % i).mpconv[1].conv
        for j in range(1, self.depth):
            seqs["up%d" % j] = getattr(model, "up%d" % j).conv.conv
        self.bn = {}             # conv key -> its BatchNorm2d module
        bn_mods = []

        def add(key, w, b):
            self.slot[key] = len(self.params)
            self.params += [w, b]

        # order: inc c0 w,b, c1 w,b ; down_i ... ; up_j: [up w,b], c0 w,b, c1 w,b ; outc w,b ;
        # [coord w,b] ; then the BatchNorm affine parameters (w,b) in conv order
        def add_double(name):
            convs = [m for m in seqs[name] if isinstance(m, torch.nn.Conv2d)]
            norms = [m for m in seqs[name] if isinstance(m, torch.nn.BatchNorm2d)]
            for idx, cm in enumerate(convs):
                add("%s.c%d" % (name, idx), cm.weight, cm.bias)
                if norms:
                    bn_mods.append(("%s.c%d" % (name, idx), norms[idx]))

        add_double("inc")
        for i in range(1, self.depth):
            add_double("down%d" % i)
        for j in range(1, self.depth):
            upm = getattr(model, "up%d" % j).up
            if isinstance(upm, torch.nn.ConvTranspose2d):
                add("up%d.up" % j, upm.weight, upm.bias)
            elif not self.bilinear:
                raise RuntimeError("up%d.up is neither ConvTranspose2d nor bilinear" % j)
            add_double("up%d" % j)
        add("outc", model.outc.conv.weight, model.outc.conv.bias)
        if self.coord is not None:
            add("coord", self.coord.conv.weight, self.coord.conv.bias)
        self.n_core = len(self.params)
        for key, m in bn_mods:
            if m.momentum is None:
                raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative averaging) is not built")
            self.bn[key] = m
            self.slot[key + ".bn"] = len(self.params)
            self.params += [m.weight, m.bias]
        if (self.bn or self.bilinear) and self.dtype != torch.float32:
            raise NotImplementedError("batch_norm / bilinear_upsample run in fp32 (precision='fp32')")

    def _stem_bf16(self, x):
        """bf16 trunk whose first conv is the single-channel stem (no BatchNorm): it writes its bf16
        output directly (PU_EPI_OUT_BF16) and its weight gradient reads the bf16 dZ (pu_wgrad math
        2) - no fp32 copies and conversion passes."""
        return (_STEM_BF16 and self.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[3] == 1 and "inc.c0" not in self.bn
                and self.params[self.slot["inc.c0"]].shape[0] in (8, 16, 32, 64))

    def backward_order(self):
        """Parameters in the order backward() completes their gradients (outc first, stem last;
        each BatchNorm pair completes just before its conv)."""
        order = []
        core = self.params[:self.n_core]
        if self.coord is not None:
            core = core[:-2]
        bn_of = {self.slot[k]: self.slot[k + ".bn"] for k in self.bn}
        for idx in range(len(core) - 2, -2, -2):
            if idx in bn_of:
                j = bn_of[idx]
                order += [self.params[j + 1], self.params[j]]
            order += [core[idx + 1], core[idx]]
        if self.coord is not None:
            order += self.params[self.n_core - 2:self.n_core]
        return order

    # -------------------------------------------------------------------------------- forward
    def _conv(self, key, P, s, x0, x1=None, out_dtype=None):
        """conv3x3 (+ BatchNorm) + ReLU of conv `key` over [x0 | x1]."""
        i = self.slot[key]
        bnm = self.bn.get(key)
        if bnm is None:
            return conv3x3(x0, P[i], P[i + 1], self.packs, x1=x1, out_dtype=out_dtype)
        z = conv3x3(x0, P[i], P[i + 1], self.packs, x1=x1, relu=False)
        y, s[key + ".stat"] = self._bn_fwd(P, self.slot[key + ".bn"], bnm, z)
        s[key + ".z"] = z
        return y

    def forward(self, x, params, save):
        P = params
        D = self.depth
        pk = self.packs
        pk.refresh()                   # operands of parameters the optimizer moved: one launch
        s = {"x": x}
        if self.coord is not None:     # stem: 1x1 conv + ReLU over the AddCoords input
            ci = self.slot["coord"]
            x = s["stem"] = conv1x1(x, P[ci], P[ci + 1], pk)
        t = self._conv("inc.c0", P, s, x, out_dtype=torch.bfloat16 if self._stem_bf16(x) else None)
        if self.dtype != t.dtype:
            t = K.to_bf16(t)
        s["inc.t"] = t
        y = self._conv("inc.c1", P, s, t)
        skips = [y]
        for i in range(1, D):
            p = K.maxpool2_fwd(skips[-1]); s["down%d.p" % i] = p
            t = self._conv("down%d.c0" % i, P, s, p); s["down%d.t" % i] = t
            y = self._conv("down%d.c1" % i, P, s, t)
            skips.append(y)
        s["skips"] = skips
        y = skips[-1]
        for j in range(1, D):
            skip = skips[D - 1 - j]
            if self.bilinear:
                u = K.upsample_bilinear2x(y)
            else:
                ui = self.slot["up%d.up" % j]
                u = convT2x2(y, P[ui], P[ui + 1], pk)
            s["up%d.u" % j] = u
            if self.up_first:
                t = self._conv("up%d.c0" % j, P, s, u, skip)
            else:
                t = self._conv("up%d.c0" % j, P, s, skip, u)
            s["up%d.t" % j] = t
            y = self._conv("up%d.c1" % j, P, s, t)
            s["up%d.y" % j] = y
        return self._outc_fwd(y, P), (s if save else None)

    # ------------------------------------------------------------------------------- backward
    def _bn_back(self, key, g, s, P, grads, out):
        """g = dL/d(BN output) (ReLU mask applied) -> dL/dz of conv `key`; BatchNorm grads."""
        if key not in self.bn:
            return g
        return self._bn_bwd(P, self.slot[key + ".bn"], s[key + ".z"], g, s[key + ".stat"], out, grads)

    # The backward of a double conv (y = relu([bn] c1(t)), t = relu([bn] c0([x0 | x1]))) in two halves;
    # c0's data gradient is the caller's - the split with masks, the plain and the stem case differ.
    # Two halves, so that _backward's `dt` is rebound right after each c1 data gradient: that is when
    # the previous stage's dZ goes back to the caching allocator, and with the side stream (the dZ is
    # record_stream-ed on it) freeing it one weight gradient later, or one data gradient earlier,
    # cost C3 0.8-1 % (9.65k against 9.74k img/s, three alternating runs each).
    def _c1_bwd(self, name, g, s, P, grads, out):
        """g = dL/d(c1's pre-ReLU) -> dL/dt masked by t; c1's BatchNorm and weight gradient."""
        c1 = self.slot[name + ".c1"]
        t = s[name + ".t"]
        if self.debug is not None:
            self.debug[name + ".c1"] = g
        g = self._bn_back(name + ".c1", g, s, P, grads, out)
        grads[c1], grads[c1 + 1] = self._wgrad(lambda o: conv3x3_wgrad(g, t, out=o), c1, out(c1), g, t)
        return conv3x3_dgrad(g, P[c1], self.packs, mask0=t)[0]

    def _c0_bwd(self, name, dt, s, P, grads, out, x0, x1=None):
        """dt = dL/d(c0's pre-ReLU) -> dL/dz of c0; its BatchNorm and weight gradient over [x0 | x1]."""
        c0 = self.slot[name + ".c0"]
        dt = self._bn_back(name + ".c0", dt, s, P, grads, out)
        grads[c0], grads[c0 + 1] = self._wgrad(lambda o: conv3x3_wgrad(dt, x0, x1, out=o), c0, out(c0), dt, x0, x1)
        if self.debug is not None:
            self.debug[name + ".c0"] = dt
        return dt

    def backward(self, s, dlogits, params):
        if dlogits.is_cuda and (_SIDE is True or (_SIDE == "bf16" and self.dtype == torch.bfloat16)):
            if self._ws is None or self._ws.device != dlogits.device:
                self._ws = torch.cuda.Stream(device=dlogits.device)
            self._side = self._ws
        try:
            return self._backward(s, dlogits, params)
        finally:
            if self._side is not None:
                torch.cuda.current_stream(self._side.device_index).wait_stream(self._side)   # grads complete before use
                self._side = None

    def _backward(self, s, dlogits, params):
        D = self.depth
        pk = self.packs
        P = list(params)
        grads = [None] * len(P)
        out = self._sinks()
        sl = self.slot
        skips = s["skips"]
        g = self._outc_bwd(s["up%d.y" % (D - 1)], dlogits, P, grads, out)

        gskip = [None] * (D - 1)
        for j in range(D - 1, 0, -1):
            name = "up%d" % j
            c0 = sl[name + ".c0"]
            u = s[name + ".u"]
            skip = skips[D - 1 - j]
            y_prev = skips[D - 1] if j == 1 else s["up%d.y" % (j - 1)]
            dt = self._c1_bwd(name, g, s, P, grads, out)
            # conv0 over [skip | u]  (up_first: [u | skip])
            if self.up_first:
                dt = self._c0_bwd(name, dt, s, P, grads, out, u, skip)
                du, dskip = conv3x3_dgrad(dt, P[c0], pk, split=u.shape[3], mask1=skip)
            else:
                dt = self._c0_bwd(name, dt, s, P, grads, out, skip, u)
                dskip, du = conv3x3_dgrad(dt, P[c0], pk, split=skip.shape[3], mask0=skip)
            if self.debug is not None:
                self.debug[name + ".up"] = du
            gskip[D - 1 - j] = dskip
            if self.bilinear:
                g = K.upsample_bilinear2x_bwd(du, mask=y_prev)
            else:
                ui = sl[name + ".up"]
                grads[ui], grads[ui + 1] = self._wgrad(lambda o: convT2x2_wgrad(y_prev, du, out=o), ui, out(ui),
                                                       y_prev, du)
                g = convT2x2_dgrad(du, P[ui], pk, mask=y_prev)

        for i in range(D - 1, 0, -1):
            name = "down%d" % i
            dt = self._c1_bwd(name, g, s, P, grads, out)
            dt = self._c0_bwd(name, dt, s, P, grads, out, s[name + ".p"])
            dp, _ = conv3x3_dgrad(dt, P[sl[name + ".c0"]], pk)
            g = K.maxpool2_bwd(skips[i - 1], dp, gskip[i - 1], relu_mask=True, accumulate=True)

        x0 = s["stem"] if self.coord is not None else s["x"]
        dt = self._c1_bwd("inc", g, s, P, grads, out)
        if dt.dtype != x0.dtype and not self._stem_bf16(x0):   # bf16 trunk: the fp32 stem's weight gradient
            dt = K.to_f32(dt)
        dt = self._c0_bwd("inc", dt, s, P, grads, out, x0)
        if self.coord is not None:     # stem 1x1 conv: dgrad of inc.c0 (masked by the stem ReLU) + wgrad
            dstem, _ = conv3x3_dgrad(dt, P[sl["inc.c0"]], pk, mask0=x0)
            cs = sl["coord"]
            grads[cs], grads[cs + 1] = self._wgrad(lambda o: conv1x1_wgrad(dstem, s["x"], out=o), cs, out(cs),
                                                   dstem, s["x"])
        return grads
