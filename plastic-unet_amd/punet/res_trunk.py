"""The UNetpRes trunk (yaricom/Plastic-UNet src/unet/unet_p_res.py:71-113) as HIP kernel sequences.

Each ``down`` / ``middle`` stack (:223-238, :256-272) is Conv3x3 -> residual_block x2 -> ReLU where a
residual_block (:166-189) is  out = conv_B(relu(conv_A(relu(in)))) + relu(in)  - its leading
in-place ReLU rewrites ``in`` before the add (S11).  With r1 = relu(conv0(x)) the stack is

    a1 = relu(A1(r1))          r2 = relu(B1(a1) + r1)          a2 = relu(A2(r2))
    y  = relu(B2(a2) + r2)

five implicit-GEMM convolutions whose epilogues carry bias, the residual add (before the ReLU) and
the ReLU; nothing else is materialised.  Backward, given g = dL/dy * (y > 0):

    g_a2 = B2^T g . (a2>0)     g_o1 = (A2^T g_a2 + g) . (r2>0)     g_a1 = B1^T g_o1 . (a1>0)
    g_z0 = (A1^T g_a1 + g_o1) . (r1>0)      dX = conv0^T g_z0   (split over the two sources)

i.e. the same dgrad kernel with the residual gradient added in its epilogue before the mask.

``up`` (:200-220): ConvTranspose2d(3, s=2, p=0) takes h -> 2h+1 and the negative F.pad crops row and
column 0 when the skip is 2h wide (S13); it runs as one GEMM over the (h+1)^2 grid of 2x2 output
blocks (PU_PACK_CONVT3_FWD) whose shuffle epilogue drops the cropped pixels.  Its dgrad is a
stride-2 3x3 conv (pad = crop) and its wgrad a stride-2 weight-gradient GEMM; the bias gradient
is a column sum.  The concat is [upsampled | skip] (upsampled FIRST, :218) and is read from the
two buffers directly.  Dropout2d (:209, :248) multiplies channels by a per-sample mask
(punet.kernels.channel_scale); masks come from torch's generator (``mask_fn`` may inject them).

The layer ops (conv3x3 with its resid / chan_scale epilogues, convT3x3) are punet.layers'; the
gradient sinks, the BatchNorm and outconv blocks and the autograd node are punet.trunk_base's.
"""
import torch

from . import kernels as K
from .layers import (conv3x3, conv3x3_dgrad, conv3x3_wgrad, convT3x3, convT3x3_dgrad, convT3x3_wgrad,    # noqa: F401
                     _crop, _fusable)
from .packs import Packs as _Packs                                                                      # noqa: F401
from .trunk_base import TrunkBase


# --------------------------------------------------------------------------------- the trunk
class ResTrunk(TrunkBase):
    """Parameter order and kernel schedule of UNetpRes.  Per stack (conv1..conv4, mid, and the
    middle of uconv4..uconv1): conv0 w,b, block1 A w,b, block1 B w,b, block2 A w,b, block2 B w,b;
    each up stage puts its ConvTranspose2d w,b before its stack; outc w,b last."""

    DOWN = ("conv1", "conv2", "conv3", "conv4")
    UP = ("uconv4", "uconv3", "uconv2", "uconv1")

    def __init__(self, model):
        super().__init__()
        self.model = model
        for name in self.DOWN + ("mid",):
            mod = getattr(model, name)
            seq = mod.dconv if name != "mid" else mod.mconv
            self.slot[name] = len(self.params)
            self.params += self._stack_params(seq)
        for name in self.UP:
            mod = getattr(model, name)
            self.slot[name + ".up"] = len(self.params)
            self.params += [mod.dconv.weight, mod.dconv.bias]
            self.slot[name] = len(self.params)
            self.params += self._stack_params(mod.uconv[1].mconv)
        self.slot["outc"] = len(self.params)
        self.params += [model.outc.conv.weight, model.outc.conv.bias]
        # batch_norm=True (unet_p_res.py:171-176): each residual block of the DOWN stacks and mid
        # carries one BatchNorm2d on its ReLU'd input, before conv A (its conv_modules are built
        # without batch_norm, :174-175); the up stages' middle has none (:211).  Affine params
        # appended after outc.
        self.bn = {}             # (stack, block) -> (param index, module)
        for name in self.DOWN + ("mid",):
            mod = getattr(model, name)
            seq = mod.dconv if name != "mid" else mod.mconv
            for blk in (1, 2):
                layers = list(seq[blk].conv)
                if len(layers) == 3:
                    continue
                m = layers[1]
                if not isinstance(m, torch.nn.BatchNorm2d) or m.momentum is None:
                    raise NotImplementedError("UNetpRes BatchNorm layout not recognised")
                self.bn[(name, blk)] = (len(self.params), m)
                self.params += [m.weight, m.bias]
        self.mask_fn = None      # (name, batch, channels, p) -> [B, C] scale; default: bernoulli
        self.mask_gen = None     # torch.Generator for the bernoulli masks (None: torch's default);
                                 # data-parallel Trainers set a per-rank one (punet.dp.rank_generator)

    @staticmethod
    def _stack_params(seq):
        out = [seq[0].weight, seq[0].bias]
        for blk in (seq[1], seq[2]):
            layers = list(blk.conv)
            convs = layers[1:] if len(layers) == 3 else layers[2:]      # [ReLU, (BN,) A, B]
            for cm in convs:
                conv = cm.conv if isinstance(cm.conv, torch.nn.Conv2d) else cm.conv[0]
                out += [conv.weight, conv.bias]
        return out

    def backward_order(self):
        """Parameters in the order backward() completes their gradients (outc first, conv1 last;
        the BatchNorm affine parameters last - they are small)."""
        n_core = self.slot["outc"] + 2
        return list(reversed(self.params[:n_core])) + list(reversed(self.params[n_core:]))

    def _mask(self, name, B, C, p, device):
        if self.mask_fn is not None:
            return self.mask_fn(name, B, C, p)
        return torch.empty(B, C, dtype=torch.float32, device=device).bernoulli_(
            1.0 - p, generator=self.mask_gen).div_(1.0 - p)

    # ---------------------------------------------------------------------------- forward
    def _stack_fwd_bn(self, P, i, name, x0, x1=None):
        """conv0 + ReLU, then per residual block: n = BN(r); a = relu(A(n)); r' = relu(B(a) + r)
        (unet_p_res.py:166-189 with batch_norm=True; the add and ReLU fused in B's epilogue)."""
        pk = self.packs
        r = conv3x3(x0, P[i], P[i + 1], pk, x1=x1)
        st = {"x0": x0, "x1": x1}
        for blk in (1, 2):
            ia = i + 2 + 4 * (blk - 1)
            j, m = self.bn[(name, blk)]
            n, sa = self._bn_fwd(P, j, m, r, relu=False)
            a = conv3x3(n, P[ia], P[ia + 1], pk)
            r_next = conv3x3(a, P[ia + 2], P[ia + 3], pk, resid=r)
            st[blk] = (r, n, a, sa)
            r = r_next
        st["y"] = r
        return r, st

    def _stack_fwd(self, P, i, x0, x1=None):
        pk = self.packs
        r1 = conv3x3(x0, P[i], P[i + 1], pk, x1=x1)
        a1 = conv3x3(r1, P[i + 2], P[i + 3], pk)
        r2 = conv3x3(a1, P[i + 4], P[i + 5], pk, resid=r1)
        a2 = conv3x3(r2, P[i + 6], P[i + 7], pk)
        y = conv3x3(a2, P[i + 8], P[i + 9], pk, resid=r2)
        return y, (x0, x1, r1, a1, r2, a2, y)

    def forward(self, x, params, save):
        training = self.training       # Dropout2d masks; BatchNorm: per-slot vs running statistics
        self.packs.refresh()           # operands of parameters the optimizer moved: one launch
        P = list(params)
        p_drop = self.model.dropout_ratio
        drop = training and p_drop > 0
        s = {}
        h = x
        skips = []
        for k, name in enumerate(self.DOWN):
            if (name, 1) in self.bn:
                y, st = self._stack_fwd_bn(P, self.slot[name], name, h)
            else:
                y, st = self._stack_fwd(P, self.slot[name], h)
            s[name] = st
            skips.append(y)
            p = p_drop / 2 if k == 0 else p_drop          # pool1 uses dropout_ratio/2 (:39)
            m = self._mask("pool%d" % (k + 1), y.shape[0], y.shape[3], p, y.device) if drop else None
            h = K.maxpool2_fwd(y, scale=m)                # pool_drop (:62): the Dropout2d fused
            if drop:
                s["pool%d.mask" % (k + 1)] = m
        if ("mid", 1) in self.bn:
            y, st = self._stack_fwd_bn(P, self.slot["mid"], "mid", h)
        else:
            y, st = self._stack_fwd(P, self.slot["mid"], h)
        s["mid"] = st
        for j, name in enumerate(self.UP):
            skip = skips[3 - j]
            i = self.slot[name + ".up"]
            # Dropout2d over cat(u, skip) (unet_p_res.py:69): u's channels scaled by the ConvT
            # epilogue (the mask's row stride spans both parts), the skip's by a scaled copy (the
            # unscaled skip stays for MaxPool2d's backward)
            m = self._mask(name, y.shape[0], P[i].shape[1] + skip.shape[3], p_drop, y.device) if drop else None
            u = convT3x3(y, P[i], P[i + 1], self.packs, skip.shape[1:3], chan_scale=_fusable(m))
            s[name + ".in"] = y
            src1 = skip
            if drop:
                cu = u.shape[3]
                if _fusable(m) is None:
                    K.channel_scale(u, m[:, :cu].contiguous(), out=u)
                src1 = K.channel_scale(skip, m[:, cu:].contiguous())
                s[name + ".mask"] = m
            y, st = self._stack_fwd(P, self.slot[name], u, src1)
            s[name] = st
        s["skips"] = skips
        return self._outc_fwd(y, P), (s if save else None)

    # --------------------------------------------------------------------------- backward
    def _conv_wgrad(self, i, dz, x0, x1, grads, out):
        """The weight and bias gradient of the 3x3 conv params[i], params[i+1] over [x0 | x1]."""
        grads[i], grads[i + 1] = conv3x3_wgrad(dz, x0, x1, out=out(i))
        self._ready(i)

    def _stack_bwd(self, P, i, st, g, grads, out, need_dx=True, split=None, mask1=None, chan_scale=None):
        pk = self.packs
        x0, x1, r1, a1, r2, a2, y = st
        dbg = self.debug
        self._conv_wgrad(i + 8, g, a2, None, grads, out)
        g_a2, _ = conv3x3_dgrad(g, P[i + 8], pk, mask0=a2)
        self._conv_wgrad(i + 6, g_a2, r2, None, grads, out)
        g_o1, _ = conv3x3_dgrad(g_a2, P[i + 6], pk, mask0=r2, resid=g)
        self._conv_wgrad(i + 4, g_o1, a1, None, grads, out)
        g_a1, _ = conv3x3_dgrad(g_o1, P[i + 4], pk, mask0=a1)
        self._conv_wgrad(i + 2, g_a1, r1, None, grads, out)
        g_z0, _ = conv3x3_dgrad(g_a1, P[i + 2], pk, mask0=r1, resid=g_o1)
        self._conv_wgrad(i, g_z0, x0, x1, grads, out)
        if dbg is not None:
            dbg[i] = (g, g_a2, g_o1, g_a1, g_z0)
        if not need_dx:
            return None, None
        return conv3x3_dgrad(g_z0, P[i], pk, split=split, mask1=mask1, chan_scale=chan_scale)

    def _stack_bwd_bn(self, P, i, name, st, g, grads, out, need_dx=True, split=None, mask1=None):
        """g = dL/d(stack output) * (y > 0)."""
        pk = self.packs
        for blk in (2, 1):
            r, n, a, sa = st[blk]
            ia = i + 2 + 4 * (blk - 1)
            self._conv_wgrad(ia + 2, g, a, None, grads, out)
            ga, _ = conv3x3_dgrad(g, P[ia + 2], pk, mask0=a)
            self._conv_wgrad(ia, ga, n, None, grads, out)
            dn, _ = conv3x3_dgrad(ga, P[ia], pk)
            # r feeds the BatchNorm and the residual add: dL/dr = BN^T dn + g, times relu's mask
            g = self._bn_bwd(P, self.bn[(name, blk)][0], r, dn, sa, out, grads, add=g, mask=r)
        self._conv_wgrad(i, g, st["x0"], st["x1"], grads, out)
        if not need_dx:
            return None, None
        return conv3x3_dgrad(g, P[i], pk, split=split, mask1=mask1)

    def backward(self, s, dlogits, params):
        P = list(params)
        grads = [None] * len(P)
        out = self._sinks()
        skips = s["skips"]
        g = self._outc_bwd(s["uconv1"][6], dlogits, P, grads, out)
        gskip = [None] * 4
        for j in range(3, -1, -1):                       # uconv1 .. uconv4
            name = self.UP[j]
            st = s[name]
            cu = st[0].shape[3]
            skip = skips[3 - j]
            # the Dropout2d backward of cat(u, skip) in the split data gradient's epilogue
            m = s.get(name + ".mask")
            g_u, g_sk = self._stack_bwd(P, self.slot[name], st, g, grads, out, split=cu, mask1=skip,
                                        chan_scale=_fusable(m))
            if m is not None and _fusable(m) is None:
                K.channel_scale(g_u, m[:, :cu].contiguous(), out=g_u)
                K.channel_scale(g_sk, m[:, cu:].contiguous(), out=g_sk)
            gskip[3 - j] = g_sk
            i = self.slot[name + ".up"]
            x_in = s[name + ".in"]
            grads[i], grads[i + 1] = convT3x3_wgrad(x_in, g_u, out=out(i))
            self._ready(i)
            g = convT3x3_dgrad(g_u, P[i], self.packs, x_in.shape[1:3], mask=x_in)
        if ("mid", 1) in self.bn:
            g_p, _ = self._stack_bwd_bn(P, self.slot["mid"], "mid", s["mid"], g, grads, out)
        else:
            g_p, _ = self._stack_bwd(P, self.slot["mid"], s["mid"], g, grads, out)
        for k in range(3, -1, -1):                       # conv4 .. conv1
            g = K.maxpool2_bwd(skips[k], g_p, gskip[k], relu_mask=True, accumulate=True,
                               scale=s.get("pool%d.mask" % (k + 1)))
            name = self.DOWN[k]
            if (name, 1) in self.bn:
                g_p, _ = self._stack_bwd_bn(P, self.slot[name], name, s[name], g, grads, out, need_dx=k > 0)
            else:
                g_p, _ = self._stack_bwd(P, self.slot[name], s[name], g, grads, out, need_dx=k > 0)
        return grads
