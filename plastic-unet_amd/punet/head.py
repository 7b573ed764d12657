"""autograd nodes for the plastic head and BCELoss, each a pair of HIP kernel launches.

Reference: yaricom/Plastic-UNet src/unet/unet_p.py:69-88 (head) and src/train.py:70,101-105
(nn.BCELoss); backward = what loss.backward() (train.py:110) computes for them.  The Lovasz loss
(LovaszLossFunction, lovasz_loss, LovaszLoss) has no call site in the reference: an extension.
"""
import torch
import torch.nn as nn

from . import kernels as K
from ._lib import PU_RULE_HEBB, PU_RULE_OJA

RULES = {"hebb": PU_RULE_HEBB, "oja": PU_RULE_OJA}

# the 1x1 outconv runs inside the head kernel (pu_plastic_head_fwd) whenever the shapes allow;
# False restores the two-launch path (outconv in the trunk, then pu_plastic_fwd) - tests compare both
FUSE_OUTCONV = True


def fused_head_ok(feat_channels, nbf, seq=False):
    return FUSE_OUTCONV and not seq and feat_channels % 4 == 0 and nbf % 16 == 0 and 16 <= nbf <= 512


_NO_TRACE_GRAD = ("backpropagation through the updated plastic trace is not supported: the "
                  "reference detaches it before reuse (src/train.py:99)")


def _trace_backward(ctx, X, H, w, alpha, eta, y, dy, dhn, need_dx, need_w, need_a, need_h, need_eta):
    """The trace_grad backward of both head nodes (pu_plastic_bwd_trace): a gradient arrived for
    H' (dhn) and / or the incoming H wants one.  Returns (dx, dw, dalpha, dH, deta), each None
    where not wanted.  The gradient-buffer sinks are never used here: in an unrolled episode
    several nodes of one parameter run before autograd sets .grad, so each returns a fresh tensor
    and autograd accumulates them."""
    dy = None if dy is None else dy.contiguous()
    dhn = None if dhn is None else dhn.contiguous()
    dx, dw, da, dh, deta = K.plastic_bwd_trace(X, H, w, alpha, eta, y, dy, dhn, ctx.rule, need_dx=need_dx,
                                               need_dw=need_w or need_a, need_dh=need_h)
    return (dx, dw if need_w else None, da if need_a else None, dh,
            deta if need_eta and dhn is not None else None)


class FusedHeadFunction(torch.autograd.Function):
    """(feat [B,N,N,C], outc weight [1,C,1,1], outc bias [1], H [B,N,N], w, alpha, eta) -> (Y, H').

    The reference's outconv (unet_p.py:67, 253-260) and plastic head (:69-88) in one launch; X
    (the logits) is produced inside and kept for the backward, which runs the head backward and
    then the outconv backward (ReLU mask of feat fused), handing the trunk dL/d(pre-ReLU)."""

    @staticmethod
    def forward(ctx, feat, wo, bo, H, w, alpha, eta, rule, update_trace, sink=None, trace_grad=False):
        # sink: optional (GradBuffer, w, alpha, outc weight, outc bias) - grads into its views
        # trace_grad: H' keeps its gradient path (H and eta become differentiable inputs)
        ctx.sink = sink
        ctx.trace_grad = bool(trace_grad)
        ctx.rule = rule
        feat = feat.contiguous()
        H = H.detach().contiguous()
        wod = wo.detach().reshape(-1)
        X, y, hn = K.plastic_head_fwd(feat, wod, bo.detach(), H, w.detach(), alpha.detach(), eta.detach(), rule,
                                      update_trace)
        ctx.save_for_backward(feat, wod, X, H, w.detach(), alpha.detach(), y, eta.detach())
        ctx.wo_shape = wo.shape
        ctx.set_materialize_grads(False)
        if hn is not None and not ctx.trace_grad:
            ctx.mark_non_differentiable(hn)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        if ctx.trace_grad and (dhn is not None or (dy is not None and ctx.needs_input_grad[3])):
            feat, wod, X, H, w, alpha, y, eta = ctx.saved_tensors
            dx, dw, da, dh, deta = _trace_backward(ctx, X, H, w, alpha, eta, y, dy, dhn, True,
                                                   ctx.needs_input_grad[4], ctx.needs_input_grad[5],
                                                   ctx.needs_input_grad[3], ctx.needs_input_grad[6])
            dfeat, dwo, dbo = K.outconv_bwd(feat, wod, dx, relu_mask=True)
            return (dfeat, dwo.view(ctx.wo_shape), dbo, dh, dw, da, deta, None, None, None, None)
        if dhn is not None:
            raise RuntimeError(_NO_TRACE_GRAD)
        if dy is None:
            return (None,) * 11
        feat, wod, X, H, w, alpha, y, _ = ctx.saved_tensors
        need_dw = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        out_h = out_o = None
        if ctx.sink is not None:
            gb, wp, ap, wop, bop = ctx.sink
            if wp.grad is None and ap.grad is None:
                out_h = (gb.view_for(wp), gb.view_for(ap))
            if wop.grad is None and bop.grad is None:
                out_o = (gb.view_for(wop).view(-1), gb.view_for(bop))
        dx, dw, da = K.plastic_bwd(X, H, w, alpha, y, dy.contiguous(), need_dx=True, need_dw=need_dw, out=out_h)
        if out_h is not None:
            ctx.sink[0].ready(ctx.sink[1], ctx.sink[2])
        dfeat, dwo, dbo = K.outconv_bwd(feat, wod, dx, relu_mask=True, out=out_o)
        if out_o is not None:
            ctx.sink[0].ready(ctx.sink[3], ctx.sink[4])
        return (dfeat, dwo.view(ctx.wo_shape), dbo, None, dw if ctx.needs_input_grad[4] else None,
                da if ctx.needs_input_grad[5] else None, None, None, None, None, None)


class PlasticHeadFunction(torch.autograd.Function):
    """(X [B,N,N], H [B,N,N], w, alpha, eta) -> (Y, H').

    By default H' is returned without a gradient path (the reference's callers always detach it
    before the next sample, train.py:99, and no loss depends on it), so eta receives no gradient
    (S3).  trace_grad=True keeps the path the reference's forward leaves open: H' is
    differentiable, H and eta receive gradients (pu_plastic_bwd_trace) whenever a gradient reaches
    H' or the incoming H wants one; otherwise the backward is the default one, bit for bit.
    """

    @staticmethod
    def forward(ctx, X, H, w, alpha, eta, rule, update_trace, sink=None, trace_grad=False):
        # sink: optional (GradBuffer, w_param, alpha_param) - write dw/dalpha into its views
        # trace_grad: H' keeps its gradient path (H and eta become differentiable inputs)
        ctx.sink = sink
        ctx.trace_grad = bool(trace_grad)
        ctx.rule = rule
        X = X.contiguous()
        H = H.detach().contiguous()
        y, hn = K.plastic_fwd(X, H, w.detach(), alpha.detach(), eta.detach(), rule, update_trace)
        ctx.save_for_backward(X, H, w.detach(), alpha.detach(), y, eta.detach())
        ctx.set_materialize_grads(False)
        if hn is not None and not ctx.trace_grad:
            ctx.mark_non_differentiable(hn)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        if ctx.trace_grad and (dhn is not None or (dy is not None and ctx.needs_input_grad[1])):
            X, H, w, alpha, y, eta = ctx.saved_tensors
            dx, dw, da, dh, deta = _trace_backward(ctx, X, H, w, alpha, eta, y, dy, dhn, ctx.needs_input_grad[0],
                                                   ctx.needs_input_grad[2], ctx.needs_input_grad[3],
                                                   ctx.needs_input_grad[1], ctx.needs_input_grad[4])
            return (dx, dh, dw, da, deta, None, None, None, None)
        if dhn is not None:
            raise RuntimeError(_NO_TRACE_GRAD)
        if dy is None:
            return (None,) * 9
        X, H, w, alpha, y, _ = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dw = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        out = None
        if ctx.sink is not None:
            gb, wp, ap = ctx.sink
            if wp.grad is None and ap.grad is None:
                out = (gb.view_for(wp), gb.view_for(ap))
        dx, dw, da = K.plastic_bwd(X, H, w, alpha, y, dy.contiguous(), need_dx=need_dx, need_dw=need_dw, out=out)
        if out is not None:
            ctx.sink[0].ready(ctx.sink[1], ctx.sink[2])
        return (dx, None, dw if ctx.needs_input_grad[2] else None, da if ctx.needs_input_grad[3] else None,
                None, None, None, None, None)


class SequentialHeadFunction(torch.autograd.Function):
    """hebb_mode='sequential': (X [B,N,N], H [N,N], w, alpha, eta) -> (Y [B,N,N], H' [N,N]).

    One trace threaded through the samples in order - B successive reference calls
    (src/train.py:91-99) sharing the parameters: sample b runs the fused head kernel on the trace
    sample b-1 left.  The traces are detached between samples (train.py:99), so the backward is
    the batched head backward with the per-sample traces H_b as constants (one launch)."""

    @staticmethod
    def forward(ctx, X, H, w, alpha, eta, rule, sink=None):
        ctx.sink = sink
        X = X.contiguous()
        B, N, _ = X.shape
        Hs = torch.empty(B, N, N, dtype=torch.float32, device=X.device)
        Y = torch.empty_like(X)
        h = H.detach().reshape(1, N, N).contiguous()
        wd, ad, ed = w.detach(), alpha.detach(), eta.detach()
        for b in range(B):
            Hs[b].copy_(h[0])
            y, h = K.plastic_fwd(X[b:b + 1], h, wd, ad, ed, rule, True)
            Y[b].copy_(y[0])
        ctx.save_for_backward(X, Hs, wd, ad, Y)
        ctx.set_materialize_grads(False)
        hn = h.reshape(N, N)
        ctx.mark_non_differentiable(hn)
        return Y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        if dhn is not None:
            raise RuntimeError(_NO_TRACE_GRAD + "; trace gradients (trace_grad=True) need hebb_mode='slots'")
        if dy is None:
            return (None,) * 7
        X, Hs, w, alpha, y = ctx.saved_tensors
        out = None
        if ctx.sink is not None:
            gb, wp, ap = ctx.sink
            if wp.grad is None and ap.grad is None:
                out = (gb.view_for(wp), gb.view_for(ap))
        need_dw = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dx, dw, da = K.plastic_bwd(X, Hs, w, alpha, y, dy.contiguous(), need_dx=ctx.needs_input_grad[0],
                                   need_dw=need_dw, out=out)
        if out is not None:
            ctx.sink[0].ready(ctx.sink[1], ctx.sink[2])
        return (dx, None, dw if ctx.needs_input_grad[2] else None, da if ctx.needs_input_grad[3] else None,
                None, None, None)


class BCELossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, t):
        y = y.contiguous()
        t = t.detach().contiguous()
        ctx.save_for_backward(y, t)
        return K.bce_fwd(y, t)

    @staticmethod
    def backward(ctx, g):
        y, t = ctx.saved_tensors
        return K.bce_bwd(y, t, g), None


def bce_loss(y, t):
    """nn.BCELoss()(y.view(-1), t.view(-1)) on the HIP path (mean, log clamped at -100)."""
    return BCELossFunction.apply(y.reshape(-1), t.reshape(-1))


class BCELoss(nn.Module):
    """Drop-in for ``nn.BCELoss()`` (reduction='mean') on ROCm tensors."""

    def forward(self, input, target):
        return bce_loss(input, target)


class LovaszLossFunction(torch.autograd.Function):
    """(y [B, n], t [B, n]) -> the mean over the images of the Lovasz loss of each (pu_lovasz_fwd).  The
    forward sorts every image once and keeps D = d loss_b / d y; the backward is D * (g / B)."""

    @staticmethod
    def forward(ctx, y, t):
        y = y.contiguous()
        t = t.detach().contiguous()
        loss, _, dtab = K.lovasz_fwd(y, t)
        ctx.save_for_backward(dtab)
        return loss

    @staticmethod
    def backward(ctx, g):
        dtab, = ctx.saved_tensors
        return K.lovasz_bwd(dtab, g), None


def lovasz_loss(y, t):
    """Lovasz extension of the Jaccard loss on probabilities (Berman's lovasz_softmax for the one
    foreground class), per image, mean over the batch: y and t [B, n] or [B, H, W], n <= 16384.  A pixel
    is foreground when 0.5 <= t <= 1, as validation reads it."""
    if y.dim() < 2:
        raise ValueError("lovasz_loss: y needs a leading batch axis, [B, n] or [B, H, W] (got shape %s)" % (tuple(y.shape),))
    if t.numel() != y.numel():
        raise ValueError("Target size (%s) must be the same as input size (%s)" % (tuple(t.shape), tuple(y.shape)))
    B = y.shape[0]
    return LovaszLossFunction.apply(y.reshape(B, -1), t.reshape(B, -1))


class LovaszLoss(nn.Module):
    """``lovasz_loss`` as a module, next to BCELoss."""

    def forward(self, input, target):
        return lovasz_loss(input, target)
