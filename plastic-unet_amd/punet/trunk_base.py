"""What UNetpTrunk (punet.trunk) and ResTrunk (punet.res_trunk) share: the state every trunk
carries, the gradient-sink and bucket-ready plumbing, the weight-gradient side-stream wrapper, the
BatchNorm and outconv blocks, and the one autograd node.  A trunk adds its parameter order
(``params``, ``slot``, ``backward_order()``) and its ``forward`` / ``backward`` schedules.
"""
import torch

from . import kernels as K
from .layers import as_nhwc_input
from .packs import Packs


class _OnStream:
    """torch.cuda.stream(s) without its per-call device resolution (host time on the backward's
    issue path): make s current, restore the previous stream of s's device on exit."""
    __slots__ = ("s", "prev")

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        self.prev = torch.cuda.current_stream(self.s.device_index)
        torch.cuda.set_stream(self.s)

    def __exit__(self, *exc):
        torch.cuda.set_stream(self.prev)
        return False


def _no_sink(i):
    return None


class TrunkBase:
    coord = None             # the CoordConv stem module of a coord trunk (its input gets AddCoords)
    with_r = False

    def __init__(self):
        self.packs = Packs()
        self.params = []
        self.slot = {}           # layer key ("inc.c0", "uconv2.up", "outc", ...) -> index of its weight
        self.training = True     # the model's mode, set by the model's forward
        self.gradbuf = None      # punet.dp.GradBuffer: backward writes grads into its views
        self.debug = None        # dict: when set, backward stores each layer's dZ (tests/diagnostics)
        # True: forward returns the last activation (the outconv runs inside the fused head,
        # punet.head.FusedHeadFunction) and backward receives dL/d(its pre-ReLU) from the head
        self.fused_head = False
        self._ws = None          # weight-gradient side stream (PU_WSTREAM), created on first use
        self._side = None        # the side stream while a backward runs with it, else None

    def _ready(self, i, n=2):
        """params[i:i+n]'s gradient kernels are enqueued: let an armed BucketReducer know.  With
        the side stream the bucket is issued from it (RCCL then orders after the stream's weight
        gradients), after the stream has caught up with the compute stream (BatchNorm grads)."""
        gb = self.gradbuf
        if gb is None or gb.reducer is None:
            return
        ws = self._side
        if ws is None:
            gb.ready(*self.params[i:i + n])
            return
        ws.wait_stream(torch.cuda.current_stream(ws.device_index))
        with _OnStream(ws):
            gb.ready(*self.params[i:i + n])

    def _wgrad(self, fn, i, out, *reads):
        """Run weight-gradient launcher fn(out) for params[i:i+2] - on the side stream when one is
        active: the stream waits for the compute stream (dZ is its last kernel), the outputs are
        allocated on the compute stream (autograd and the optimizer use them there) and every
        tensor the side stream reads is recorded against it, so the caching allocator does not
        hand its memory out again before the side stream is done with it."""
        ws = self._side
        if ws is None:
            r = fn(out)
        else:
            if out is None:
                out = (torch.empty_like(self.params[i], memory_format=torch.contiguous_format),
                       torch.empty_like(self.params[i + 1]))
            ws.wait_stream(torch.cuda.current_stream(ws.device_index))
            with _OnStream(ws):
                r = fn(out)
            for t in reads:
                if t is not None:
                    t.record_stream(ws)
        self._ready(i)
        return r

    def grad_sinks(self):
        """Views of the flat gradient buffer to write into, or None.  Only used when every
        parameter's .grad is None (autograd then adopts the views; if a .grad already existed it
        would accumulate into an aliased buffer).  With the fused head the outconv parameters
        are the head's (its backward runs first and autograd has already adopted their views),
        so they are not checked."""
        gb = self.gradbuf
        if gb is None:
            return None
        outc = self.slot["outc"]
        skip = (outc, outc + 1) if self.fused_head else ()
        if any(p.grad is not None for i, p in enumerate(self.params) if i not in skip):
            return None
        return [gb.view_for(p) for p in self.params]

    def _sinks(self):
        """out(i) -> the (dW, db) views a backward writes params[i], params[i+1]'s gradients into,
        or None (fresh tensors)."""
        sink = self.grad_sinks()
        if sink is None:
            return _no_sink
        return lambda i: (sink[i], sink[i + 1])

    # ------------------------------------------------------------------------- BatchNorm
    def _bn_fwd(self, P, j, m, z, relu=True, resid=None):
        """BatchNorm2d module m (affine P[j], P[j+1]) over z, per slot -> (y, (mean, rstd))."""
        training = self.training or not m.track_running_stats
        update = self.training and m.track_running_stats
        y, mean, rstd = K.bn_fwd(z, P[j], P[j + 1], m.running_mean if (update or not training) else None,
                                 m.running_var if (update or not training) else None, m.eps, m.momentum, training,
                                 relu=relu, resid=resid)
        if update:
            m.num_batches_tracked.add_(z.shape[0])     # one reference forward per slot
        return y, (mean, rstd)

    def _bn_bwd(self, P, j, z, g, stat, out, grads, add=None, mask=None):
        """g = dL/d(BN output) -> dL/dz (+ add, times (mask > 0)); the affine gradients."""
        o = out(j)
        dgam = torch.empty_like(P[j]) if o is None else o[0]
        dbet = torch.empty_like(P[j + 1]) if o is None else o[1]
        dz = K.bn_bwd(z, g, stat[0], stat[1], P[j], dgam, dbet, add=add, mask=mask)
        grads[j], grads[j + 1] = dgam, dbet
        self._ready(j)
        return dz

    # --------------------------------------------------------------------------- outconv
    def _outc_fwd(self, y, P):
        """The trunk's result: the logits, or with fused_head the last activation itself."""
        if self.fused_head:
            return y
        o = self.slot["outc"]
        return K.outconv_fwd(y, P[o].reshape(-1), P[o + 1])

    def _outc_bwd(self, y_last, dlogits, P, grads, out):
        """-> dL/d(pre-ReLU of y_last); the outconv's gradients unless the fused head owns them."""
        if self.fused_head:
            return dlogits               # the fused head's outconv backward already applied the mask
        i = self.slot["outc"]
        o = out(i)
        g, dw, db = K.outconv_bwd(y_last, P[i].reshape(-1), dlogits, relu_mask=True,
                                  out=None if o is None else (o[0].view(-1), o[1]))
        grads[i] = dw.view_as(P[i])
        grads[i + 1] = db
        self._ready(i)
        return g

    def prepare_input(self, x):
        """Model input NCHW -> the trunk's NHWC input (with the AddCoords channels for a coord stem)."""
        if self.coord is not None:
            return K.add_coords(x.contiguous(), self.with_r)
        return as_nhwc_input(x)


class TrunkFunction(torch.autograd.Function):
    """autograd node: (trunk, save, x NCHW, *trunk params) -> logits [B,H,W] (or, with
    trunk.fused_head, the last activation [B,H,W,C] for the fused head)."""

    @staticmethod
    def forward(ctx, trunk, save, x, *params):
        # ``save`` is decided by the caller: grad mode is always off inside Function.forward
        detached = [p.detach() for p in params]
        logits, saved = trunk.forward(trunk.prepare_input(x.detach()), detached, save)
        ctx.trunk = trunk
        ctx.saved_acts = saved
        ctx.params = detached
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.saved_acts is None:
            raise RuntimeError("trunk activations were not saved (forward ran without grad)")
        grads = ctx.trunk.backward(ctx.saved_acts, dlogits.contiguous(), ctx.params)
        ctx.saved_acts = None
        return (None, None, None) + tuple(grads)
