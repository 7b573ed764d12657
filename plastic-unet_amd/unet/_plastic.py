"""What UNetp, UNetpRes and CoordConvUNetp share: the trunk plan and zero trace (PlasticModel),
the input checks, and the tail of forward - trunk, then the fused, sequential or plain plastic head.

Each model keeps its own batch-size rule, its image-side rule (``_check_side``), its trunk class
(``_new_trunk``) and whether it has a sequential mode.
"""
import torch


def _check_gpu_tensor(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(
            "%s must be a tensor on the ROCm device: this UNetp runs only as HIP kernels on MI355X "
            "(no CPU fallback); got %s" % (what, getattr(t, "device", type(t))))


class PlasticModel:
    """Mixin of the three models (before nn.Module in the bases)."""
    _trunk = None

    def _trunk_plan(self):
        if self._trunk is None:
            self._trunk = self._new_trunk()
        return self._trunk

    def _check_config(self):
        """Constructor flags that cannot run together (checked after the device checks)."""

    def initialZeroHebb(self, batch=None):
        """Zero trace [nbf,nbf] (unet_p.py:90-94), or [batch,nbf,nbf] per-slot traces."""
        shape = (self.nbf, self.nbf) if batch is None else (batch, self.nbf, self.nbf)
        return torch.zeros(*shape, dtype=torch.float, device=self.torch_dev)


def check_inputs(model, x, hebb, single, seq):
    """The checks every model runs after its batch-size rule, in their order.  Returns (x as
    float32, H [B or 1, nbf, nbf])."""
    if model.alfa_type not in ("free", "yoked"):
        raise ValueError("Must select one plasticity coefficient type ('free' or 'yoked')")
    if model.rule not in ("hebb", "oja"):
        raise ValueError("Must select one learning rule ('hebb' or 'oja')")
    _check_gpu_tensor(x, "x")
    _check_gpu_tensor(hebb, "hebb")
    model._check_config()
    if model.n_classes != 1:
        raise RuntimeError("the plastic head needs n_classes == 1 (activin = x.view(nbf, nbf))")
    B, C, Hh, Ww = x.shape
    if C != model.n_channels:
        raise RuntimeError("expected input with %d channels, got %d" % (model.n_channels, C))
    if Hh * Ww != model.nbf * model.nbf or Hh != Ww:
        raise RuntimeError("shape '[%d, %d]' is invalid for input of size %d" % (model.nbf, model.nbf, Hh * Ww))
    model._check_side(Hh)
    H = hebb.unsqueeze(0) if single else hebb
    if H.shape != (B if not seq else 1, model.nbf, model.nbf):
        raise ValueError("hebb must be [nbf,nbf] or [B,nbf,nbf]; got %s for batch %d" % (tuple(hebb.shape), B))
    if x.dtype != torch.float32:
        x = x.float()
    return x, H


def run_trunk_and_head(model, x, hebb, H, single, seq):
    """Trunk (HIP kernel schedule, one autograd node), then the plastic head: fused with the
    outconv where it can be, else the sequential or the per-slot head.  -> (Y, hebb')."""
    from punet.trunk_base import TrunkFunction
    from punet.head import (PlasticHeadFunction, SequentialHeadFunction, FusedHeadFunction, RULES,
                            fused_head_ok)
    trunk = model._trunk_plan()
    trunk.training = model.training     # Dropout2d; BatchNorm: per-slot batch statistics vs running statistics
    params = trunk.params
    save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    wo, bo = model.outc.conv.weight, model.outc.conv.bias
    trunk.fused_head = fused_head_ok(wo.shape[1], model.nbf, seq)
    logits = TrunkFunction.apply(trunk, save, x, *params)
    rule = RULES[model.rule]
    if trunk.fused_head:
        sink = None if trunk.gradbuf is None else (trunk.gradbuf, model.w, model.alpha, wo, bo)
        Y, Hn = FusedHeadFunction.apply(logits, wo, bo, H, model.w, model.alpha, model.eta, rule, True, sink,
                                        model.trace_grad)
        return (Y[0], Hn[0]) if single else (Y, Hn)
    sink = None if trunk.gradbuf is None else (trunk.gradbuf, model.w, model.alpha)
    if seq:
        Y, Hn = SequentialHeadFunction.apply(logits, hebb, model.w, model.alpha, model.eta, rule, sink)
        return (Y[0], Hn) if x.shape[0] == 1 else (Y, Hn)
    Y, Hn = PlasticHeadFunction.apply(logits, H, model.w, model.alpha, model.eta, rule, True, sink, model.trace_grad)
    return (Y[0], Hn[0]) if single else (Y, Hn)
