"""FusedAdam: torch.optim.Adam semantics, one multi-tensor HIP launch per step.

Reference: yaricom/Plastic-UNet src/train.py:66 (``torch.optim.Adam(net.parameters(), lr)``) and
:111 (``optimizer.step()``).  Parameters without a gradient (``eta``, S3) are skipped exactly like
torch's Adam skips them.  The state layout (``step``, ``exp_avg``, ``exp_avg_sq``) is torch's, so
optimizer state_dicts move between the two.  StepLR (train.py:67) works unchanged on top.

``max_grad_norm`` (not in the reference): clip the gradients by their global 2-norm as
``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` before ``step()`` would - one norm over
every parameter of every group that has a gradient - with two differences.  The norm is summed on
the device in fp64 in a fixed order (kernels.grad_norm), and the coefficient is applied to each
gradient as Adam reads it: ``.grad`` is left UNSCALED, where torch scales it in place.  After a
step ``grad_norm`` and ``clip_coef`` are 0-d device tensors of that step's norm (before clipping)
and coefficient; reading them does not synchronise.
"""
import math

import torch
from torch.autograd.graph import increment_version

from . import kernels as K


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {}".format(betas))
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError("Invalid max_grad_norm: {} (None turns clipping off)".format(max_grad_norm))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self.clip_coef = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        launches = []
        for group in self.param_groups:
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = int(st["step"].item())
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(t, []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            launches.extend((group, t, items) for t, items in by_step.items())
        scale = None
        if self.max_grad_norm is not None and launches:
            # one norm over the gradients Adam is about to read, before any parameter moves
            out = K.grad_norm([i[1] for _, _, items in launches for i in items], self.max_grad_norm)
            self.grad_norm, self.clip_coef = out[0], out[1]
            scale = out[1:]
        for group, t, items in launches:
            beta1, beta2 = group["betas"]
            bc1 = 1 - beta1 ** t
            bc2 = 1 - beta2 ** t
            step_size = group["lr"] / bc1
            args = ([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items],
                    beta1, beta2, group["eps"], group["weight_decay"], step_size, math.sqrt(bc2))
            if scale is None:
                K.adam_multi(*args)
            else:
                K.adam_multi(*args, grad_scale=scale)
            # the kernel writes through raw pointers: bump the version counters so every cache
            # keyed on them (the trunk's packed / split GEMM operands) sees the new values
            increment_version([i[0] for i in items])
        return loss
