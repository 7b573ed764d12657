"""Device time of gradient clipping on C2's real parameter list (UNetp depth 5 / base 64, 14.81 M
parameters in their own tensor sizes, the gradients laid out in a GradBuffer as the Trainer holds them):
pu_grad_norm (its grad_sumsq launches + the finish), pu_adam_multi_clipped and pu_adam_multi, alternated
in one process, HIP-graph replay as tools/head_bench.py, best of 5 rounds with the spread over the rounds.

    python tools/clip_bench.py [rounds]

Prints us per call and the share of 8 TB/s the byte floors come to (4 B per parameter + 8 B per 4096-
element chunk for the norm, 28 B per parameter for Adam)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from punet import _lib, dp, kernels as K  # noqa: E402
from unet import UNetp  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
torch.manual_seed(0)
net = UNetp(1, 1, dev, rule="oja", nbf=128, depth=5, base_ch=64)
params = [p.detach() for p in net.parameters() if p is not net.eta]
buf = dp.GradBuffer(params, dev)
for v in buf.views:
    v.normal_(0.0, 1e-3)
grads = buf.views
ms = [torch.zeros_like(p) for p in params]
vs = [torch.zeros_like(p) for p in params]
n = sum(p.numel() for p in params)
chunks = sum(-(-p.numel() // 4096) for p in params)
scale = K.grad_norm(grads, 1.0)[1:]
sc = (0.9, 0.999, 1e-8, 0.0, 1e-9, 1.0)        # a step of 1e-9: the parameters stay where they are
cases = (("grad_norm", lambda: K.grad_norm(grads, 1.0), 4.0 * n + 8.0 * chunks),
         ("adam_multi", lambda: K.adam_multi(params, grads, ms, vs, *sc), 28.0 * n),
         ("adam_multi_clipped", lambda: K.adam_multi(params, grads, ms, vs, *sc, grad_scale=scale), 28.0 * n))
times = {label: [] for label, _, _ in cases}
for _ in range(rounds):
    for label, fn, _ in cases:
        us, how = bench._launch_time_us(fn, 20)
        times[label].append(us)
print("build %s  %d tensors, %.2f M parameters, %d chunks  (%s, best of %d rounds)" % (
    _lib.build_id(), len(params), n / 1e6, chunks, how, rounds))
for label, _, nbytes in cases:
    t = times[label]
    print("%-20s %8.2f us  (rounds %s, spread %.2f us)  %6.1f MB floor: %.0f GB/s, %.3f of 8 TB/s" % (
        label, min(t), " ".join("%.2f" % x for x in t), max(t) - min(t), nbytes / 1e6, nbytes / min(t) / 1e3,
        nbytes / min(t) / 8e6))
d = min(times["adam_multi_clipped"]) - min(times["adam_multi"])
print("clipped - plain Adam: %+.2f us (spreads %.2f / %.2f us)" % (
    d, max(times["adam_multi_clipped"]) - min(times["adam_multi_clipped"]),
    max(times["adam_multi"]) - min(times["adam_multi"])))
