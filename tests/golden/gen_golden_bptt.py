"""Generate the golden vectors that pin the oracle's UN-DETACHED trace path to the reference itself.

Same conventions as gen_golden.py: runs only in the build container, where yaricom/Plastic-UNet is
mounted read-only at /root/reference; it imports the reference's own ``src/unet`` package, runs it
on seeded inputs on the CPU and writes data only (inputs + the reference's outputs).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bptt.py

The reference's forward leaves the trace update differentiable (unet_p.py:69-88); only its
training loop cuts the path (train.py:97-99).  Here the reference UNetp runs a 3-sample episode
twice, once carrying ``hebb`` as returned (live) and once detaching it between the samples (cut),
with loss = mean of the three BCE losses and one backward.

Fixtures (each < 2 MB):
  bptt_{hebb,oja}.npz   the seeded default UNetp (torch.manual_seed(0), unet_p.py defaults) at 64x64
                        with alpha = 0.5 rand and eta = 0.1 (at the default init the trace path is
                        ~1e-4 of the gradient): inputs, raised alpha / eta, and for both runs the
                        losses, the final trace, the gradients of eta, w, alpha and outc, and
                        (sum, sum|.|, norm) of every trunk gradient in fp64
"""
import os
import sys

import numpy as np

REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))

if not os.path.isdir(REF):
    print("reference not present; nothing to generate")
    sys.exit(0)
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

torch.set_num_threads(8)
from unet import UNetp  # noqa: E402  (the reference package)

CPU = torch.device("cpu")
FULL = ("w", "alpha", "eta", "outc.conv.weight", "outc.conv.bias")


def t2n(t):
    return t.detach().cpu().numpy().copy()


def run(net, xs, ts, hebb0, live):
    net.zero_grad()
    for p in net.parameters():
        p.grad = None
    crit = nn.BCELoss()
    hebb = hebb0.clone()
    losses = []
    for k in range(xs.shape[0]):
        y, hebb = net(xs[k], hebb if live else hebb.detach())
        losses.append(crit(y.view(-1), ts[k].view(-1)))
    (sum(losses) / len(losses)).backward()
    tag = "live." if live else "cut."
    arr = {tag + "losses": np.array([l.item() for l in losses], np.float64), tag + "hebb": t2n(hebb)}
    for k, p in net.named_parameters():
        if p.grad is None:
            assert k == "eta" and not live
            continue
        if k in FULL:
            arr[tag + "g." + k] = t2n(p.grad)
        else:
            g = t2n(p.grad).astype(np.float64)
            arr[tag + "gsum." + k] = np.array([g.sum(), np.abs(g).sum(), np.sqrt((g ** 2).sum())])
    return arr


def gen_bptt():
    N, K = 64, 3
    for rule in ("hebb", "oja"):
        torch.manual_seed(0)
        net = UNetp(1, 1, CPU, rule=rule, nbf=N)
        g = torch.Generator().manual_seed(41 + (rule == "oja"))
        with torch.no_grad():
            net.alpha.copy_(0.5 * torch.rand(N, N, generator=g))
            net.eta.fill_(0.1)
        xs = torch.rand(K, 1, 1, N, N, generator=g)
        ts = (torch.rand(K, N, N, generator=g) > 0.5).float()
        hebb0 = 0.1 * torch.randn(N, N, generator=g)
        arr = {"xs": t2n(xs), "ts": t2n(ts).astype(np.uint8), "hebb0": t2n(hebb0), "alpha": t2n(net.alpha),
               "eta": t2n(net.eta)}
        arr.update(run(net, xs, ts, hebb0, True))
        arr.update(run(net, xs, ts, hebb0, False))
        path = os.path.join(OUT, "bptt_%s.npz" % rule)
        np.savez_compressed(path, **arr)
        print("wrote %-28s %7.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    gen_bptt()
