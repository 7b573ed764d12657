"""Device time of the validation metrics and the wall time of a validation pass, device path against
host path.

    python tools/metrics_bench.py [rounds]

1. pu_seg_metrics (its two launches) at B 32 x 128^2, B 32 x 101^2 and B 16 x 512^2, each with no
   threshold (eval_net) and with the 31 thresholds of score_model_best_iou, next to the B pu_bce_fwd
   calls it replaces in eval_net; HIP-graph replay as tools/clip_bench.py, best of `rounds` (5) with the
   spread over the rounds, and the share of 8 TB/s its 8 B per pixel come to.
2. eval_net plus score_model_best_iou on 800 synthetic 101^2 samples with a small UNetpRes (neurons 8;
   UNetp takes no odd image side), wall time with a synchronise at both ends, device and host path
   alternated three times in one process (after one untimed pass of each)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
from unet import UNetpRes  # noqa: E402
import bench  # noqa: E402
import eval as ev  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOGIT_TH = np.log(np.linspace(0.3, 0.7, 31) / (1 - np.linspace(0.3, 0.7, 31)))
g = torch.Generator(device="cpu").manual_seed(0)

print("build %s  (best of %d rounds)" % (_lib.build_id(), rounds))
for B, side in ((32, 128), (32, 101), (16, 512)):
    n = side * side
    y = torch.rand(B, n, generator=g).to(dev)
    t = (torch.rand(B, n, generator=g) > 0.5).float().to(dev)
    cases = (("seg_metrics T=0", lambda: K.seg_metrics(y, t)),
             ("seg_metrics T=31", lambda: K.seg_metrics(y, t, LOGIT_TH)),
             ("%d x bce_fwd" % B, lambda: [K.bce_fwd(y[b], t[b]) for b in range(B)]))
    times = {label: [] for label, _ in cases}
    for _ in range(rounds):
        for label, fn in cases:
            us, how = bench._launch_time_us(fn, 20)
            times[label].append(us)
    nbytes = 8.0 * B * n
    for label, _ in cases:
        tm = times[label]
        print("B %2d x %3d^2  %-17s %8.2f us  (rounds %s, spread %.2f us, %s)  %5.1f MB floor: %.0f GB/s, %.3f of 8 TB/s" % (
            B, side, label, min(tm), " ".join("%.2f" % x for x in tm), max(tm) - min(tm), how, nbytes / 1e6,
            nbytes / min(tm) / 1e3, nbytes / min(tm) / 8e6))

# ---- a validation pass
N, side = 800, 101
rs = np.random.RandomState(0)
X = rs.rand(N, 1, side, side).astype(np.float32)
Y = (rs.rand(N, 1, side, side) > 0.5).astype(np.float32)
torch.manual_seed(0)
net = UNetpRes(1, 1, dev, neurons=8, rule="oja", nbf=side)


def one_pass(metrics):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc_loss = ev.eval_net(net, X, Y, dev, metrics=metrics)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    best = ev.score_model_best_iou(net, X, Y, dev, metrics=metrics)
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1, acc_loss, best


res = {m: one_pass(m) for m in ("device", "host")}             # untimed: first launches, pools
same = res["device"][2] == res["host"][2] and res["device"][3] == res["host"][3]
print("validation pass: %d samples of %d^2, UNetpRes neurons 8, batch 32; results equal: %s %r %r" % (
    N, side, same, res["device"][2], res["device"][3]))
for r in range(3):
    for m in ("device", "host"):
        e, s, _, _ = one_pass(m)
        print("  round %d  %-6s eval_net %8.1f ms   score_model_best_iou %8.1f ms" % (r, m, e * 1e3, s * 1e3))
