"""Device time of the augmentation kernels next to a device copy of the same bytes, and the step time of a
training loop fed by the prefetcher with and without an augmentation plan.

    python tools/augment_bench.py [rounds]

1. pu_augment (image and mask plane per slot, random rows within +-8, flips on) and pu_flip_mean at
   B 32 x 101^2, B 32 x 128^2 and B 16 x 512^2, and as the yardstick torch's device-to-device copy_ of the
   bytes pu_augment moves (both planes: every byte read once and written once, as the kernel does).
   pu_augment is timed three times: with the random rows, with all-zero rows ("identity": source and
   destination rows equally aligned, as in the copy) and with every slot mirrored but not shifted ("mirror"),
   to tell what the shifted source rows cost from what the kernel's 4-byte lanes cost.
   HIP-graph replay as tools/rle_bench.py, the cases alternated in one process, best of `rounds` (5) with
   the spread over the rounds.  The two small shapes are a few hundred KB to 4 MB: launch-bound, recorded
   next to the copy; at 16 x 512^2 (32 MB each way) the ratio to the copy is the figure of merit.
2. A Trainer loop (UNetp depth 4, base 16, 128^2, batch 32, 8 steps per epoch) fed by BatchPrefetcher, ten
   epochs (80 steps) per timing with a synchronise at both ends, with and without a plan ("hflip,shift:8"),
   alternated `rounds` times in one process after one untimed epoch of each; best, median and spread."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
from punet.augment import AugmentPlan, mirror_table  # noqa: E402
from punet.engine import Trainer  # noqa: E402
from punet.loader import BatchPrefetcher  # noqa: E402
from unet import UNetp  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
S = 8

print("build %s  (best of %d rounds)" % (_lib.build_id(), rounds))
cases = []
for B, side in ((32, 101), (32, 128), (16, 512)):
    g = torch.Generator(device="cpu").manual_seed(side)
    x, t = torch.rand(B, 1, side, side, generator=g).to(dev), torch.rand(B, 1, side, side, generator=g).to(dev)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    rows = torch.from_numpy(AugmentPlan("hflip,shift:%d" % S, B, side).table(0)).to(dev)
    zero, mirror = torch.zeros_like(rows), torch.from_numpy(mirror_table(B)).to(dev)
    both, both_o = torch.cat([x, t]), torch.empty(2 * B, 1, side, side, device=dev)      # the copy: the same bytes, one call
    y, ym, yo = x[:, 0].contiguous(), t[:, 0].contiguous(), torch.empty(B, side, side, device=dev)
    cases.append((B, side, {
        "augment": (lambda x=x, t=t, rows=rows, xo=xo, to=to: K.augment(x, t, rows, S, out=(xo, to)), 16.0 * B * side * side),
        "identity": (lambda x=x, t=t, rows=zero, xo=xo, to=to: K.augment(x, t, rows, S, out=(xo, to)), 16.0 * B * side * side),
        "mirror": (lambda x=x, t=t, rows=mirror, xo=xo, to=to: K.augment(x, t, rows, S, out=(xo, to)), 16.0 * B * side * side),
        "copy_": (lambda both=both, both_o=both_o: both_o.copy_(both), 16.0 * B * side * side),
        "flip_mean": (lambda y=y, ym=ym, yo=yo: K.flip_mean(y, ym, out=yo), 12.0 * B * side * side)}))
times = {}
for _ in range(rounds):
    for B, side, fns in cases:
        for name, (fn, _) in fns.items():
            us, how = bench._launch_time_us(fn, 20)
            times.setdefault((B, side, name), []).append(us)
for B, side, fns in cases:
    for name, (_, nbytes) in fns.items():
        tm = times[(B, side, name)]
        print("B %2d x %3d^2  %-9s %8.2f us  (rounds %s, spread %.2f us, %s)  %5.1f MB moved: %.0f GB/s" % (
            B, side, name, min(tm), " ".join("%.2f" % v for v in tm), max(tm) - min(tm), how, nbytes / 1e6,
            nbytes / min(tm) / 1e3))
    print("B %2d x %3d^2  augment / copy_ = %.3f" % (B, side, min(times[(B, side, "augment")]) / min(times[(B, side, "copy_")])))

# ---- the training loop under the prefetcher
N, side, bs = 256, 128, 32
g = np.random.RandomState(0)
X = g.rand(N, 1, side, side).astype(np.float32)
Y = (g.rand(N, 1, side, side) > 0.5).astype(np.float32)
ranges = [(lo, lo + bs) for lo in range(0, N, bs)]
torch.manual_seed(0)
net = UNetp(1, 1, dev, rule="oja", nbf=side, depth=4, base_ch=16)
trainer = Trainer(net, lr=3e-5, steplr=1e6, gamma=0.666)
feeds = {"plain": BatchPrefetcher(X, Y, ranges, dev), "augment": BatchPrefetcher(X, Y, ranges, dev, augment=AugmentPlan("hflip,shift:%d" % S, N, 0))}
epoch = 0


def epochs(feed, count):
    """seconds per step over `count` epochs"""
    global epoch
    net.train()
    hebb = net.initialZeroHebb(bs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        feed.set_epoch(epoch)
        epoch += 1
        for (lo, hi), (x, yb) in zip(ranges, feed):
            _, hebb = trainer.step(x, yb.reshape(hi - lo, -1), hebb)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (count * len(ranges))


for feed in feeds.values():
    epochs(feed, 1)                     # untimed: first launches, pools, pinned buffers
step = {name: [] for name in feeds}
for r in range(rounds):
    for name, feed in feeds.items():
        step[name].append(epochs(feed, 10) * 1e3)
print("training loop: UNetp depth 4 base 16, %d^2, batch %d, %d steps per epoch, prefetcher depth 2" % (side, bs, len(ranges)))
for name, tm in step.items():
    print("  %-8s %7.3f ms / step best, %7.3f median  (rounds %s, spread %.3f ms)" % (
        name, min(tm), float(np.median(tm)), " ".join("%.3f" % v for v in tm), max(tm) - min(tm)))
print("  augment / plain = %.4f (best of each), %.4f (medians)" % (
    min(step["augment"]) / min(step["plain"]), float(np.median(step["augment"]) / np.median(step["plain"]))))
