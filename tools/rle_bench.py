"""Device time of the run-length encoding and the wall time of infer.predict, device path against
host path.

    python tools/rle_bench.py [rounds]

1. pu_rle_encode (its three launches) at B 32 x 101^2, B 32 x 128^2 and B 16 x 512^2 on two kinds of
   mask: noise at density 0.5 (about n / 4 runs per image, the bad case) and a thresholded smooth field
   (a few runs per column, the realistic one).  HIP-graph replay as tools/metrics_bench.py, the cases
   alternated in one process, best of `rounds` (5) with the spread over the rounds, next to the 4 B per
   pixel floor and the share of 8 TB/s it comes to.
2. infer.predict on 800 synthetic 101^2 images with a small UNetpRes (neurons 8), wall time with a
   synchronise at both ends, rle="device" and rle="host" alternated three times in one process (after
   one untimed pass of each), for both kinds of mask.  The model's forward runs as it is; to choose the
   kind of mask its probabilities are then replaced by the planted maps of the same images (a copy of
   4 B per pixel on the device, the same on both paths)."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
from unet import UNetpRes  # noqa: E402
import bench  # noqa: E402
import infer  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def maps(kind, B, side, seed):
    """fp32 probability maps [B, side, side] on the host: noise, or a smooth field through a sigmoid"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "noise":
        return torch.rand(B, side, side, generator=g)
    coarse = torch.rand(B, 1, max(side // 16, 2), max(side // 16, 2), generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(side, side), mode="bicubic", align_corners=False)[:, 0]
    return torch.sigmoid(12.0 * (field - 0.5)).contiguous()


print("build %s  (best of %d rounds)" % (_lib.build_id(), rounds))
cases = []
for B, side in ((32, 101), (32, 128), (16, 512)):
    for kind in ("noise", "smooth"):
        y = maps(kind, B, side, 0).to(dev)
        offsets, _ = K.rle_encode(y, 0.5)
        cases.append((B, side, kind, y, int(offsets[-1].item())))
times = {c[:3]: [] for c in cases}
for _ in range(rounds):
    for B, side, kind, y, _ in cases:
        us, how = bench._launch_time_us(lambda: K.rle_encode(y, 0.5), 20)
        times[(B, side, kind)].append(us)
for B, side, kind, y, pairs in cases:
    tm = times[(B, side, kind)]
    nbytes = 4.0 * B * side * side
    print("B %2d x %3d^2  %-6s %8.1f pairs/image %8.2f us  (rounds %s, spread %.2f us, %s)  %5.1f MB floor: %.0f GB/s, "
          "%.4f of 8 TB/s" % (B, side, kind, pairs / B, min(tm), " ".join("%.2f" % x for x in tm), max(tm) - min(tm), how,
                              nbytes / 1e6, nbytes / min(tm) / 1e3, nbytes / min(tm) / 8e6))

# ---- predict
N, side = 800, 101
X = np.random.RandomState(0).rand(N, 1, side, side).astype(np.float32)
torch.manual_seed(0)
net = UNetpRes(1, 1, dev, neurons=8, rule="oja", nbf=side)


class Planted:
    """the model, its forward run as it is, its probabilities replaced by the planted maps of the chunk"""

    def __init__(self, net, planted):
        self.net, self.planted, self.at = net, planted, 0

    def eval(self):
        self.net.eval()
        self.at = 0
        return self

    def parameters(self):
        return self.net.parameters()

    def initialZeroHebb(self, B):
        return self.net.initialZeroHebb(B)

    def __call__(self, x, hebb):
        y, h = self.net(x, hebb)
        y.copy_(self.planted[self.at:self.at + x.shape[0]])
        self.at += x.shape[0]
        return y, h


ids = ["i%d" % i for i in range(N)]
with tempfile.TemporaryDirectory() as out:
    params = {"device": dev, "mask_threshold": 0.5, "out_dir": out}
    for kind in ("noise", "smooth"):
        model = Planted(net, maps(kind, N, side, 1).to(dev))

        def one_pass(rle):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = infer.predict(model, (ids, X), dict(params, subm_file=rle + ".csv"), rle=rle)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, rows
        res = {rle: one_pass(rle) for rle in ("device", "host")}          # untimed: first launches, pools
        chars = sum(len(r[1]) for r in res["device"][1])
        print("predict: %d images of %d^2, UNetpRes neurons 8, batch 32, %s masks (%.0f characters per row); rows equal: %s" % (
            N, side, kind, chars / N, res["device"][1] == res["host"][1]))
        wall = {"device": [], "host": []}
        for r in range(3):
            for rle in ("device", "host"):
                wall[rle].append(one_pass(rle)[0])
                print("  round %d  %-6s predict %8.1f ms" % (r, rle, wall[rle][-1] * 1e3))
        print("  host / device: %.2f (best of each)" % (min(wall["host"]) / min(wall["device"])))
