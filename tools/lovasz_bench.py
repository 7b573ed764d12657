"""Device time of the Lovasz loss beside the BCE loss.

    python tools/lovasz_bench.py [rounds]

pu_lovasz_fwd + pu_lovasz_bwd (three launches: sort and Jaccard gradient per image, the mean, the
elementwise backward) and pu_bce_fwd + pu_bce_bwd at B 32 x 101^2 and B 32 x 128^2, on the same
probabilities and targets: uniform noise against a noise mask of density 0.39 (every key differs: the
sort does the same work whatever the values), and a smooth field against its own thresholded mask.
HIP-graph replay as tools/rle_bench.py, the cases alternated in one process, best of `rounds` (5) with
the spread over the rounds.  The forward alone is timed too."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def maps(kind, B, side, seed):
    """(y, t) [B, side^2] on the host: noise against a noise mask, or a smooth field against its mask"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "noise":
        return torch.rand(B, side * side, generator=g), (torch.rand(B, side * side, generator=g) < 0.39).float()
    coarse = torch.rand(2, B, 1, max(side // 16, 2), max(side // 16, 2), generator=g)
    field = [torch.nn.functional.interpolate(c, size=(side, side), mode="bicubic", align_corners=False)[:, 0] for c in coarse]
    y = torch.sigmoid(12.0 * (field[0] - 0.5)).reshape(B, -1).contiguous()
    return y, (field[0] + 0.2 * (field[1] - 0.5) > 0.5).float().reshape(B, -1).contiguous()


def lovasz(y, t, one):
    _, _, D = K.lovasz_fwd(y, t)
    K.lovasz_bwd(D, one)


def bce(y, t, one):
    K.bce_fwd(y.view(-1), t.view(-1))
    K.bce_bwd(y.view(-1), t.view(-1), one)


print("build %s  (best of %d rounds)" % (_lib.build_id(), rounds))
one = torch.ones((), device=dev)
cases = []
for B, side in ((32, 101), (32, 128)):
    for kind in ("noise", "smooth"):
        y, t = (a.to(dev) for a in maps(kind, B, side, 0))
        for name, fn in (("lovasz fwd+bwd", lambda y=y, t=t: lovasz(y, t, one)), ("lovasz fwd", lambda y=y, t=t: K.lovasz_fwd(y, t)),
                         ("bce fwd+bwd", lambda y=y, t=t: bce(y, t, one))):
            cases.append(((B, side, kind, name), fn))
times = {c[0]: [] for c in cases}
modes = {c[0]: set() for c in cases}
for _ in range(rounds):
    for key, fn in cases:
        us, how = bench._launch_time_us(fn, 20)
        times[key].append(us)
        modes[key].add(how)
for key, _ in cases:
    tm = times[key]
    print("B %2d x %3d^2  %-6s %-15s %8.2f us  (rounds %s, spread %.2f us, %s)" % (
        key + (min(tm), " ".join("%.2f" % x for x in tm), max(tm) - min(tm), "/".join(sorted(modes[key])))))
