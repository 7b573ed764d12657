"""Device time of pu_fit next to torch's own operators on the same tensors.

    python tools/fit_bench.py [rounds]

Batch 32 of 101^2 planes to 128^2 and back - the TGS images on the 128^2 net - and 16 x 512^2 to 640^2 as a
shape where bytes, not the launch, are what is timed:
  pad      kernels.fit(x, S, 'pad', top, left)         against  torch.nn.functional.pad(x, ..., mode='reflect')
  crop     kernels.fit(y, s, 'crop', top, left)        against  y[..., top:top+s, left:left+s].contiguous()
  resize   kernels.fit(x, S, 'resize') and back        against  torch.nn.functional.interpolate(mode='bilinear',
           align_corners=False) - not the same function at the frame (it clamps where pu_fit reads zeros), timed
           as the nearest operator torch has
HIP-graph replay as tools/augment_bench.py, the cases alternated in one process, best of `rounds` (5) with the
spread over the rounds.  Bytes moved: every output word written once, and read once what it is made of."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5

print("build %s  (best of %d rounds)" % (_lib.build_id(), rounds))


def make_case(B, s, S):
    g = torch.Generator(device="cpu").manual_seed(s)
    x, y = torch.rand(B, 1, s, s, generator=g).to(dev), torch.rand(B, 1, S, S, generator=g).to(dev)
    xo, yo = torch.empty_like(x), torch.empty_like(y)
    top = left = (S - s) // 2
    frame = (left, S - s - left, top, S - s - top)
    small, large = 4.0 * B * s * s, 4.0 * B * S * S
    assert torch.equal(K.fit(x, S, "pad", top, left), TF.pad(x, frame, mode="reflect"))
    assert torch.equal(K.fit(y, s, "crop", top, left), y[..., top:top + s, left:left + s])
    return B, s, S, {
        "pu_fit pad": (lambda: K.fit(x, S, "pad", top, left, out=yo), small + large),
        "torch pad reflect": (lambda: TF.pad(x, frame, mode="reflect"), small + large),
        "pu_fit crop": (lambda: K.fit(y, s, "crop", top, left, out=xo), 2 * small),
        "torch slice+contiguous": (lambda: y[..., top:top + s, left:left + s].contiguous(), 2 * small),
        "pu_fit resize up": (lambda: K.fit(x, S, "resize", out=yo), small + large),
        "torch interpolate up": (lambda: TF.interpolate(x, size=(S, S), mode="bilinear", align_corners=False), small + large),
        "pu_fit resize down": (lambda: K.fit(y, s, "resize", out=xo), 5 * small),
        "torch interpolate down": (lambda: TF.interpolate(y, size=(s, s), mode="bilinear", align_corners=False), 5 * small)}


cases = [make_case(32, 101, 128), make_case(16, 512, 640)]
times = {}
for _ in range(rounds):
    for B, s, S, fns in cases:
        for name, (fn, _) in fns.items():
            us, how = bench._launch_time_us(fn, 20)
            times.setdefault((B, s, name), []).append(us)
for B, s, S, fns in cases:
    for name, (_, nbytes) in fns.items():
        tm = times[(B, s, name)]
        print("B %2d x %3d^2 <-> %3d^2  %-24s %8.2f us  (rounds %s, spread %.2f us, %s)  %5.1f MB moved: %.0f GB/s" % (
            B, s, S, name, min(tm), " ".join("%.2f" % v for v in tm), max(tm) - min(tm), how, nbytes / 1e6,
            nbytes / min(tm) / 1e3))
