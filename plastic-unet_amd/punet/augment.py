"""Training augmentation and test-time augmentation on top of kernels.augment / kernels.flip_mean.

Training (``train.py --augment hflip,shift:8``): every epoch each sample gets a fresh random row
{flip, dy, dx, 0}; its image and mask planes are translated by (dy, dx) with reflected borders and then
mirrored left-right when flip is set (pu_augment, include/plastic_unet.h).  The rows are drawn on the
host, one table per epoch (AugmentPlan), and applied on the device: by the prefetcher on its copy stream
(punet/loader.py) or, with the training set resident, per batch slice (train.py).

Inference (``--tta hflip``): the prediction of a batch is the mean of the net's output on the images and
its un-mirrored output on the mirrored images (tta_forward), merged on the device so that the threshold,
the metrics and the run-length encoding that follow stay there.  With a FitSpec (punet/fit.py: the net's side is
not the data's) each of the two forwards is fitted to the net and brought back, and the merge is at the data size.
"""
import numpy as np
import torch

from . import kernels as K

TTA_MODES = (None, "hflip")


class AugmentSpec:
    """What --augment asks for: hflip (random left-right mirror) and shift (the largest |dy|, |dx| of the
    random reflected translation, 0: none)."""

    def __init__(self, hflip=False, shift=0):
        self.hflip, self.shift = bool(hflip), int(shift)

    def __bool__(self):
        return self.hflip or self.shift > 0

    def __eq__(self, other):
        return isinstance(other, AugmentSpec) and (self.hflip, self.shift) == (other.hflip, other.shift)

    def __repr__(self):
        return "AugmentSpec(hflip=%r, shift=%d)" % (self.hflip, self.shift)

    def check_fits(self, h, w):
        """A reflection must stay inside the plane: shift <= min(h, w) - 1."""
        if self.shift > min(h, w) - 1:
            raise ValueError("augment: shift %d above min(h %d, w %d) - 1" % (self.shift, h, w))
        return self


def parse_augment(text, hw=None):
    """'hflip', 'shift:S' or both, comma-separated -> AugmentSpec; '' and None mean off (a false spec).
    hw: the (h, w) of the images, to refuse a shift above min(h, w) - 1 here already."""
    if isinstance(text, AugmentSpec):
        spec = text
    else:
        spec = AugmentSpec()
        for word in (text or "").split(","):
            word = word.strip()
            if not word:
                continue
            if word == "hflip":
                spec.hflip = True
            elif word.startswith("shift"):
                head, sep, value = word.partition(":")
                if head != "shift" or not sep or not value.strip().isdigit():     # a sign is no digit: negative refused
                    raise ValueError("augment: %r must be shift:S with an integer S >= 0" % word)
                spec.shift = int(value)
            else:
                raise ValueError("augment: unknown transform %r (hflip, shift:S)" % word)
    if hw is not None:
        spec.check_fits(*hw)
    return spec


class AugmentPlan:
    """The augment rows of every sample and epoch: table(epoch) -> int32 [n_samples, 4] of {flip, dy, dx, 0}.

    The table of an epoch comes from numpy's counter-based Philox generator keyed by (seed, epoch), in one
    fixed order of draws whatever the spec is:
      1. flips  = integers(0, 2, n_samples)
      2. shifts = integers(-S, S + 1, (n_samples, 2))      (dy, dx) per sample, S = spec.shift
    and the flips are zeroed when the spec has no hflip (S = 0 draws zeros by itself).  Row i therefore
    depends on (seed, epoch, i) alone - not on the batch size, the number of ranks or how the batches reach
    the device: whoever trains sample i in epoch e reads row i of table(e)."""

    def __init__(self, spec, n_samples, seed):
        self.spec = parse_augment(spec)
        self.n_samples, self.seed = int(n_samples), int(seed)
        if self.n_samples < 0 or self.seed < 0:
            raise ValueError("AugmentPlan: n_samples %d and seed %d must not be negative" % (self.n_samples, self.seed))

    @property
    def max_shift(self):
        return self.spec.shift

    def table(self, epoch):
        if int(epoch) < 0:
            raise ValueError("AugmentPlan: epoch %d is negative" % epoch)
        rng = np.random.Generator(np.random.Philox(key=[self.seed, int(epoch)]))
        S, n = self.spec.shift, self.n_samples
        flips = rng.integers(0, 2, n)
        shifts = rng.integers(-S, S + 1, (n, 2))
        rows = np.zeros((n, 4), dtype=np.int32)
        if self.spec.hflip:
            rows[:, 0] = flips
        rows[:, 1:3] = shifts
        return rows


def mirror_table(batch):
    """int32 [batch, 4] of {1, 0, 0, 0}: every slot mirrored, nothing shifted (the second view of TTA)."""
    rows = np.zeros((int(batch), 4), dtype=np.int32)
    rows[:, 0] = 1
    return rows


_MIRROR_DEV = {}


def _mirror_rows(batch, device):
    """mirror_table for K.augment: on a ROCm device one resident copy per (device, batch) - no upload per chunk"""
    if device.type != "cuda":
        return mirror_table(batch)
    key = (device.index, batch)
    if key not in _MIRROR_DEV:
        _MIRROR_DEV[key] = torch.from_numpy(mirror_table(batch)).to(device)
    return _MIRROR_DEV[key]


def check_tta(tta):
    if tta not in TTA_MODES:
        raise ValueError("tta must be None or 'hflip', not %r" % (tta,))


def tta_forward(net, xb, tta=None, fit=None):
    """The zero-trace forward every prediction path goes through: xb [B, C, H, W] -> probabilities.
    tta None: net(xb, zero trace) as it is.  'hflip': two forwards of the same batch size, each with a
    fresh zero trace - xb, then xb mirrored left-right (kernels.augment with mirror_table) - merged by
    kernels.flip_mean: 0.5 * (y + mirror(y_mirror)), on the device.
    fit: None, or the punet.fit.FitSpec of a net whose side is not the data's: a forward is then
    P(x) = fit.to_data(net(fit.to_net(x), zero trace)), so xb and the result are at the data size, and so are
    the mirror and the merge of 'hflip'."""
    check_tta(tta)
    B = xb.shape[0]

    def forward(x):
        y, _ = net(fit.to_net(x.contiguous()) if fit else x, net.initialZeroHebb(B))
        return fit.to_data(y.contiguous()) if fit else y

    y = forward(xb)
    if tta is None:
        return y
    xm, _ = K.augment(xb.contiguous(), None, _mirror_rows(B, xb.device), 0)
    return K.flip_mean(y.contiguous(), forward(xm).contiguous())
