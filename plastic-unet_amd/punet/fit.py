"""Data of one size on a net of another (``--fit pad|resize --net-size S``), on top of kernels.fit.

The TGS images are 101 x 101 and a submission is scored at that size, while UNetp wants a side that is a
multiple of 2^(depth-1), 128 for the headline configurations.  A FitSpec says how a batch at the data size
becomes one at the net's side S and how a prediction at S comes back:

  pad     to_net: reflected borders (the edge pixel not repeated), (S - h) // 2 rows above and (S - w) // 2
          columns before the data - numpy.pad(mode='reflect');  to_data: the crop of that window.  Bit copies:
          a binary mask stays binary, and to_data(to_net(x)) is x.
  resize  to_net and to_data: bilinear with zeros outside (skimage's resize(order=1, mode='constant'), the one
          utils/data_set.py applies on the host when --img-size differs from the files' size).

Both run on the device (pu_fit, include/plastic_unet.h).  The data keep their own size on the host, in the
pinned buffers and through augmentation; the prefetcher (punet/loader.py) or the resident path (train.py)
fits each training batch, image and mask alike, and every prediction path comes back to the data size inside
punet.augment.tta_forward before anything is thresholded, scored or encoded.
"""
from . import kernels as K

FIT_MODES = ("pad", "resize")


class FitSpec:
    """mode 'pad' or 'resize' (None: off, a false spec), the data's (h, w) and the net's side S."""

    def __init__(self, mode=None, data_hw=None, net_side=None):
        self.mode = mode or None
        if self.mode is None:
            self.h = self.w = self.side = self.top = self.left = 0
            return
        if self.mode not in FIT_MODES:
            raise ValueError("fit: mode must be 'pad' or 'resize', not %r" % (mode,))
        if net_side is None:
            raise ValueError("fit: %s needs the net's side (--net-size)" % self.mode)
        if data_hw is None or len(tuple(data_hw)) != 2:
            raise ValueError("fit: %s needs the data's (h, w), got %r" % (self.mode, data_hw))
        self.h, self.w, self.side = int(data_hw[0]), int(data_hw[1]), int(net_side)
        if self.h != self.w or self.h < 1:
            raise ValueError("fit: the data must be square (got %d x %d): the net's plane is" % (self.h, self.w))
        if self.side < self.h:
            raise ValueError("fit: the net's side %d is below the data's %d" % (self.side, self.h))
        if self.mode == "pad" and self.side > 2 * min(self.h, self.w) - 1:
            raise ValueError("fit: pad to %d above 2 min(h %d, w %d) - 1: a reflection would leave the image" % (
                self.side, self.h, self.w))
        self.top, self.left = (self.side - self.h) // 2, (self.side - self.w) // 2

    def __bool__(self):
        return self.mode is not None

    def __eq__(self, other):
        return isinstance(other, FitSpec) and (self.mode, self.h, self.w, self.side) == (other.mode, other.h, other.w, other.side)

    def __repr__(self):
        return "FitSpec(%r, (%d, %d), %d)" % (self.mode, self.h, self.w, self.side) if self else "FitSpec(None)"

    def _check(self, t, hw, what):
        if not self:
            raise ValueError("fit: %s of an empty spec" % what)
        if t.dim() < 2 or tuple(t.shape[-2:]) != hw:
            raise ValueError("fit: %s takes [..., %d, %d] (got shape %s)" % ((what,) + hw + (tuple(t.shape),)))

    def to_net(self, x, out=None):
        """x [..., h, w] at the data size -> [..., S, S]: padded, or resized up"""
        self._check(x, (self.h, self.w), "to_net")
        if self.mode == "pad":
            return K.fit(x, self.side, "pad", self.top, self.left, out=out)
        return K.fit(x, self.side, "resize", out=out)

    def to_data(self, y, out=None):
        """y [..., S, S] at the net's side -> [..., h, w]: the crop of the padded window, or resized back"""
        self._check(y, (self.side, self.side), "to_data")
        if self.mode == "pad":
            return K.fit(y, (self.h, self.w), "crop", self.top, self.left, out=out)
        return K.fit(y, (self.h, self.w), "resize", out=out)


def parse_fit(text, data_hw=None, net_side=None):
    """'pad' or 'resize' with the data's (h, w) and the net's side -> FitSpec; '' and None mean off (a false
    spec, whatever the sizes).  A FitSpec passes through."""
    if isinstance(text, FitSpec):
        return text
    text = (text or "").strip()
    if not text:
        return FitSpec()
    return FitSpec(text, data_hw, net_side)
