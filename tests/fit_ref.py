"""What tests/test_fit.py and tests/test_fit_gpu.py share: pu_fit restated in numpy, never through the index
formulas of the kernel - the pad as numpy.pad(mode='reflect'), the crop as a slice, the resize as the host
loader's utils.data_set.resize_bilinear_constant in float64 -, the shapes the kernel tests run and the spec's
offsets."""
import numpy as np

from augment_ref import bits, random_words  # noqa: F401  (re-exported for the tests)


def pad(a, H, W, top, left):
    """a [..., h, w] of any dtype -> [..., H, W] with reflected borders, `top` rows above and `left` columns
    before the data.  A copy of elements only: the bits of a survive."""
    a = np.asarray(a)
    h, w = a.shape[-2:]
    return np.ascontiguousarray(np.pad(a, [(0, 0)] * (a.ndim - 2) + [(top, H - h - top), (left, W - w - left)], mode="reflect"))


def crop(a, H, W, top, left):
    return np.ascontiguousarray(np.asarray(a)[..., top:top + H, left:left + W])


def resize(a, H, W):
    """a [..., h, w] -> float64 [..., H, W]: the host loader's bilinear resize of every plane"""
    from utils.data_set import resize_bilinear_constant
    a = np.asarray(a, dtype=np.float64)
    planes = a.reshape((-1,) + a.shape[-2:])
    return np.stack([resize_bilinear_constant(p, (H, W)) for p in planes]).reshape(a.shape[:-2] + (H, W))


def centre(h, w, H, W):
    """the offsets of punet.fit.FitSpec"""
    return (H - h) // 2, (W - w) // 2


# (planes..., h, w) -> (H, W) with the (top, left) offsets to run: a single pixel, maximal reflection on both sides,
# the data set's own sizes at the spec's offsets and at both ends of the range, rows that cross the 64- and the
# 128-column run boundaries, and a height above one block with a width just above one run
PAD_CASES = [
    ((3, 1, 5, 7), (8, 12), [(1, 2), (0, 0), (3, 5)]),
    ((2, 1, 1, 1), (1, 1), [(0, 0)]),
    ((2, 2, 2, 3), (3, 5), [(0, 0), (1, 2), (0, 1)]),
    ((2, 1, 101, 101), (128, 128), [(13, 13), (0, 0), (27, 27)]),
    ((1, 1, 65, 129), (128, 256), [(31, 63), (0, 127), (63, 0)]),
    ((1, 1, 300, 65), (320, 70), [(10, 2), (20, 5), (0, 0)]),
]
