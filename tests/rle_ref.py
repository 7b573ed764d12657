"""What tests/test_rle.py and tests/test_rle_gpu.py share: the run table of kernels.rle_encode restated
in numpy on top of utils.encode, the threshold bound of the entry, and the masks the tests plant."""
import numpy as np
import torch


def bound_above(th):
    """The smallest fp32 above the double th (csrc/rle.hip): y >= it  <=>  float64(y) > th."""
    f = np.float32(th)
    if np.float64(f) <= th:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def pairs_of(mask):
    """[runs, 2] int32 (start, length) of one mask, from the string utils.encode prints."""
    from utils import encode
    return np.array(encode(np.round(mask)).split(), dtype=np.int32).reshape(-1, 2)


def table_of(y, th):
    """(offsets [B + 1], runs [total, 2]) int32 of the maps y [B, H, W] under float64(y) > th."""
    per = [pairs_of(m.astype(np.float64) > th) for m in np.asarray(y)]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    return offsets, np.concatenate(per, 0).astype(np.int32).reshape(-1, 2)


def numpy_rle_encode(calls):
    """kernels.rle_encode on CPU tensors, for the host-side plumbing"""
    def rle_encode(y, threshold, cap=None):
        calls.append((y.shape[0], threshold))
        B, H, W = y.shape
        offsets, runs = table_of(y.numpy(), threshold)
        cap = B * ((H * W + 1) // 2) if cap is None else cap
        out = np.full((cap, 2), -7, dtype=np.int32)
        out[:min(cap, len(runs))] = runs[:cap]
        return torch.from_numpy(offsets), torch.from_numpy(out)
    return rle_encode


def planted_masks(h, w, seed=0):
    """{name: bool [h, w]}: the masks of the issue, column-major where that matters"""
    n = h * w
    g = np.random.RandomState(seed + 131 * h + w)

    def colmajor(flat):
        return np.asarray(flat, dtype=bool).reshape(w, h).T.copy()
    rows = np.zeros((h, w), dtype=bool)
    rows[0], rows[-1] = True, True
    last, first = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    last[-1], first[0] = True, True
    out = {"empty": np.zeros((h, w), dtype=bool), "full": np.ones((h, w), dtype=bool),
           "alternating": colmajor(np.arange(n) % 2 == 0), "top and bottom rows": rows,
           "last pixel": colmajor(last), "first pixel": colmajor(first)}
    for density in (0.02, 0.5, 0.98):
        out["random %.2f" % density] = g.rand(h, w) < density
    return out


def maps_of(masks, th=0.5, seed=0):
    """fp32 maps whose pixels lie on the mask's side of th, at random distances"""
    masks = np.asarray(masks)
    u = np.random.RandomState(seed).rand(*masks.shape).astype(np.float32)
    return np.where(masks, np.float32(th) + np.float32(0.01) + np.float32(0.4) * u,
                    np.float32(th) - np.float32(0.01) - np.float32(0.4) * u).astype(np.float32)
