"""The Lovasz loss on probabilities as include/plastic_unet.h states it (rules 1 - 6 of pu_lovasz_fwd),
restated in numpy, and the inputs tests/test_lovasz.py and tests/test_lovasz_gpu.py share.  The order is
np.lexsort on (index, -e) with e in fp32; everything after it is fp64 from integer counts."""
import numpy as np


def foreground(t):
    """rule 1: 0.5 <= t <= 1 (utils.iou_metric._foreground)"""
    t = np.asarray(t, dtype=np.float32)
    return (t >= np.float32(0.5)) & (t <= np.float32(1.0))


def errors(y, t):
    """rule 2: e = fg ? 1.0f - y : y, one fp32 rounding"""
    y = np.asarray(y, dtype=np.float32)
    return np.where(foreground(t), np.float32(1.0) - y, y).astype(np.float32)


def image(y, t):
    """One image, y and t [n] -> (loss_b as fp64 before its rounding, D [n] fp32)."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    fg = foreground(np.asarray(t).reshape(-1))
    e = errors(y, np.asarray(t).reshape(-1))
    n = y.size
    order = np.lexsort((np.arange(n), -e))                     # rule 3: e descending, equal e by index ascending
    f = fg[order].astype(np.int64)
    G = int(f.sum())
    cf = np.cumsum(f)
    cb = np.cumsum(1 - f)
    J = 1.0 - (G - cf).astype(np.float64) / (G + cb).astype(np.float64)     # rule 4
    g = J - np.concatenate([[0.0], J[:-1]])
    loss = float(np.sum(e[order].astype(np.float64) * g))      # rule 5 (numpy's own order of summation)
    D = np.empty(n, dtype=np.float32)
    D[order] = np.where(f == 1, -g, g).astype(np.float32)      # rule 6
    return loss, D


def batch(y, t):
    """y and t [B, n] -> (loss fp64, loss_per_image [B] fp64, D [B, n] fp32); the mean is over the fp32
    roundings of the image losses, in image order."""
    y = np.asarray(y, dtype=np.float32)
    B = y.shape[0]
    per, D = np.empty(B), np.empty((B, y[0].size), dtype=np.float32)
    for b in range(B):
        per[b], D[b] = image(y[b], np.asarray(t)[b])
    total = 0.0
    for b in range(B):
        total += float(np.float32(per[b]))
    return total / B, per, D.reshape(y.shape)


def backward(D, g, B):
    """dy = D * (g / (float)B): one fp32 division, one fp32 multiply per element"""
    return (np.asarray(D, dtype=np.float32) * (np.float32(g) / np.float32(B))).astype(np.float32)


def berman(y, t):
    """lovasz_softmax_flat for the one foreground class with plain cumsums (Berman's lovasz_grad): the
    loss of one image in fp64, any order among equal errors."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    fg = foreground(np.asarray(t).reshape(-1)).astype(np.float64)
    e = np.abs(fg - y)
    order = np.argsort(-e, kind="stable")
    gt = fg[order]
    gts = gt.sum()
    inter = gts - np.cumsum(gt)
    union = gts + np.cumsum(1.0 - gt)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return float(np.dot(e[order], jac)), order, jac


def ulp32(x):
    """the spacing of fp32 at |x| (of the smallest normal below it)"""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


MASKS = ("empty", "full", "one", "random", "fractional")
PROBS = ("uniform", "constant", "eighths", "planted")


def targets(kind, B, n, g):
    if kind == "empty":
        return np.zeros((B, n), dtype=np.float32)
    if kind == "full":
        return np.ones((B, n), dtype=np.float32)
    if kind == "one":
        t = np.zeros((B, n), dtype=np.float32)
        t[np.arange(B), g.randint(0, n, B)] = 1.0
        return t
    if kind == "random":
        return (g.rand(B, n) < g.rand(B, 1)).astype(np.float32)
    if kind == "fractional":                                   # a resized mask: values around 0.5, some above 1
        half = np.float32(0.5)
        pool = np.array([0.0, 0.25, np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1)), 0.75, 1.0,
                         np.nextafter(np.float32(1), np.float32(2)), 1.5], dtype=np.float32)
        return pool[g.randint(0, len(pool), (B, n))]
    raise ValueError(kind)


def probabilities(kind, B, n, g):
    if kind == "uniform":
        return g.rand(B, n).astype(np.float32)
    if kind == "constant":                                     # everything ties (within fg and within bg: 0.5 ties all)
        return np.full((B, n), [0.5, 0.3, 0.5][B % 3], dtype=np.float32)
    if kind == "eighths":
        return (g.randint(0, 9, (B, n)) / 8.0).astype(np.float32)
    if kind == "planted":                                      # exact 0, 1 and -0 among uniform values
        y = g.rand(B, n).astype(np.float32)
        y[g.rand(B, n) < 0.2] = 0.0
        y[g.rand(B, n) < 0.2] = 1.0
        y[g.rand(B, n) < 0.1] = -0.0                           # a background e of -0 ties with +0, by index
        return y
    raise ValueError(kind)
