"""CPU checks of fitting data to a net of another size (csrc/fit.hip, kernels.fit, punet.fit, the prefetcher's
fitted slots, train / infer plumbing): the argument validation of the C-ABI without a device, the wrapper's range
checks, the spec and its offsets, the numpy reference against itself, the plumbing of the prediction and loading
paths on CPU tensors, and the kernel set of the build."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
import fit_ref as F

# stand-in pointers far apart: validation never dereferences them
IN, OUT = 0x100000, 0x900000
PAD, CROP, RESIZE = 0, 1, 2


def _pkg():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)


# ---- the C-ABI without a device
def test_header_declares_pu_fit_and_the_binding_has_it():
    from punet import _lib
    src = open(os.path.join(ROOT, "include", "plastic_unet.h")).read()
    assert "int pu_fit(const float* in, float* out, long long planes, int h, int w, int H, int W, int mode, int top, int left," in src
    assert "enum { PU_FIT_PAD = 0, PU_FIT_CROP = 1, PU_FIT_RESIZE = 2 };" in src
    assert "pu_fit" in {n for n, _, _ in _lib.SIGNATURES} and _lib.load().pu_fit is not None


def test_pu_fit_rejects_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the launch."""
    from punet import _lib
    lib = _lib.load()
    call = lib.pu_fit

    def rejected(rc, word):
        assert rc == -1, rc
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_fit:") and word in msg, msg

    P, h, w, H, W = 3, 5, 7, 8, 12
    for bad in (-1, 3, 7):
        rejected(call(IN, OUT, P, h, w, H, W, bad, 0, 0, None), b"mode")
    for bad in (0, -2, 1 << 40):
        rejected(call(IN, OUT, bad, h, w, H, W, PAD, 1, 2, None), b"planes")
    for bad in (0, -1):
        rejected(call(IN, OUT, P, bad, w, H, W, RESIZE, 0, 0, None), b"planes of")
        rejected(call(IN, OUT, P, h, bad, H, W, RESIZE, 0, 0, None), b"planes of")
        rejected(call(IN, OUT, P, h, w, bad, W, RESIZE, 0, 0, None), b"planes of")
        rejected(call(IN, OUT, P, h, w, H, bad, RESIZE, 0, 0, None), b"planes of")
    rejected(call(IN, 1 << 40, 1, 1 << 15, (1 << 15) + 1, 4, 4, RESIZE, 0, 0, None), b"pixels per plane")
    rejected(call(IN, 1 << 40, 1, 4, 4, 1 << 15, (1 << 15) + 1, RESIZE, 0, 0, None), b"pixels per plane")
    # pad: a smaller target, and each of top, bottom, left, right out of 0 .. n - 1
    rejected(call(IN, OUT, P, h, w, 4, W, PAD, 0, 2, None), b"to a smaller")
    rejected(call(IN, OUT, P, h, w, H, 6, PAD, 1, 0, None), b"to a smaller")
    rejected(call(IN, OUT, P, h, w, H, W, PAD, -1, 2, None), b"pad rows")
    rejected(call(IN, OUT, P, h, w, H, W, PAD, 4, 2, None), b"pad rows")            # bottom -1
    rejected(call(IN, OUT, P, h, w, 10, W, PAD, 5, 2, None), b"pad rows")           # top 5 > h - 1
    rejected(call(IN, OUT, P, h, w, 10, W, PAD, 0, 2, None), b"pad rows")           # bottom 5 > h - 1
    rejected(call(IN, OUT, P, h, w, H, W, PAD, 1, -1, None), b"pad columns")
    rejected(call(IN, OUT, P, h, w, H, W, PAD, 1, 6, None), b"pad columns")         # right -1
    rejected(call(IN, OUT, P, h, w, H, 14, PAD, 1, 7, None), b"pad columns")        # left 7 > w - 1
    rejected(call(IN, OUT, P, h, w, H, 14, PAD, 1, 0, None), b"pad columns")        # right 7 > w - 1
    rejected(call(IN, OUT, P, 1, 1, 2, 1, PAD, 0, 0, None), b"pad rows")            # a single pixel reflects nowhere
    # crop: a larger target, a window that leaves the plane
    rejected(call(IN, OUT, P, H, W, h, W + 1, CROP, 0, 0, None), b"to a larger")
    rejected(call(IN, OUT, P, H, W, H + 1, w, CROP, 0, 0, None), b"to a larger")
    for top, left in ((-1, 0), (0, -1), (4, 0), (0, 6)):
        rejected(call(IN, OUT, P, H, W, h, w, CROP, top, left, None), b"leaves the plane")
    # resize: no offsets
    rejected(call(IN, OUT, P, h, w, H, W, RESIZE, 1, 0, None), b"top = left = 0")
    rejected(call(IN, OUT, P, h, w, H, W, RESIZE, 0, -1, None), b"top = left = 0")
    # pointers
    rejected(call(None, OUT, P, h, w, H, W, PAD, 1, 2, None), b"in is null")
    rejected(call(IN, None, P, h, w, H, W, PAD, 1, 2, None), b"out is null")
    rejected(call(IN + 2, OUT, P, h, w, H, W, PAD, 1, 2, None), b"4-byte aligned")
    rejected(call(IN, OUT + 1, P, h, w, H, W, PAD, 1, 2, None), b"4-byte aligned")
    ib, ob = P * h * w * 4, P * H * W * 4
    for out in (IN, IN + 4, IN + ib - 4, IN - ob + 4):
        for mode, top, left in ((PAD, 1, 2), (RESIZE, 0, 0)):
            rejected(call(IN, out, P, h, w, H, W, mode, top, left, None), b"out overlaps in")
    rejected(call(IN, IN + 4, P, H, W, h, w, CROP, 1, 2, None), b"out overlaps in")
    # a plane too tall for one grid
    rejected(call(IN, 1 << 40, 1, 4, 4, 1 << 29, 1, RESIZE, 0, 0, None), b"2^24 blocks")


# ---- the wrapper
def test_wrapper_is_exported_checks_ranges_and_refuses_cpu_planes():
    from punet import kernels as K
    assert "fit" in K.__all__
    x = torch.rand(2, 1, 5, 7)
    for args, word in [(((8, 12), "mirror"), "mode must be"), (((4, 12), "pad", 0, 2), "to a smaller"),
                       (((8, 12), "pad", 4, 2), "pad rows"), (((8, 12), "pad", -1, 2), "pad rows"),
                       (((8, 12), "pad", 1, 6), "pad columns"), (((8, 14), "pad", 1, 0), "pad columns"),
                       (((6, 7), "crop"), "to a larger"), (((3, 3), "crop", 3, 0), "leaves the plane"),
                       (((3, 3), "crop", 0, 5), "leaves the plane"), (((8, 12), "resize", 1, 0), "top = left = 0"),
                       (((0, 12), "resize"), "pixels each")]:
        with pytest.raises(ValueError, match=word):
            K.fit(x, *args)
    with pytest.raises(ValueError, match=r"\[\.\.\., h, w\]"):
        K.fit(torch.rand(5), 8, "resize")
    with pytest.raises(ValueError, match="no empty axis"):
        K.fit(torch.rand(0, 5, 7), 8, "resize")
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.fit(x, (8, 12), "pad", 1, 2)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.fit(x, 9, "resize")


# ---- the spec
def test_parse_fit_and_the_offsets():
    from punet.fit import FitSpec, parse_fit
    for off in ("", None, "  "):
        assert not parse_fit(off) and not parse_fit(off, (101, 101), 128) and parse_fit(off) == FitSpec()
    s = parse_fit("pad", (101, 101), 128)
    assert s and s == FitSpec("pad", (101, 101), 128) and parse_fit(s) is s
    assert (s.mode, s.h, s.w, s.side, s.top, s.left) == ("pad", 101, 101, 128, 13, 13)
    assert (s.top, s.left) == F.centre(101, 101, 128, 128)
    assert parse_fit("pad", (27, 27), 32).top == 2 and parse_fit(" resize ", (27, 27), 32).left == 2
    assert parse_fit("pad", (27, 27), 32) != parse_fit("resize", (27, 27), 32)
    assert parse_fit("pad", (101, 101), 201).top == 50 and parse_fit("pad", (101, 101), 101).top == 0
    assert parse_fit("resize", (101, 101), 512).side == 512               # no upper bound on a resize
    for text, hw, side, word in [("pad", (101, 101), 100, "below the data"), ("resize", (101, 101), 64, "below the data"),
                                 ("pad", (101, 101), 202, "above 2 min"), ("pad", (1, 1), 2, "above 2 min"),
                                 ("pad", (101, 99), 128, "square"), ("resize", (99, 101), 128, "square"),
                                 ("reflect", (101, 101), 128, "mode must be"), ("pad,resize", (101, 101), 128, "mode must be"),
                                 ("pad", (101, 101), None, "net-size"), ("pad", None, 128, "the data's"),
                                 ("pad", (0, 0), 128, "square")]:
        with pytest.raises(ValueError, match=word):
            parse_fit(text, hw, side)
    with pytest.raises(ValueError, match="empty spec"):
        FitSpec().to_net(torch.rand(1, 3, 3))
    with pytest.raises(ValueError, match="to_net takes"):
        s.to_net(torch.rand(2, 1, 128, 128))
    with pytest.raises(ValueError, match="to_data takes"):
        s.to_data(torch.rand(2, 101, 101))


def test_spec_calls_the_kernel_with_its_offsets(monkeypatch):
    from punet import kernels as K
    from punet.fit import parse_fit
    calls = []
    monkeypatch.setattr(K, "fit", lambda x, size, mode, top=0, left=0, out=None: calls.append((tuple(x.shape), size, mode, top, left, out)))
    pad, res = parse_fit("pad", (27, 27), 32), parse_fit("resize", (27, 27), 32)
    x, y = torch.rand(2, 1, 27, 27), torch.rand(2, 32, 32)
    pad.to_net(x); pad.to_data(y); res.to_net(x); res.to_data(y, out=x)
    assert calls == [((2, 1, 27, 27), 32, "pad", 2, 2, None), ((2, 32, 32), (27, 27), "crop", 2, 2, None),
                     ((2, 1, 27, 27), 32, "resize", 0, 0, None), ((2, 32, 32), (27, 27), "resize", 0, 0, x)]


# ---- the reference
def test_reference_pad_crop_and_resize():
    """the numpy reference against hand-made planes, and the crop undoing the pad"""
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert np.array_equal(F.pad(a, 3, 5, 1, 1), [[4, 3, 4, 5, 4], [1, 0, 1, 2, 1], [4, 3, 4, 5, 4]])
    for shape, (H, W), offsets in F.PAD_CASES:
        x = F.random_words(shape, 1)
        for top, left in offsets:
            p = F.pad(F.bits(x), H, W, top, left)
            assert p.shape == shape[:-2] + (H, W)
            assert np.array_equal(F.crop(p, shape[-2], shape[-1], top, left), F.bits(x))
    # a resize to the same size is the identity; a constant plane upsized by 2 keeps its value inside and halves
    # it on the frame, where one of the two neighbours is the zero outside
    b = np.random.RandomState(0).rand(4, 5)
    assert np.allclose(F.resize(b, 4, 5), b, rtol=0, atol=1e-15)
    up = F.resize(np.ones((1, 3, 3)), 6, 6)[0]
    assert np.allclose(up[1:-1, 1:-1], 1.0) and np.allclose(up[0, 1:-1], 0.75) and np.allclose(up[0, 0], 0.5625)


def _numpy_fit(calls):
    """kernels.fit on CPU tensors, for the host-side plumbing"""
    def fit(x, size, mode, top=0, left=0, out=None):
        H, W = (size, size) if np.ndim(size) == 0 else size
        calls.append((tuple(x.shape), (H, W), mode, top, left))
        a = x.numpy()
        if mode == "pad":
            r = F.pad(F.bits(a), H, W, top, left).view(np.float32)
        elif mode == "crop":
            r = F.crop(F.bits(a), H, W, top, left).view(np.float32)
        else:
            r = F.resize(a, H, W).astype(np.float32)
        r = torch.from_numpy(r)
        if out is not None:
            out.copy_(r)
            return out
        return r
    return fit


# ---- prediction
class _Net:
    """side 8: the 'prediction' is a function of the pixel and of its position, so a wrong crop shows"""
    ramp = torch.linspace(0.0, 0.3, 64).reshape(8, 8)

    def eval(self):
        return self

    def parameters(self):
        return iter([torch.zeros(1)])

    def initialZeroHebb(self, B):
        return torch.zeros(B, 1)

    def __call__(self, x, hebb):
        assert x.shape[-2:] == (8, 8), x.shape
        return torch.sigmoid(8.0 * (x[:, 0] - 0.5)) * 0.7 + self.ramp, hebb


def test_prediction_paths_fit_and_come_back_on_the_cpu(monkeypatch, tmp_path):
    _pkg()
    import augment_ref as R
    import eval as ev
    import infer
    from punet import kernels as K
    from punet.augment import tta_forward
    from punet.fit import parse_fit
    from utils import encode
    calls = []
    monkeypatch.setattr(K, "fit", _numpy_fit(calls))
    monkeypatch.setattr(K, "augment", R.numpy_augment([]))
    monkeypatch.setattr(K, "flip_mean", lambda y, ym, out=None: torch.from_numpy(R.flip_mean(y.numpy(), ym.numpy())))
    spec = parse_fit("pad", (5, 5), 8)
    x = torch.rand(3, 1, 5, 5)

    def plain(v):
        padded = torch.from_numpy(np.pad(v.numpy(), [(0, 0), (0, 0), (1, 2), (1, 2)], mode="reflect"))
        return _Net()(padded, None)[0][:, 1:6, 1:6]

    y = tta_forward(_Net(), x, None, spec)
    assert y.shape == (3, 5, 5) and torch.equal(y, plain(x))
    assert [c[2] for c in calls] == ["pad", "crop"] and calls[0][3:] == (1, 1) and calls[1][3:] == (1, 1)
    yt = tta_forward(_Net(), x, "hflip", spec)
    assert np.array_equal(yt.numpy(), R.flip_mean(plain(x).numpy(), plain(x.flip(-1)).numpy()))       # merged at 5 x 5
    assert not torch.equal(yt, y)
    # a false spec and None are today's path: the net sees the batch as it is
    x8 = torch.rand(2, 1, 8, 8)
    assert torch.equal(tta_forward(_Net(), x8, None, parse_fit("")), _Net()(x8, None)[0])
    cpu = torch.device("cpu")
    Xn, Yn = x.numpy(), (x.numpy() > 0.5).astype(np.float32)
    masks = infer.predict_masks(_Net(), Xn, cpu, batch=2, fit=spec)
    assert masks.shape == (3, 5, 5) and np.array_equal(masks, y.numpy())
    rows = infer.predict(_Net(), (["a", "b", "c"], Xn), {"device": cpu, "mask_threshold": 0.5, "out_dir": str(tmp_path), "fit": spec},
                         rle="host")
    assert rows == [(i, encode(np.round(m > 0.5))) for i, m in zip("abc", y.numpy())]
    acc, loss = ev.eval_net(_Net(), Xn, Yn, cpu, criterion=torch.nn.BCELoss(), metrics="host", fit=spec)
    want = float(np.mean([np.mean((m > 0.5) == (t[0] > 0.5)) for m, t in zip(y.numpy(), Yn)]))
    assert abs(acc - want) < 1e-6 and np.isfinite(loss)
    sweep = ev.iou_sweep(_Net(), Xn, Yn, cpu, [0.4, 0.6], metrics="host", fit=spec)
    assert sweep.shape == (2,)
    with pytest.raises(ValueError, match="a spec for 5 x 5 data"):
        infer.start_inference({}, (["a"], Xn[:1]), Xn, Yn, str(tmp_path), 7, 7, 1, fit=spec)


# ---- loading and training
def test_prefetcher_fits_after_the_augmentation_on_the_cpu_device(monkeypatch):
    """K.fit has no CPU form (the product has no fallback), so the fitted slots are checked with a numpy stand-in
    for it: the plumbing - which pair is fitted, which is yielded - is what runs here; the kernel runs in
    tests/test_fit_gpu.py"""
    import augment_ref as R
    from punet import kernels as K
    from punet.augment import AugmentPlan
    from punet.fit import parse_fit
    from punet.loader import BatchPrefetcher
    calls = []
    monkeypatch.setattr(K, "fit", _numpy_fit(calls))
    monkeypatch.setattr(K, "augment", R.numpy_augment([]))
    n, h = 10, 6
    Xs, Ys = R.random_words((n, 1, h, h), 5), R.random_words((n, h, h), 6)
    ranges = [(0, 4), (4, 8), (8, 10)]
    spec = parse_fit("pad", (h, h), 9)
    for plan in (None, AugmentPlan("hflip,shift:3", n, 2)):
        pf = BatchPrefetcher(Xs, Ys, ranges, "cpu", augment=plan, fit=spec)
        for e in range(2):
            pf.set_epoch(e)
            seen = 0
            for (lo, hi), (x, y) in zip(ranges, pf):
                xa, ya = R.bits(Xs[lo:hi]), R.bits(Ys[lo:hi])
                if plan is not None:
                    rows = plan.table(e)[lo:hi]
                    xa, ya = R.augment_batch(xa, rows), R.augment_batch(ya, rows)
                assert x.shape == (hi - lo, 1, 9, 9) and y.shape == (hi - lo, 9, 9)
                assert np.array_equal(R.bits(x.numpy()), F.pad(xa, 9, 9, 1, 1)), (e, lo)
                assert np.array_equal(R.bits(y.numpy()), F.pad(ya, 9, 9, 1, 1)), (e, lo)
                seen += 1
            assert seen == 3
    assert len(calls) == 2 * 2 * 3 * 2 and {c[2] for c in calls} == {"pad"}
    # without a fit the kernel is never reached
    calls.clear()
    assert len(list(BatchPrefetcher(Xs, Ys, ranges, "cpu", fit=parse_fit("")))) == 3 and calls == []
    with pytest.raises(ValueError, match="must end in the spec's"):
        BatchPrefetcher(Xs, Ys, ranges, "cpu", fit=parse_fit("pad", (7, 7), 9))


def test_train_flags_and_refusals():
    _pkg()
    import train
    a = train.parse_args(["--fit", "pad", "--net-size", "128", "--model-type", "unetp"])
    assert (a.fit, a.net_size, a.img_size) == ("pad", 128, 101)
    d = train.parse_args([])
    assert (d.fit, d.net_size) == ("", None)
    X = np.zeros((4, 1, 27, 27), dtype=np.float32)
    with pytest.raises(ValueError, match="go together"):
        train.start_train(X, X, X, X, "out", "m", 27, 27, 1, fit="pad")
    with pytest.raises(ValueError, match="go together"):
        train.start_train(X, X, X, X, "out", "m", 27, 27, 1, net_size=32)


# ---- the build
def test_kernel_set_of_the_build():
    """fit.hip holds exactly its kernels, free of scratch, spills and LDS"""
    _pkg()
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    mine = [sym for sym, k in d["kernels"].items() if k["source"] == "fit.hip"]
    names = sorted(re.match(r"_ZN2pu\d+([a-z_]+_kernel)", s).group(1) for s in mine)       # fit_resize_kernel<int>, <long long>
    assert names == ["fit_move_kernel", "fit_resize_kernel", "fit_resize_kernel"]
    for sym in mine:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, (sym, k)
    for name in ("fit_move_kernel", "fit_resize_kernel"):
        assert name in open(os.path.join(ROOT, "DESIGN.md")).read()
