"""Fitting data to a net of another size on the MI355X (pu_fit: fit_move_kernel, fit_resize_kernel) against the
numpy reference of tests/fit_ref.py: pad and crop bit for bit on random words, the resize against float64 under
a counted bound; then what is built on it - the fitted prediction against torch's own reflect pad, flip-averaged
prediction merged at the data size, metrics and run-length rows from the device and the host, the prefetcher's
fitted slots, and training with --fit through both data paths and against host-padded arrays."""
import csv
import os

import numpy as np
import pytest
import torch

import augment_ref as R
import fit_ref as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
POISON = np.int32(0x5A5A5A5A)


def _words(shape, seed):
    """random 32-bit words as float32, none of them the poison the outputs are pre-filled with"""
    a = R.random_words(shape, seed)
    v = a.view(np.int32)
    v[v == POISON] ^= 1
    return a


def _poisoned(shape):
    return torch.full(shape, int(POISON), dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


# ---- pad and crop
@pytest.mark.parametrize("case", F.PAD_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])))
def test_pad_and_crop_move_the_reference_bits(gpu_device, case):
    from punet import kernels as K
    shape, (H, W), offsets = case
    h, w = shape[-2:]
    x = _words(shape, 1)
    big = _words(shape[:-2] + (H, W), 2)
    xd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(big).to(DEV)
    for top, left in offsets:
        po = _poisoned(big.shape)
        assert K.fit(xd, (H, W), "pad", top, left, out=po) is po
        assert np.array_equal(_bits(po), F.pad(R.bits(x), H, W, top, left)), (top, left)
        co = _poisoned(x.shape)
        assert K.fit(bd, (h, w), "crop", top, left, out=co) is co
        assert np.array_equal(_bits(co), F.crop(R.bits(big), h, w, top, left)), (top, left)
        # the crop undoes the pad, and without out a new tensor comes back
        back = K.fit(po, (h, w), "crop", top, left)
        assert back is not po and back.shape == xd.shape and np.array_equal(_bits(back), R.bits(x)), (top, left)
    assert np.array_equal(_bits(xd), R.bits(x)) and np.array_equal(_bits(bd), R.bits(big))          # the inputs untouched
    if H == W:
        assert np.array_equal(_bits(K.fit(xd, H, "pad", *offsets[0])), F.pad(R.bits(x), H, W, *offsets[0]))     # one side for a square


# ---- resize
# the pad shapes in both directions (128^2 -> 101^2, the data set's way back, among them), an index numerator above 2^31 (the 64-bit form of the
# coordinate) and a denominator above 2^24 (the weight from the fp64 quotient)
RESIZE_CASES = [(c[0], c[1]) for c in F.PAD_CASES] + [(c[0][:-2] + c[1], c[0][-2:]) for c in F.PAD_CASES] + \
    [((1, 1, 40000), (1, 33000)), ((1, 1, 3), (1, (1 << 23) + 5))]
assert ((2, 1, 128, 128), (101, 101)) in RESIZE_CASES


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])))
def test_resize_equals_the_float64_reference(gpu_device, case):
    """The bound is counted, not measured.  With u = 2^-24 and M = max|x|: fx and gx = 1.0f - fx are each within u
    of the exact weights (fx one rounding of the exact quotient; gx that error plus its own rounding, fx + gx <= 1);
    a lerp fmaf(b, fx, a * gx) then carries M u from gx, M u gx from the product's rounding, M u fx from fx and M u
    from the fma's: 3 M u.  The third lerp adds its own 3 M u to the 3 M u that top and bot bring in with weights
    summing to one: 6 M u in the first order - inside the 16 M u the bound allows for about ten roundings.  A
    half-pixel or off-by-one mistake is of the order 0.1 M."""
    from punet import kernels as K
    shape, (H, W) = case
    x = np.random.RandomState(sum(shape) + H).rand(*shape).astype(np.float32)
    want = F.resize(x, H, W)
    xd = torch.from_numpy(x).to(DEV)
    out = _poisoned(shape[:-2] + (H, W))
    assert K.fit(xd, (H, W), "resize", out=out) is out
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    cap = 16 * 2.0 ** -24 * float(np.abs(x).max())
    print("resize %s -> %s: max error %.3g, cap %.3g" % (shape, (H, W), err, cap))
    assert np.isfinite(got).all() and err <= cap, (err, cap)
    again = K.fit(xd, (H, W), "resize")
    assert again is not out and np.array_equal(_bits(again), _bits(out))                     # the same bits on every call
    assert np.array_equal(xd.cpu().numpy(), x)


def test_resize_reads_zeros_outside_and_never_a_neighbouring_plane(gpu_device):
    """planes of NaN around the one resized: a read past the plane's rows would bring one in; the frame of an
    upsized plane of ones is 0.75 and 0.5625 (one and two neighbours outside), exactly"""
    from punet import kernels as K
    x = torch.full((3, 3, 3), float("nan"), device=DEV)
    x[1] = 1.0
    up = K.fit(x, 6, "resize")[1].cpu().numpy()
    assert np.array_equal(up[1:-1, 1:-1], np.ones((4, 4), dtype=np.float32))
    assert np.array_equal(up[0, 1:-1], np.full(4, 0.75, dtype=np.float32)) and up[0, 0] == up[-1, -1] == np.float32(0.5625)


def test_wrapper_checks_shapes_outputs_and_ranges(gpu_device):
    from punet import kernels as K
    x = torch.rand(2, 1, 5, 7, device=DEV)
    with pytest.raises(ValueError, match="out must be"):
        K.fit(x, (8, 12), "pad", 1, 2, out=torch.empty(2, 1, 8, 11, device=DEV))
    with pytest.raises(ValueError, match="pad rows"):
        K.fit(x, (8, 12), "pad", 4, 2)
    with pytest.raises(ValueError, match="leaves the plane"):
        K.fit(x, (3, 3), "crop", 3, 0)
    with pytest.raises(RuntimeError, match="out must be torch.float32"):
        K.fit(x, (8, 12), "pad", 1, 2, out=torch.empty(2, 1, 8, 12, device=DEV, dtype=torch.float64))
    buf = torch.zeros(70 + 192, device=DEV)
    xin = buf[:70].view(2, 1, 5, 7)
    for at in (0, 69, 36):
        if at + 192 <= buf.numel():
            with pytest.raises(RuntimeError, match="pu_fit: out overlaps in"):
                K.fit(xin, (8, 12), "pad", 1, 2, out=buf[at:at + 192].view(2, 1, 8, 12))
    assert K.fit(xin, (8, 12), "pad", 1, 2, out=buf[70:].view(2, 1, 8, 12)).shape == (2, 1, 8, 12)        # adjacent is fine


# ---- prediction
SIDE, DATA = 32, 27


def _small_net():
    from unet import UNetp
    torch.manual_seed(4)
    return UNetp(1, 1, DEV, rule="oja", nbf=SIDE, depth=4, base_ch=16)


@pytest.fixture(scope="module", params=["unetp", "unetpres"])
def fit_case(request):
    from unet import UNetpRes
    from punet.fit import parse_fit
    import infer
    if request.param == "unetp":
        net = _small_net()
    else:
        torch.manual_seed(5)
        net = UNetpRes(1, 1, DEV, neurons=4, nbf=SIDE)
    net.eval()
    X = np.random.RandomState(21).rand(5, 1, DATA, DATA).astype(np.float32)
    Xm = np.ascontiguousarray(X[..., ::-1])
    spec = parse_fit("pad", (DATA, DATA), SIDE)
    return {"net": net, "X": X, "Xm": Xm, "spec": spec, "plain": infer.predict_masks(net, X, DEV, fit=spec),
            "plain_m": infer.predict_masks(net, Xm, DEV, fit=spec), "tta": infer.predict_masks(net, X, DEV, tta="hflip", fit=spec)}


def test_fitted_prediction_is_the_crop_of_the_net_on_torchs_reflect_pad(gpu_device, fit_case):
    from punet.augment import tta_forward
    c = fit_case
    s = c["spec"]
    x = torch.from_numpy(c["X"]).to(DEV)
    with torch.no_grad():
        got = tta_forward(c["net"], x, None, s)
        padded = torch.nn.functional.pad(x, (s.left, SIDE - DATA - s.left, s.top, SIDE - DATA - s.top), mode="reflect")
        full, _ = c["net"](padded, c["net"].initialZeroHebb(len(x)))
    want = full[..., s.top:s.top + DATA, s.left:s.left + DATA]
    assert got.shape == (5, DATA, DATA) and full.shape == (5, SIDE, SIDE)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert np.array_equal(R.bits(c["plain"]), _bits(got))
    # resized: the same kernel up and back around the same forward
    from punet import kernels as K
    from punet.fit import parse_fit
    r = parse_fit("resize", (DATA, DATA), SIDE)
    with torch.no_grad():
        got_r = tta_forward(c["net"], x, None, r)
        full_r, _ = c["net"](K.fit(x, SIDE, "resize"), c["net"].initialZeroHebb(len(x)))
    assert torch.equal(got_r.view(torch.int32), K.fit(full_r.contiguous(), DATA, "resize").view(torch.int32))
    assert got_r.shape == got.shape and not torch.equal(got_r, got)


def test_fitted_tta_is_the_merge_of_two_fitted_predictions_at_the_data_size(gpu_device, fit_case):
    c = fit_case
    assert c["tta"].shape == c["plain"].shape == (5, DATA, DATA) and c["tta"].dtype == np.float32
    assert np.array_equal(R.bits(c["tta"]), R.bits(R.flip_mean(c["plain"], c["plain_m"])))
    assert not np.array_equal(c["tta"], c["plain"])


@pytest.mark.parametrize("tta", [None, "hflip"])
def test_fitted_metrics_are_the_same_from_the_device_and_the_host(gpu_device, fit_case, tta):
    import eval as ev
    from utils import iou_metric_batch
    c = fit_case
    preds = c["plain"] if tta is None else c["tta"]
    Y = (np.random.RandomState(2).rand(*c["X"].shape) > 0.5).astype(np.float32)
    ths = [float(np.quantile(preds, q)) for q in (0.1, 0.5, 0.9)]
    dev = ev.iou_sweep(c["net"], c["X"], Y, DEV, ths, metrics="device", tta=tta, fit=c["spec"])
    host = ev.iou_sweep(c["net"], c["X"], Y, DEV, ths, metrics="host", tta=tta, fit=c["spec"])
    assert dev.tobytes() == host.tobytes()
    at_data = preds.reshape(len(Y), 1, 1, DATA, DATA)
    assert host.tobytes() == np.array([iou_metric_batch(Y, at_data > np.float64(th)) for th in ths]).tobytes()
    a = ev.eval_net(c["net"], c["X"], Y, DEV, batch=3, tta=tta, fit=c["spec"])
    b = ev.eval_net(c["net"], c["X"], Y, DEV, batch=3, metrics="host", tta=tta, fit=c["spec"])
    assert a == b and np.isfinite(a).all()
    # the accuracy is the share of agreeing pixels among the 27 x 27 of the data, not among the net's 32 x 32
    import infer
    chunked = infer.predict_masks(c["net"], c["X"], DEV, batch=3, tta=tta, fit=c["spec"])
    agree = np.mean([np.mean((p > 0.5) == (t[0] > 0.5)) for p, t in zip(chunked, Y)])
    assert abs(a[0] - agree) < 1e-6


def test_fitted_rows_are_the_same_from_the_device_and_the_host_encoding(gpu_device, fit_case, tmp_path):
    import infer
    from utils import encode
    c = fit_case
    ids = ["id%d" % i for i in range(len(c["X"]))]
    thr = float(np.quantile(c["plain"], 0.5))
    rows = {}
    for rle in ("device", "host"):
        out = str(tmp_path / rle)
        os.makedirs(out)
        params = {"device": DEV, "mask_threshold": thr, "out_dir": out}
        # the spec through the keyword on one path and through params on the other: the same thing
        rows[rle] = infer.predict(c["net"], (ids, c["X"]), dict(params, fit=c["spec"]), rle=rle) if rle == "host" else \
            infer.predict(c["net"], (ids, c["X"]), params, rle=rle, fit=c["spec"])
        with open(os.path.join(out, "submission.csv")) as f:
            assert [tuple(r) for r in list(csv.reader(f))[1:]] == rows[rle]
    assert rows["device"] == rows["host"] == [(i, encode(np.round(m > thr))) for i, m in zip(ids, c["plain"])]
    runs = 0
    for _, code in rows["device"]:
        v = [int(t) for t in code.split()]
        assert len(v) % 2 == 0
        for start, length in zip(v[::2], v[1::2]):                          # 1-based starts, column-major in 27 x 27
            assert 1 <= start and length >= 1 and start + length - 1 <= DATA * DATA, (start, length)
            runs += 1
    assert runs > 0


# ---- loading
def test_prefetcher_yields_fitted_batches_on_the_device(gpu_device):
    """depth 2, 5 batches with a ragged last one, 2 epochs, with and without a plan: the fitted pair is what is
    yielded, padded from the batch's own augmented rows"""
    from punet.augment import AugmentPlan
    from punet.fit import parse_fit
    from punet.loader import BatchPrefetcher
    n, h, S = 18, 37, 64
    Xs, Ys = _words((n, 1, h, h), 3), _words((n, h, h), 4)
    ranges = [(0, 4), (4, 8), (8, 12), (12, 16), (16, 18)]
    spec = parse_fit("pad", (h, h), S)
    for plan in (None, AugmentPlan("hflip,shift:9", n, 6)):
        pf = BatchPrefetcher(Xs, Ys, ranges, DEV, depth=2, augment=plan, fit=spec)
        for e in range(2):
            pf.set_epoch(e)
            seen = 0
            for (lo, hi), (x, y) in zip(ranges, pf):
                assert x.shape == (hi - lo, 1, S, S) and y.shape == (hi - lo, S, S) and x.device == DEV
                xa, ya = R.bits(Xs[lo:hi]), R.bits(Ys[lo:hi])
                if plan is not None:
                    xa, ya = R.augment_batch(xa, plan.table(e)[lo:hi]), R.augment_batch(ya, plan.table(e)[lo:hi])
                assert np.array_equal(_bits(x), F.pad(xa, S, S, spec.top, spec.left)), (e, lo)
                assert np.array_equal(_bits(y), F.pad(ya, S, S, spec.top, spec.left)), (e, lo)
                seen += 1
            assert seen == 5


# ---- training
STEPS = 4           # whole batches of 4 among 18 samples: the steps of an epoch


def _train_losses(tmp, X, Y, prefetch, fit=None, augment=None, seed=None):
    import train
    net = _small_net()
    params = {"out_dir": tmp, "device": DEV, "epochs": 1, "stop_time": -1, "lr": 3e-4, "val_every": 100,
              "save_every": 100, "rollout": 50000, "gamma": 0.666, "steplr": 4, "debug": False, "batch_size": 4,
              "prefetch": prefetch}
    if fit is not None:
        params.update(fit=fit, net_size=SIDE)
    if augment is not None:
        params.update(augment=augment, augment_seed=seed)
    losses = train.train(net, X, X[:2], Y, Y[:2], params)[0]
    return losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope="module")
def training_runs(tmp_path_factory):
    """18 samples of 27 x 27 in batches of 4 on the small net at side 32, one epoch; each run computed once"""
    from punet.augment import AugmentPlan
    tmp = str(tmp_path_factory.mktemp("fit"))
    g = np.random.RandomState(9)
    X = g.rand(18, 1, DATA, DATA).astype(np.float32)
    Y = (g.rand(18, 1, DATA, DATA) > 0.5).astype(np.float32)
    top, left = F.centre(DATA, DATA, SIDE, SIDE)
    aug, seed = "hflip,shift:4", 13
    rows = AugmentPlan(aug, 18, seed).table(0)
    assert rows[:, 0].any() and rows[:, 1:3].any()
    frame = [(0, 0), (0, 0), (top, SIDE - DATA - top), (left, SIDE - DATA - left)]
    return {"streamed": _train_losses(tmp, X, Y, True, "pad"),
            "resident": _train_losses(tmp, X, Y, False, "pad"),
            "host-padded": _train_losses(tmp, F.pad(X, SIDE, SIDE, top, left), F.pad(Y, SIDE, SIDE, top, left), True),
            "streamed augmented": _train_losses(tmp, X, Y, True, "pad", aug, seed),
            "resident augmented": _train_losses(tmp, X, Y, False, "pad", aug, seed),
            "host-augmented-and-padded": _train_losses(tmp, F.pad(R.augment_batch(X, rows), SIDE, SIDE, top, left),
                                                       F.pad(R.augment_batch(Y, rows), SIDE, SIDE, top, left), True),
            "framed by zeros": _train_losses(tmp, np.pad(X, frame), np.pad(Y, frame), True),
            "streamed resized": _train_losses(tmp, X, Y, True, "resize"),
            "resident resized": _train_losses(tmp, X, Y, False, "resize")}


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_padded_training_is_the_same_streamed_resident_and_on_host_padded_arrays(gpu_device, training_runs):
    a = training_runs["streamed"]
    assert len(a[0]) == STEPS and all(np.isfinite(a[0]))
    assert _same(a, training_runs["resident"])
    assert _same(a, training_runs["host-padded"])


def test_padded_training_follows_the_augmentation_at_the_data_size(gpu_device, training_runs):
    a = training_runs["streamed augmented"]
    assert len(a[0]) == STEPS and _same(a, training_runs["resident augmented"])
    assert _same(a, training_runs["host-augmented-and-padded"])
    assert all(p != q for p, q in zip(a[0], training_runs["streamed"][0]))


def test_padded_training_differs_from_training_on_a_frame_of_zeros(gpu_device, training_runs):
    """the same 27 x 27 samples at the same place in 32 x 32 planes, nothing around them: what the net sees when
    the borders are not reflected - the flag is not a no-op"""
    other = training_runs["framed by zeros"]
    assert len(other[0]) == STEPS and all(np.isfinite(other[0]))
    assert all(p != q for p, q in zip(training_runs["streamed"][0], other[0]))


def test_resized_training_is_the_same_streamed_and_resident(gpu_device, training_runs):
    a = training_runs["streamed resized"]
    assert len(a[0]) == STEPS and all(np.isfinite(a[0])) and _same(a, training_runs["resident resized"])
    assert all(p != q for p, q in zip(a[0], training_runs["streamed"][0]))


def test_resize_refuses_a_lovasz_loss_and_fit_needs_the_net_size(gpu_device, tmp_path):
    import train
    X = np.zeros((4, 1, DATA, DATA), dtype=np.float32)
    params = {"out_dir": str(tmp_path), "device": DEV, "epochs": 1, "stop_time": -1, "lr": 3e-4, "val_every": 100,
              "save_every": 100, "rollout": 50000, "gamma": 0.666, "steplr": 4, "debug": False, "batch_size": 4}
    for loss in ("lovasz", "bce+lovasz"):
        with pytest.raises(ValueError, match="not binary"):
            train.train(_small_net(), X, X[:2], X, X[:2], dict(params, fit="resize", net_size=SIDE, loss=loss))
    with pytest.raises(ValueError, match="net-size"):
        train.train(_small_net(), X, X[:2], X, X[:2], dict(params, fit="pad"))
