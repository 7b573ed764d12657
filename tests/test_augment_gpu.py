"""The device augmentation on the MI355X (pu_augment: augment_kernel; pu_flip_mean: flip_mean_kernel)
against the numpy reference of tests/augment_ref.py, bit for bit: the kernels on the smallest shapes with a
single pixel, maximal reflection on both sides, rows that are not 16-byte aligned, an aligned width, a null
mask, widths above 64 and above 256 lanes and a height above one block; the prefetcher's augmented slots;
training with --augment through both data paths and against host-augmented arrays; flip-averaged
prediction through infer and eval."""
import csv
import os

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
POISON = np.int32(0x5A5A5A5A)


def _words(shape, seed):
    """random 32-bit words as float32, none of them the poison the outputs are pre-filled with"""
    a = R.random_words(shape, seed)
    v = a.view(np.int32)
    v[v == POISON] ^= 1
    return a


SHAPES = [(3, 1, 1, 5, 7), (2, 1, 1, 1, 1), (2, 2, 1, 2, 3), (2, 1, 1, 101, 101), (2, 1, 1, 128, 128), (2, 1, 0, 64, 200),
          (1, 1, 1, 300, 65)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_augment_kernel_moves_the_reference_bits(gpu_device, shape):
    from punet import kernels as K
    B, cx, ct, h, w = shape
    x = _words((B, cx, h, w), 1)
    t = _words((B, ct, h, w), 2) if ct else None
    xd = torch.from_numpy(x).to(DEV)
    td = torch.from_numpy(t).to(DEV) if ct else None
    top = min(h, w) - 1
    for S in sorted({top, 0, 8} - ({8} if 8 > top else set())):
        rows = R.grid_rows(S)
        rows = np.concatenate([rows, rows[: -len(rows) % B]])             # whole batches
        for at in range(0, len(rows), B):
            chunk = rows[at:at + B]
            xo = torch.full(xd.shape, int(POISON), dtype=torch.int32, device=DEV).view(torch.float32)
            to = torch.full(td.shape, int(POISON), dtype=torch.int32, device=DEV).view(torch.float32) if ct else None
            # host tables are checked and uploaded; every other batch goes up as a device table, used as it is
            table = torch.from_numpy(chunk).to(DEV) if (at // B) % 2 else chunk
            got = K.augment(xd, td, table, S, out=(xo, to))
            assert got[0] is xo and got[1] is to
            assert np.array_equal(xo.view(torch.int32).cpu().numpy(), R.augment_batch(R.bits(x), chunk)), (S, chunk)
            if ct:
                assert np.array_equal(to.view(torch.int32).cpu().numpy(), R.augment_batch(R.bits(t), chunk)), (S, chunk)
    # without out: new tensors, and None for the mask that was not given
    xo, to = K.augment(xd, td, np.zeros((B, 4), dtype=np.int32), 0)
    assert torch.equal(xo.view(torch.int32), xd.view(torch.int32)) and (to is None) == (ct == 0)


def test_augment_wrapper_checks_device_tables_and_outputs(gpu_device):
    from punet import kernels as K
    x = torch.rand(2, 1, 5, 7, device=DEV)
    with pytest.raises(ValueError, match="table must be"):
        K.augment(x, None, torch.zeros(3, 4, dtype=torch.int32, device=DEV), 2)
    with pytest.raises(RuntimeError, match="table must be torch.int32"):
        K.augment(x, None, torch.zeros(2, 4, dtype=torch.int64, device=DEV), 2)
    with pytest.raises(ValueError, match="out must be"):
        K.augment(x, None, np.zeros((2, 4), dtype=np.int32), 2, out=(torch.empty(2, 1, 5, 6, device=DEV), None))
    with pytest.raises(RuntimeError, match="pu_augment: an output aliases an input"):
        K.augment(x, None, np.zeros((2, 4), dtype=np.int32), 2, out=(x, None))


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 5, 7), (2, 101, 101), (2, 128, 128), (1, 3, 300)], ids=lambda s: "x".join(map(str, s)))
def test_flip_mean_equals_the_float32_reference(gpu_device, shape):
    from punet import kernels as K
    g = np.random.RandomState(sum(shape))
    y, m = g.rand(*shape).astype(np.float32), g.rand(*shape).astype(np.float32)
    for a in (y, m):                                                    # exact zeros and ones among them
        a.flat[:: 5] = np.where(g.rand(a.flat[:: 5].size) < 0.5, 0.0, 1.0)
    want = R.flip_mean(y, m)
    yd, md = torch.from_numpy(y).to(DEV), torch.from_numpy(m).to(DEV)
    out = K.flip_mean(yd, md)
    assert out is not yd and np.array_equal(R.bits(out.cpu().numpy()), R.bits(want))
    assert np.array_equal(yd.cpu().numpy(), y)                          # the inputs untouched
    poisoned = torch.full(yd.shape, float("nan"), device=DEV)
    assert K.flip_mean(yd, md, out=poisoned) is poisoned and np.array_equal(R.bits(poisoned.cpu().numpy()), R.bits(want))
    assert K.flip_mean(yd, md, out=yd) is yd                            # in place on y
    assert np.array_equal(R.bits(yd.cpu().numpy()), R.bits(want)) and np.array_equal(md.cpu().numpy(), m)
    with pytest.raises(RuntimeError, match="pu_flip_mean: out overlaps y_mirror"):
        K.flip_mean(yd, md, out=md)


def test_prefetcher_yields_the_reference_on_the_device(gpu_device):
    """depth 2, 5 batches with a ragged last one, 2 epochs: a slot overwritten before the compute stream is
    done with it, or augmented by another batch's rows, shows in the copy taken before advancing"""
    from punet.augment import AugmentPlan
    from punet.loader import BatchPrefetcher
    n, h, w = 18, 37, 70
    Xs, Ys = _words((n, 1, h, w), 3), _words((n, 1, h, w), 4)
    ranges = [(0, 4), (4, 8), (8, 12), (12, 16), (16, 18)]
    plan = AugmentPlan("hflip,shift:9", n, 6)
    pf = BatchPrefetcher(Xs, Ys, ranges, DEV, depth=2, augment=plan)
    for e in range(2):
        pf.set_epoch(e)
        table = plan.table(e)
        seen = 0
        for (lo, hi), (x, y) in zip(ranges, pf):
            assert x.shape == (hi - lo, 1, h, w) and x.device == DEV
            xc, yc = x.view(torch.int32).cpu().numpy(), y.view(torch.int32).cpu().numpy()
            assert np.array_equal(xc, R.augment_batch(R.bits(Xs[lo:hi]), table[lo:hi])), (e, lo)
            assert np.array_equal(yc, R.augment_batch(R.bits(Ys[lo:hi]), table[lo:hi])), (e, lo)
            seen += 1
        assert seen == 5


# ---- training
STEPS = 4           # whole batches of 4 among 18 samples: the steps of an epoch


def _small_net():
    from unet import UNetp
    torch.manual_seed(4)
    return UNetp(1, 1, DEV, rule="oja", nbf=32, depth=4, base_ch=16)


def _train_losses(tmp, X, Y, epochs, prefetch, augment=None, seed=None):
    import train
    net = _small_net()
    params = {"out_dir": tmp, "device": DEV, "epochs": epochs, "stop_time": -1, "lr": 3e-4, "val_every": 100,
              "save_every": 100, "rollout": 50000, "gamma": 0.666, "steplr": 4, "debug": False, "batch_size": 4,
              "prefetch": prefetch}
    if augment is not None:
        params.update(augment=augment, augment_seed=seed)
    losses = train.train(net, X, X[:2], Y, Y[:2], params)[0]
    return losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope="module")
def training_runs(tmp_path_factory):
    """18 samples of 32 x 32 in batches of 4 (train._batches keeps the 4 whole ones of an epoch), the small net of
    tests/test_entry_gpu.py::test_streamed_batches_train_identically_to_resident; each run computed once"""
    from punet.augment import AugmentPlan
    tmp = str(tmp_path_factory.mktemp("augment"))
    g = np.random.RandomState(9)
    X = g.rand(18, 1, 32, 32).astype(np.float32)
    Y = (g.rand(18, 1, 32, 32) > 0.5).astype(np.float32)
    spec, seed = "hflip,shift:4", 13
    rows = AugmentPlan(spec, 18, seed).table(0)
    assert rows[:, 0].any() and rows[:, 1:3].any()
    Xa, Ya = R.augment_batch(X, rows), R.augment_batch(Y, rows)
    return {"streamed 2": _train_losses(tmp, X, Y, 2, True, spec, seed),
            "resident 2": _train_losses(tmp, X, Y, 2, False, spec, seed),
            "streamed 1": _train_losses(tmp, X, Y, 1, True, spec, seed),
            "host-augmented 1": _train_losses(tmp, Xa, Ya, 1, True),
            "plain 1": _train_losses(tmp, X, Y, 1, True)}


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_augmented_training_is_the_same_streamed_and_resident(gpu_device, training_runs):
    a, b = training_runs["streamed 2"], training_runs["resident 2"]
    assert len(a[0]) == 2 * STEPS and a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert a[0][:STEPS] == training_runs["streamed 1"][0] and a[0][STEPS:] != a[0][:STEPS]       # the second epoch has other rows


def test_augmented_training_equals_training_on_host_augmented_arrays(gpu_device, training_runs):
    want = training_runs["host-augmented 1"]
    assert len(want[0]) == STEPS
    assert _same(training_runs["streamed 1"], want)


def test_augmented_training_differs_from_plain_training(gpu_device, training_runs):
    plain = training_runs["plain 1"]
    assert len(plain[0]) == STEPS and all(np.isfinite(plain[0]))
    assert all(a != p for a, p in zip(training_runs["streamed 1"][0], plain[0]))


# ---- test-time augmentation
@pytest.fixture(scope="module", params=["unetp", "unetpres"])
def tta_case(request):
    from unet import UNetpRes
    import infer
    g = np.random.RandomState(21)
    if request.param == "unetp":
        net, side = _small_net(), 32
    else:
        torch.manual_seed(5)
        net, side = UNetpRes(1, 1, DEV, neurons=4, nbf=101), 101
    net.eval()
    X = g.rand(5, 1, side, side).astype(np.float32)
    Xm = np.ascontiguousarray(X[..., ::-1])
    plain, plain_m = infer.predict_masks(net, X, DEV), infer.predict_masks(net, Xm, DEV)
    return {"net": net, "X": X, "Xm": Xm, "plain": plain, "plain_m": plain_m,
            "tta": infer.predict_masks(net, X, DEV, tta="hflip")}


def test_tta_prediction_is_the_merge_of_the_two_plain_ones(gpu_device, tta_case):
    c = tta_case
    assert c["tta"].shape == c["plain"].shape and c["tta"].dtype == np.float32
    assert np.array_equal(R.bits(c["tta"]), R.bits(R.flip_mean(c["plain"], c["plain_m"])))
    assert not np.array_equal(c["tta"], c["plain"])
    # in chunks of 3 and 2: each forward at the chunk's own batch size, the merge per chunk
    import infer
    chunked = infer.predict_masks(c["net"], c["X"], DEV, batch=3, tta="hflip")
    want = R.flip_mean(infer.predict_masks(c["net"], c["X"], DEV, batch=3), infer.predict_masks(c["net"], c["Xm"], DEV, batch=3))
    assert np.array_equal(R.bits(chunked), R.bits(want))


def test_tta_prediction_of_the_mirror_is_the_mirror_of_the_prediction(gpu_device, tta_case):
    import infer
    c = tta_case
    mirrored = infer.predict_masks(c["net"], c["Xm"], DEV, tta="hflip")
    assert np.array_equal(R.bits(mirrored), R.bits(c["tta"][..., ::-1]))


def test_tta_rows_are_the_same_from_the_device_and_the_host_encoding(gpu_device, tta_case, tmp_path):
    import infer
    from utils import encode
    c = tta_case
    ids = ["id%d" % i for i in range(len(c["X"]))]
    thr = 0.5
    rows = {}
    for rle in ("device", "host"):
        out = str(tmp_path / rle)
        os.makedirs(out)
        params = {"device": DEV, "mask_threshold": thr, "out_dir": out}
        # the mode through the keyword on one path and through params on the other: the same thing
        rows[rle] = infer.predict(c["net"], (ids, c["X"]), dict(params, tta="hflip"), rle=rle) if rle == "host" else \
            infer.predict(c["net"], (ids, c["X"]), params, rle=rle, tta="hflip")
        with open(os.path.join(out, "submission.csv")) as f:
            assert [tuple(r) for r in list(csv.reader(f))[1:]] == rows[rle]
    assert rows["device"] == rows["host"] == [(i, encode(np.round(m > thr))) for i, m in zip(ids, c["tta"])]
    assert rows["device"] != [(i, encode(np.round(m > thr))) for i, m in zip(ids, c["plain"])]


def test_tta_sweep_is_the_same_from_the_device_and_the_host_metrics(gpu_device, tta_case):
    import eval as ev
    c = tta_case
    Y = (np.random.RandomState(2).rand(*c["X"].shape) > 0.5).astype(np.float32)
    ths = [float(np.quantile(c["tta"], q)) for q in (0.1, 0.5, 0.9)]
    dev = ev.iou_sweep(c["net"], c["X"], Y, DEV, ths, metrics="device", tta="hflip")
    host = ev.iou_sweep(c["net"], c["X"], Y, DEV, ths, metrics="host", tta="hflip")
    assert dev.tobytes() == host.tobytes()
    preds = c["tta"].reshape(len(Y), 1, 1, *c["tta"].shape[-2:])
    from utils import iou_metric_batch
    assert host.tobytes() == np.array([iou_metric_batch(Y, preds > np.float64(th)) for th in ths]).tobytes()
    assert ev.eval_net(c["net"], c["X"], Y, DEV, batch=3, tta="hflip") == ev.eval_net(c["net"], c["X"], Y, DEV, batch=3,
                                                                                   metrics="host", tta="hflip")
