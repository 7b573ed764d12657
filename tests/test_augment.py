"""CPU checks of the device augmentation (csrc/augment.hip, kernels.augment / flip_mean, punet.augment,
the prefetcher's plan, train._batches): the argument validation of the C-ABI without a device, the host
table checks, the spec parser, the plan's rows and who gets which, the prefetcher's plumbing on the CPU
device against the numpy reference, and the kernel set of the build."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import augment_ref as R

# stand-in pointers, far enough apart that no two buffers of the calls below overlap: validation never
# dereferences them
X, T, XO, TO, TAB = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000


def _train():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train
    return train


# ---- the C-ABI without a device
def test_augment_rejects_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the launch."""
    from punet import _lib
    lib = _lib.load()
    B, cx, ct, h, w, S = 3, 2, 1, 5, 7, 4

    def rejected(rc, word):
        assert rc == -1, rc
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_augment:") and word in msg, msg

    call = lib.pu_augment
    rejected(call(X, T, XO, TO, B, cx, ct, h, w, TAB, -1, None), b"max_shift -1 is negative")
    rejected(call(X, T, XO, TO, B, cx, ct, h, w, TAB, 5, None), b"max_shift 5 above")
    rejected(call(X, T, XO, TO, B, cx, ct, 7, 5, TAB, 5, None), b"max_shift 5 above")
    rejected(call(X, T, XO, TO, B, cx, ct, 1, 1, TAB, 1, None), b"max_shift 1 above")
    for bad in (0, -2, 65536):
        rejected(call(X, T, XO, TO, bad, cx, ct, h, w, TAB, S, None), b"batch")
    for bad in (0, -1):
        rejected(call(X, T, XO, TO, B, bad, ct, h, w, TAB, S, None), b"planes per slot")
        rejected(call(X, T, XO, TO, B, cx, ct, bad, w, TAB, 0, None), b"plane of")
        rejected(call(X, T, XO, TO, B, cx, ct, h, bad, TAB, 0, None), b"plane of")
    rejected(call(X, T, XO, TO, B, cx, -1, h, w, TAB, S, None), b"planes per slot")
    rejected(call(X, T, XO, TO, 1, 1, 1, 1 << 15, (1 << 15) + 1, TAB, S, None), b"pixels per plane")
    rejected(call(None, T, XO, TO, B, cx, ct, h, w, TAB, S, None), b"x is null")
    rejected(call(X, T, None, TO, B, cx, ct, h, w, TAB, S, None), b"x_out is null")
    rejected(call(X, T, XO, TO, B, cx, ct, h, w, None, S, None), b"table is null")
    rejected(call(X, None, XO, TO, B, cx, ct, h, w, TAB, S, None), b"t or t_out is null")
    rejected(call(X, T, XO, None, B, cx, ct, h, w, TAB, S, None), b"t or t_out is null")
    rejected(call(X + 2, T, XO, TO, B, cx, ct, h, w, TAB, S, None), b"4-byte aligned")
    # an output on an input: the same buffer, one word into it, its last word; image and mask crosswise
    xbytes, tbytes = B * cx * h * w * 4, B * ct * h * w * 4
    for xo, to in ((X, TO), (X + 4, TO), (X + xbytes - 4, TO), (X - xbytes + 4, TO), (T, TO), (XO, T), (XO, X),
                   (XO, T + tbytes - 4)):
        rejected(call(X, T, xo, to, B, cx, ct, h, w, TAB, S, None), b"aliases an input")
    rejected(call(X, T, XO, XO + xbytes - 4, B, cx, ct, h, w, TAB, S, None), b"x_out and t_out overlap")
    rejected(call(X, T, XO, TO, B, cx, ct, h, w, XO + 16, S, None), b"aliases the table")
    # with no mask planes the mask pointers are not looked at - the next check is what fails
    rejected(call(X, None, X, None, B, cx, 0, h, w, TAB, S, None), b"aliases an input")


def test_flip_mean_rejects_bad_arguments_without_a_device():
    from punet import _lib
    lib = _lib.load()
    B, h, w = 3, 5, 7
    nb = B * h * w * 4

    def rejected(rc, word):
        assert rc == -1, rc
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_flip_mean:") and word in msg, msg

    call = lib.pu_flip_mean
    for bad in (0, -1):
        rejected(call(X, T, XO, bad, h, w, None), b"batch")
        rejected(call(X, T, XO, B, bad, w, None), b"batch")
        rejected(call(X, T, XO, B, h, bad, None), b"batch")
    rejected(call(X, T, XO, 1 << 16, 1 << 15, 1, None), b"2^31 rows")
    rejected(call(None, T, XO, B, h, w, None), b"y is null")
    rejected(call(X, None, XO, B, h, w, None), b"y_mirror is null")
    rejected(call(X, T, None, B, h, w, None), b"out is null")
    rejected(call(X, T, XO + 1, B, h, w, None), b"4-byte aligned")
    for out in (T, T + 4, T + nb - 4, T - nb + 4):
        rejected(call(X, T, out, B, h, w, None), b"overlaps y_mirror")
    rejected(call(X, X, X, B, h, w, None), b"overlaps y_mirror")               # out == y is fine, y_mirror on it is not
    for out in (X + 4, X + nb - 4, X - 4):
        rejected(call(X, T, out, B, h, w, None), b"overlaps y without being y")


# ---- the wrappers
def test_wrappers_are_exported_and_refuse_cpu_images():
    from punet import kernels as K
    assert "augment" in K.__all__ and "flip_mean" in K.__all__
    x = torch.rand(2, 1, 5, 7)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.augment(x, x.clone(), np.zeros((2, 4), dtype=np.int32), 2)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.augment(x, None, torch.zeros(2, 4, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.flip_mean(x, x.clone())


@pytest.mark.parametrize("rows, word", [
    ([[2, 0, 0, 0], [0, 0, 0, 0]], "flip"), ([[-1, 0, 0, 0], [0, 0, 0, 0]], "flip"),
    ([[0, 3, 0, 0], [0, 0, 0, 0]], "shift"), ([[0, 0, 0, 0], [1, 0, -3, 0]], "shift"),
    ([[0, 0, 0, 0]], "table must be"), ([[0, 0, 0], [0, 0, 0]], "table must be"), ([0, 0, 0, 0], "table must be"),
    ([[0.0, 0, 0, 0], [0, 0, 0, 0]], "integers")])
def test_augment_rejects_bad_host_tables(rows, word):
    """before the images are looked at: the check of a host table needs no device"""
    from punet import kernels as K
    x = torch.rand(2, 1, 5, 7)
    for table in (np.array(rows), torch.tensor(rows)):
        with pytest.raises(ValueError, match=word):
            K.augment(x, None, table, 2)
    assert K.check_augment_table(np.array([[1, 2, -2, 0], [0, -2, 2, 0]], dtype=np.int64), 2, 2).dtype == np.int32
    with pytest.raises(ValueError, match="max_shift"):
        K.augment(x, None, np.zeros((2, 4), dtype=np.int32), 5)


# ---- the spec and the plan
def test_parse_augment():
    from punet.augment import AugmentSpec, parse_augment
    assert not parse_augment("") and not parse_augment(None) and not parse_augment(" , ")
    assert parse_augment("hflip") == AugmentSpec(True, 0)
    assert parse_augment("shift:8") == AugmentSpec(False, 8)
    assert parse_augment("hflip,shift:8") == parse_augment(" shift:8 , hflip ") == AugmentSpec(True, 8)
    assert parse_augment("hflip,shift:8", hw=(101, 9)).shift == 8
    assert not parse_augment("shift:0")
    for bad in ("vflip", "hflip,rot90", "shift", "shift:", "shift:-1", "shift:x", "shift8", "shifted:3", "hflip shift:2"):
        with pytest.raises(ValueError, match="augment"):
            parse_augment(bad)
    with pytest.raises(ValueError, match="above min"):
        parse_augment("shift:8", hw=(101, 8))
    with pytest.raises(ValueError, match="above min"):
        parse_augment("shift:1", hw=(1, 1))


def test_plan_rows():
    from punet.augment import AugmentPlan, mirror_table
    n = 500
    plan = AugmentPlan("hflip,shift:8", n, 3)
    a = plan.table(0)
    assert a.shape == (n, 4) and a.dtype == np.int32
    assert np.array_equal(a, AugmentPlan("hflip,shift:8", n, 3).table(0))             # the same (seed, epoch)
    assert not np.array_equal(a, plan.table(1)) and not np.array_equal(a, AugmentPlan("hflip,shift:8", n, 4).table(0))
    assert not np.array_equal(plan.table(1), AugmentPlan("hflip,shift:8", n, 4).table(0))    # (3, 1) is not (4, 0)
    for e in range(3):
        t = plan.table(e)
        assert set(np.unique(t[:, 0])) == {0, 1} and (t[:, 3] == 0).all()
        assert t[:, 1:3].min() == -8 and t[:, 1:3].max() == 8                            # both ends are drawn
    only_flip, only_shift = AugmentPlan("hflip", n, 3).table(0), AugmentPlan("shift:8", n, 3).table(0)
    assert (only_flip[:, 1:] == 0).all() and (only_shift[:, 0] == 0).all() and (only_shift[:, 3] == 0).all()
    # one order of draws whatever the spec: the flips and the shifts of a transform do not depend on the other
    assert np.array_equal(only_flip[:, 0], a[:, 0]) and np.array_equal(only_shift[:, 1:3], a[:, 1:3])
    # the documented draws
    rng = np.random.Generator(np.random.Philox(key=[3, 2]))
    flips, shifts = rng.integers(0, 2, n), rng.integers(-8, 9, (n, 2))
    assert np.array_equal(plan.table(2), np.column_stack([flips, shifts, np.zeros(n)]).astype(np.int32))
    assert not AugmentPlan("", n, 0).spec and (AugmentPlan("", n, 0).table(0) == 0).all()
    assert np.array_equal(mirror_table(3), [[1, 0, 0, 0]] * 3) and mirror_table(3).dtype == np.int32


def _samples(n=18, h=6, w=9, seed=5):
    return R.random_words((n, 1, h, w), seed), R.random_words((n, 1, h, w), seed + 1)


def _run_prefetcher(monkeypatch, Xs, Ys, ranges, plan, epochs, depth=2):
    """[(epoch, lo, hi, x, y)] of every yielded batch, copied out before the iterator advances, and the
    calls kernels.augment received"""
    from punet import kernels as K
    from punet.loader import BatchPrefetcher
    calls = []
    monkeypatch.setattr(K, "augment", R.numpy_augment(calls))
    pf = BatchPrefetcher(Xs, Ys, ranges, "cpu", depth=depth, augment=plan)
    got = []
    for e in range(epochs):
        pf.set_epoch(e)
        for (lo, hi), (x, y) in zip(ranges, pf):
            got.append((e, lo, hi, x.numpy().copy(), y.numpy().copy()))
    return got, calls


def test_every_rank_takes_the_single_process_rows(monkeypatch):
    """train._batches at world 1, 2 and 4: the rows a rank applies to the samples of its shard are rows
    lo .. hi of the epoch's table - the rows the single process applies to the same samples"""
    train = _train()
    from punet.augment import AugmentPlan
    n, bs = 37, 3
    Xs, Ys = _samples(n)
    plan = AugmentPlan("hflip,shift:3", n, 11)
    for epoch in (0, 1):
        table = plan.table(epoch)
        seen = {}
        for world in (1, 2, 4):
            rows_of = {}
            for rank in range(world):
                ranges = list(train._batches(n, bs, world, rank))
                from punet import kernels as K
                from punet.loader import BatchPrefetcher
                calls = []
                monkeypatch.setattr(K, "augment", R.numpy_augment(calls))
                pf = BatchPrefetcher(Xs, Ys, ranges, "cpu", augment=plan)
                pf.set_epoch(epoch)
                assert len(list(pf)) == len(ranges) == len(calls)
                for (lo, hi), (b, rows, S) in zip(ranges, calls):
                    assert b == hi - lo and S == 3
                    for i in range(lo, hi):
                        assert i not in rows_of                      # no sample on two ranks
                        rows_of[i] = tuple(rows[i - lo])
            assert rows_of == {i: tuple(table[i]) for i in rows_of}
            seen[world] = rows_of
        assert len(seen[1]) == n - n % bs and len(seen[2]) == n - n % (2 * bs) and len(seen[4]) == n - n % (4 * bs)


@pytest.mark.parametrize("ydims", [4, 3])
def test_prefetcher_yields_the_reference_on_the_cpu_device(monkeypatch, ydims):
    from punet.augment import AugmentPlan
    Xs, Ys = _samples(18)
    if ydims == 3:
        Ys = Ys[:, 0]
    ranges = [(0, 4), (4, 8), (8, 12), (12, 16), (16, 18)]                # 5 batches, the last one ragged
    plan = AugmentPlan("hflip,shift:5", 18, 2)
    got, calls = _run_prefetcher(monkeypatch, Xs, Ys, ranges, plan, epochs=2)
    assert len(got) == len(calls) == 10
    tables = [plan.table(0), plan.table(1)]
    assert not np.array_equal(*tables)
    for e, lo, hi, x, y in got:
        rows = tables[e][lo:hi]
        assert np.array_equal(R.bits(x), R.augment_batch(R.bits(Xs[lo:hi]), rows)), (e, lo)
        assert np.array_equal(R.bits(y), R.augment_batch(R.bits(Ys[lo:hi]), rows)), (e, lo)
    assert any(not np.array_equal(R.bits(x), R.bits(Xs[lo:hi])) for _, lo, hi, x, _ in got)


def test_prefetcher_without_a_plan_never_augments(monkeypatch):
    from punet.augment import AugmentPlan
    Xs, Ys = _samples(10)
    ranges = [(0, 4), (4, 8), (8, 10)]
    for plan in (None, AugmentPlan("", 10, 0)):
        got, calls = _run_prefetcher(monkeypatch, Xs, Ys, ranges, plan, epochs=2)
        assert calls == []
        for _, lo, hi, x, y in got:
            assert np.array_equal(R.bits(x), R.bits(Xs[lo:hi])) and np.array_equal(R.bits(y), R.bits(Ys[lo:hi]))


def test_prefetcher_refuses_a_plan_that_does_not_fit():
    from punet.augment import AugmentPlan
    from punet.loader import BatchPrefetcher
    Xs, Ys = _samples(10, h=6, w=9)
    with pytest.raises(ValueError, match="above min"):
        BatchPrefetcher(Xs, Ys, [(0, 4)], "cpu", augment=AugmentPlan("shift:6", 10, 0))
    with pytest.raises(ValueError, match="plan for 8 samples"):
        BatchPrefetcher(Xs, Ys, [(0, 4), (6, 10)], "cpu", augment=AugmentPlan("hflip", 8, 0))
    with pytest.raises(ValueError, match="same H x W"):
        BatchPrefetcher(Xs, Ys[:, :, :5], [(0, 4)], "cpu", augment=AugmentPlan("hflip", 10, 0))


# ---- test-time augmentation
class _Net:
    def eval(self):
        return self

    def parameters(self):
        return iter([torch.zeros(1)])

    def initialZeroHebb(self, B):
        return torch.zeros(B, 1)

    def __call__(self, x, hebb):
        return torch.sigmoid(8.0 * (x[:, 0] - 0.5)), hebb


def test_tta_modes(tmp_path):
    from punet.augment import tta_forward
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import eval as ev
    import infer
    x = torch.rand(3, 1, 5, 7)
    assert torch.equal(tta_forward(_Net(), x, None), _Net()(x, None)[0]) and torch.equal(tta_forward(_Net(), x), _Net()(x, None)[0])
    cpu = torch.device("cpu")
    Xn, Yn = x.numpy(), (x.numpy() > 0.5).astype(np.float32)
    params = {"device": cpu, "mask_threshold": 0.5, "out_dir": str(tmp_path)}
    for bad in ("vflip", "hflip,vflip", True, ""):
        for call in (lambda: tta_forward(_Net(), x, bad),
                     lambda: infer.predict_masks(_Net(), Xn, cpu, tta=bad),
                     lambda: infer.predict_rle(_Net(), Xn, cpu, 0.5, tta=bad),
                     lambda: infer.predict(_Net(), (["a", "b", "c"], Xn), params, tta=bad),
                     lambda: infer.predict(_Net(), (["a", "b", "c"], Xn), dict(params, tta=bad)),
                     lambda: infer.start_inference({}, (["a", "b", "c"], Xn), Xn, Yn, str(tmp_path), 7, 5, 1, tta=bad),
                     lambda: ev.eval_net(_Net(), Xn, Yn, cpu, metrics="host", tta=bad),
                     lambda: ev.iou_sweep(_Net(), Xn, Yn, cpu, [0.0], metrics="host", tta=bad),
                     lambda: ev.score_model_best_iou(_Net(), Xn, Yn, cpu, metrics="host", tta=bad)):
            with pytest.raises(ValueError, match="tta"):
                call()
    assert not os.path.exists(os.path.join(str(tmp_path), "submission.csv"))


def test_tta_hflip_plumbing_on_the_cpu(monkeypatch):
    """two forwards of the chunk's own batch size - the images, then their mirrors - merged by flip_mean"""
    from punet import kernels as K
    from punet.augment import tta_forward
    calls = []
    monkeypatch.setattr(K, "augment", R.numpy_augment(calls))
    monkeypatch.setattr(K, "flip_mean", lambda y, ym, out=None: torch.from_numpy(R.flip_mean(y.numpy(), ym.numpy())))
    seen = []

    class Net(_Net):
        def __call__(self, x, hebb):
            seen.append((x.clone(), hebb))
            return _Net.__call__(self, x, hebb)

    x = torch.rand(3, 1, 5, 7)
    y = tta_forward(Net(), x, "hflip")
    assert len(seen) == 2 and seen[0][1] is not seen[1][1]                 # a fresh zero trace each
    assert torch.equal(seen[0][0], x) and torch.equal(seen[1][0], x.flip(-1))
    assert len(calls) == 1 and calls[0][0] == 3 and calls[0][2] == 0 and np.array_equal(calls[0][1], [[1, 0, 0, 0]] * 3)
    plain = _Net()(x, None)[0].numpy()
    mirrored = _Net()(x.flip(-1), None)[0].numpy()
    assert np.array_equal(y.numpy(), R.flip_mean(plain, mirrored))


# ---- the build
def test_kernel_set_of_the_build():
    """augment.hip holds exactly its two kernels, free of scratch, spills and LDS"""
    import build_native
    from wgrad_matrix import demangle
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    mine = [sym for sym, k in d["kernels"].items() if k["source"] == "augment.hip"]
    assert sorted(demangle(s) for s in mine) == ["augment_kernel", "flip_mean_kernel"]
    for sym in mine:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, (sym, k)
    for name in ("augment_kernel", "flip_mean_kernel"):
        assert name in open(os.path.join(os.path.dirname(PKG), "DESIGN.md")).read()
