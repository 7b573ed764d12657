"""CPU checks of the device run-length encoding (csrc/rle.hip, kernels.rle_encode, punet.rle,
infer.predict / predict_rle): the workspace formula and the argument validation of the C-ABI without a
device, the compare value against NumPy's own comparisons, the strings against utils.encode and the
reference's recorded strings, the kernel set of the build, and the plumbing of predict."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden
import rle_ref as R

A = 0x10000          # 16-byte aligned stand-in pointer: validation never dereferences it


def _infer():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import infer
    return infer


# ---- the C-ABI without a device
REJECTED_SHAPES = ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, 8, -3),
                   (1, 1 << 15, (1 << 15) + 1),         # h w > 2^30
                   (4, 1 << 15, 1 << 15),               # batch ceil(n / 2) = 2^31
                   (65535, 257, 1 << 8))                # the same through the batch


def test_workspace_formula():
    from punet import _lib
    ws = _lib.load().pu_rle_encode_workspace_bytes
    for h, w in ((1, 1), (64, 3), (65, 3), (101, 101), (1024, 1024), (3, 64), (3, 65)):
        for batch in (1, 3, 32):
            assert ws(batch, h, w) == batch * w * -(-h // 64) * 8 + batch * 4
    assert ws(3, 1 << 15, 1 << 15) == 3 * (1 << 15) * (1 << 9) * 8 + 12       # the largest image, 3 of them
    assert ws(65535, 1, 1) == 65535 * 12
    assert ws(65535, 1 << 8, 1 << 8) > 0                                      # 2^31 - 2^15 pairs at the most
    for bad in REJECTED_SHAPES:
        assert ws(*bad) == 0, bad


def test_rle_encode_rejects_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the first launch."""
    from punet import _lib
    lib = _lib.load()
    B, h, w = 3, 70, 9
    nb = lib.pu_rle_encode_workspace_bytes(B, h, w)
    cap = B * ((h * w + 1) // 2)

    def rejected(rc, word, code=-1):
        assert rc == code, rc
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_rle_encode:") and word in msg, msg

    call = lib.pu_rle_encode
    rejected(call(None, B, h, w, 0.5, A, A, cap, A, nb, None), b"y is null")
    rejected(call(A, B, h, w, 0.5, None, A, cap, A, nb, None), b"offsets is null")
    rejected(call(A, B, h, w, 0.5, A, None, cap, A, nb, None), b"runs is null")
    rejected(call(A, B, h, w, 0.5, A, A, cap, None, nb, None), b"workspace is null")
    for bad in (0, -2, 65536):
        rejected(call(A, bad, h, w, 0.5, A, A, cap, A, 1 << 40, None), b"batch")
    for bad in (0, -1):
        rejected(call(A, B, bad, w, 0.5, A, A, cap, A, nb, None), b"image of")
        rejected(call(A, B, h, bad, 0.5, A, A, cap, A, nb, None), b"image of")
    rejected(call(A, 1, 1 << 15, (1 << 15) + 1, 0.5, A, A, cap, A, 1 << 40, None), b"pixels per image")
    rejected(call(A, 4, 1 << 15, 1 << 15, 0.5, A, A, cap, A, 1 << 40, None), b"2^31 pairs")
    rejected(call(A, 65535, 257, 1 << 8, 0.5, A, A, cap, A, 1 << 40, None), b"2^31 pairs")
    for bad in (float("nan"), float("inf"), float("-inf")):
        rejected(call(A, B, h, w, bad, A, A, cap, A, nb, None), b"threshold is not finite")
    for bad in (-1, -(1 << 40)):
        rejected(call(A, B, h, w, 0.5, A, A, bad, A, nb, None), b"cap")
    rejected(call(A, B, h, w, 0.5, A, A, cap, A + 4, nb, None), b"8-byte aligned")
    rejected(call(A, B, h, w, 0.5, A, A, cap, A, nb - 1, None), b"workspace", code=-4)
    rejected(call(A, B, h, w, 0.5, A, A, cap, A, 0, None), b"workspace", code=-4)
    # no room asked for: a null runs is fine - the next check is what fails
    rejected(call(A, B, h, w, 0.5, A, None, 0, A + 4, nb, None), b"8-byte aligned")


def test_wrapper_is_exported_and_checks_its_tensors():
    from punet import kernels as K
    assert "rle_encode" in K.__all__
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.rle_encode(torch.rand(2, 8, 8), 0.5)


# ---- the compare value
@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7, -0.8472978603872037, 1e-3])
def test_compare_value_gives_numpys_own_comparison(thr):
    from punet.rle import compare_value
    f = np.float32(thr)
    y = np.array([np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf)),
                  np.nan, np.inf, -np.inf, 0.0, 1.0], dtype=np.float32)
    for given in (float(thr), np.float32(thr), np.float64(thr)):
        cv = compare_value(given)
        assert type(cv) is float
        assert np.array_equal(y.astype(np.float64) > cv, y > given), (given, type(given))
        # ... and the entry's bound on the compare value is the same comparison once more
        assert np.array_equal(y >= R.bound_above(cv), y > given)
    # the two kinds do differ on float32(thr) itself whenever thr is no fp32 number
    if np.float64(f) != thr:
        assert compare_value(float(thr)) == compare_value(np.float32(thr)) == float(f) != compare_value(np.float64(thr))
    else:
        assert compare_value(float(thr)) == compare_value(np.float64(thr)) == thr
    assert compare_value(1) == 1.0 and compare_value(np.array(thr)) == thr


# ---- the strings
def test_rle_strings_equal_encode_and_the_reference_fixture():
    from punet.rle import rle_strings
    from utils import encode
    g = golden("metrics.npz")                                    # the reference's own strings
    offsets, runs = R.table_of(g["masks"].astype(np.float32), 0.5)
    assert rle_strings(offsets, runs) == [str(r) for r in g["rles"]]
    g = golden("iou_batch.npz")                                  # the fixture tests/test_host.py scores
    preds = g["preds"].reshape(-1, 24, 24)
    for th in g["thresholds"][[0, 15, 30]]:
        offsets, runs = R.table_of(preds, th)
        assert rle_strings(offsets, runs) == [encode(np.round(m > th)) for m in preds]
    masks = np.stack(list(R.planted_masks(5, 3).values())).astype(np.float32)
    got = rle_strings(*R.table_of(masks, 0.5))
    assert got == [encode(m) for m in masks]
    assert got[0] == "" and got[1] == "1 15" and got[2] == "1 1 3 1 5 1 7 1 9 1 11 1 13 1 15 1"
    assert got[3] == "1 1 5 2 10 2 15 1"                          # rows 0 and 4: the runs cross the columns
    # spare rows past the total are not read
    assert rle_strings(offsets, np.concatenate([runs, np.full((3, 2), -7, dtype=np.int32)])) == rle_strings(offsets, runs)


def test_run_table_fetches_the_pairs_in_use():
    from punet.rle import RunTable
    offsets, runs = R.table_of(np.stack(list(R.planted_masks(5, 3).values())).astype(np.float32), 0.5)
    spare = np.concatenate([runs, np.full((4, 2), -7, dtype=np.int32)])
    tab = RunTable(torch.from_numpy(offsets), torch.from_numpy(spare))
    o, r = tab.fetch()
    assert np.array_equal(o, offsets) and np.array_equal(r, runs)
    with pytest.raises(ValueError):
        RunTable(torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32))


# ---- the build
def test_kernel_set_of_the_build():
    """rle.hip holds exactly its three kernels, free of scratch and spills"""
    import build_native
    from wgrad_matrix import demangle
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    mine = [sym for sym, k in d["kernels"].items() if k["source"] == "rle.hip"]
    assert sorted(demangle(s) for s in mine) == ["rle_bits_kernel", "rle_count_kernel", "rle_emit_kernel"]
    for sym in mine:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (sym, k)
    for name in ("rle_bits_kernel", "rle_count_kernel", "rle_emit_kernel"):
        assert name in open(os.path.join(os.path.dirname(PKG), "DESIGN.md")).read()


# ---- predict
class _Net:
    """a stand-in model on the CPU: probabilities from the image, the trace ignored"""

    def __init__(self):
        self.batches = []

    def eval(self):
        return self

    def parameters(self):
        return iter([torch.zeros(1)])

    def initialZeroHebb(self, B):
        return torch.zeros(B, 1)

    def __call__(self, x, hebb):
        self.batches.append(x.shape[0])
        return torch.sigmoid(8.0 * (x[:, 0] - 0.5)), hebb


def _images(n=70, h=9, w=7):
    X = np.random.RandomState(11).rand(n, 1, h, w).astype(np.float32)
    X[1], X[2] = 0.0, 1.0                        # an empty and a full mask among them
    return ["id%d" % i for i in range(n)], X


@pytest.mark.parametrize("thr", [0.5, np.float64(0.43), np.float32(0.6)])
def test_predict_paths_give_the_same_rows_and_file(monkeypatch, tmp_path, thr):
    infer = _infer()
    from punet import kernels as K
    from punet.rle import compare_value
    calls = []
    monkeypatch.setattr(K, "rle_encode", R.numpy_rle_encode(calls))
    ids, X = _images()
    cpu = torch.device("cpu")
    host_dir, dev_dir = str(tmp_path / "host"), str(tmp_path / "device")
    os.makedirs(host_dir), os.makedirs(dev_dir)
    host = infer.predict(_Net(), (ids, X), {"device": cpu, "mask_threshold": thr, "out_dir": host_dir}, rle="host")
    assert calls == []                                           # the host path never reaches the kernel
    assert host[1] == ("id1", "") and host[2] == ("id2", "1 63")

    def no_encode(im):
        raise AssertionError("utils.encode on the device path")
    monkeypatch.setattr(infer, "encode", no_encode)
    net = _Net()
    dev = infer.predict(net, (ids, X), {"device": cpu, "mask_threshold": thr, "out_dir": dev_dir})      # the default
    assert dev == host
    assert net.batches == [32, 32, 6] and calls == [(32, compare_value(thr)), (32, compare_value(thr)), (6, compare_value(thr))]
    with open(os.path.join(host_dir, "submission.csv"), "rb") as f, open(os.path.join(dev_dir, "submission.csv"), "rb") as g:
        assert f.read() == g.read()
    with open(os.path.join(dev_dir, "submission.csv")) as f:
        got = list(csv.reader(f))
    assert got[0] == ["id", "rle_mask"] and [tuple(r) for r in got[1:]] == dev
    assert infer.predict_rle(_Net(), X, cpu, thr, batch=7) == [r for _, r in host]
    assert infer.predict_rle(_Net(), X[:0], cpu, thr) == []


def test_predict_rle_hands_the_maps_back_when_asked(monkeypatch):
    infer = _infer()
    from punet import kernels as K
    monkeypatch.setattr(K, "rle_encode", R.numpy_rle_encode([]))
    _, X = _images(9)
    kept = []
    infer.predict_rle(_Net(), X, torch.device("cpu"), 0.5, batch=4, keep=kept)
    assert [k.shape[0] for k in kept] == [4, 4, 1]
    assert np.array_equal(np.concatenate(kept, 0), infer.predict_masks(_Net(), X, torch.device("cpu"), batch=4))


def test_entry_points_reject_an_unknown_rle_path(tmp_path):
    infer = _infer()
    ids, X = _images(3)
    params = {"device": torch.device("cpu"), "mask_threshold": 0.5, "out_dir": str(tmp_path)}
    for bad in ("gpu", None, "Device"):
        with pytest.raises(ValueError, match="rle"):
            infer.predict(_Net(), (ids, X), params, rle=bad)
        with pytest.raises(ValueError, match="rle"):
            infer.start_inference({}, (ids, X), X, X, str(tmp_path), 7, 9, 1, rle=bad)
    assert not os.path.exists(os.path.join(str(tmp_path), "submission.csv"))
