"""CPU checks of the device validation metrics (csrc/metrics.hip, kernels.seg_metrics, punet.metrics,
eval.eval_net / iou_sweep): argument validation and the workspace formula of the C-ABI without a
device, the score from counts against the reference fixture, the dealing of chunks to ranks, the
kernel sets of the build, and the host path left as it was."""
import ctypes
import json
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden

A = 0x10000          # 16-byte aligned stand-in pointer: validation never dereferences it
LOGIT_TH = np.log(np.linspace(0.3, 0.7, 31) / (1 - np.linspace(0.3, 0.7, 31)))


def _th(values):
    return (ctypes.c_double * max(len(values), 1))(*values)


def _ev():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import eval as ev
    return ev


# ---- the C-ABI without a device
def test_workspace_formula():
    from punet import _lib
    ws = _lib.load().pu_seg_metrics_workspace_bytes
    for n in (1, 255, 256, 257, 101 * 101, 512 * 256, 512 * 256 + 257, 1 << 33):
        blocks = min(512, -(-n // 256))
        for batch in (1, 3, 32):
            for T in (0, 1, 31, 32):
                got = ws(batch, n, T)
                assert got == batch * blocks * (8 + 4 * (2 + 2 * T)) and got > 0 and got % 8 == 0
        assert ws(1, n, 0) < ws(2, n, 0) < ws(3, n, 0)                    # monotone in batch
        assert all(ws(2, n, T) < ws(2, n, T + 1) for T in range(32))      # and in n_thr
    for bad in ((0, 10, 0), (-1, 10, 0), (1, 0, 0), (1, -5, 0), (1, 10, -1), (1, 10, 33)):
        assert ws(*bad) == 0


def test_seg_metrics_rejects_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the first launch."""
    from punet import _lib
    lib = _lib.load()
    B, n, T = 3, 1000, 4
    th = _th([-0.5, 0.0, 0.25, 2.0])
    nb = lib.pu_seg_metrics_workspace_bytes(B, n, T)

    def rejected(rc, word, code=-1):
        assert rc == code, rc
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_seg_metrics:") and word in msg, msg

    call = lib.pu_seg_metrics
    rejected(call(None, A, B, n, th, T, A, A, A, nb, None), b"y or t")
    rejected(call(A, None, B, n, th, T, A, A, A, nb, None), b"y or t")
    rejected(call(A, A, B, n, th, T, None, A, A, nb, None), b"loss or counts")
    rejected(call(A, A, B, n, th, T, A, None, A, nb, None), b"loss or counts")
    for bad in (0, -2):
        rejected(call(A, A, bad, n, th, T, A, A, A, nb, None), b"batch")
        rejected(call(A, A, B, bad, th, T, A, A, A, nb, None), b"n ")
    for bad in (-1, 33):
        rejected(call(A, A, B, n, th, bad, A, A, A, 1 << 30, None), b"n_thr")
    rejected(call(A, A, B, n, None, T, A, A, A, nb, None), b"thresholds is null")
    for bad in ([0.0, 0.0, 1.0, 2.0], [0.0, 1.0, 0.5, 2.0], [3.0, 2.0, 1.0, 0.0]):
        rejected(call(A, A, B, n, _th(bad), T, A, A, A, nb, None), b"is not above")
    for bad in (float("nan"), float("inf"), float("-inf")):
        rejected(call(A, A, B, n, _th([-1.0, 0.0, bad, 2.0]), T, A, A, A, nb, None), b"thresholds[2] is not finite")
    rejected(call(A, A, B, n, th, T, A, A, None, nb, None), b"workspace", code=-4)
    rejected(call(A, A, B, n, th, T, A, A, A, nb - 1, None), b"workspace", code=-4)
    rejected(call(A, A, B, n, th, T, A, A, A + 4, nb, None), b"8-byte aligned")
    # no thresholds: a null list is fine, the smaller workspace is enough - the next check is what fails
    nb0 = lib.pu_seg_metrics_workspace_bytes(B, n, 0)
    rejected(call(A, A, B, n, None, 0, A, A, A + 4, nb0, None), b"8-byte aligned")


def test_wrapper_is_exported_and_checks_its_tensors():
    from punet import kernels as K
    assert "seg_metrics" in K.__all__
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.seg_metrics(torch.rand(2, 8), torch.rand(2, 8))


# ---- the score from counts
def _counts(y_true, pred):
    from utils.iou_metric import _foreground
    n = y_true.shape[0]
    t, p = _foreground(y_true.reshape(n, -1)), np.asarray(pred).reshape(n, -1)
    return np.logical_and(t, p).sum(axis=1), t.sum(axis=1), p.sum(axis=1)


def test_score_from_counts_equals_the_reference_fixture():
    """counts taken in numpy from the fixture of tests/test_host.py (empty truth, empty prediction and
    a full truth among its samples) -> the reference's scores, bitwise; iou_metric_batch, which now
    calls the same function, still gives them too"""
    from utils import iou_metric_batch, iou_score_from_counts
    g = golden("iou_batch.npz")
    empty = 0
    for th, want in zip(g["thresholds"], g["ious"]):
        inter, tsum, psum = _counts(g["y_valid"], g["preds"] > th)
        empty += int(((tsum == 0) & (psum == 0)).sum())
        got = iou_score_from_counts(inter, tsum, psum)
        assert got.dtype == np.float32 and got.shape == ()
        assert got.tobytes() == np.asarray(want).tobytes()
        assert iou_metric_batch(g["y_valid"], g["preds"] > th).tobytes() == np.asarray(want).tobytes()
    assert empty > 0
    # the counts are not modified, whatever their type
    inter = np.array([0, 3], dtype=np.int64)
    iou_score_from_counts(inter, np.array([0, 4]), np.array([0, 5]))
    assert inter.tolist() == [0, 3]
    # two empty masks score 1; IoU 4 / 6 passes the thresholds 0.5, 0.55, 0.6 and 0.65 of the ten
    assert iou_score_from_counts([0, 4], [0, 5], [0, 5]) == np.float32((1.0 + 0.4) / 2)


# ---- chunks to ranks
@pytest.mark.parametrize("n,batch,world", [(5, 2, 2), (5, 2, 1), (0, 4, 2), (7, 7, 3), (8, 7, 3), (800, 32, 8), (3, 1, 5)])
def test_chunks_for_rank_deals_every_chunk_once(n, batch, world):
    from punet.metrics import chunks_for_rank
    whole = [(s, min(n, s + batch)) for s in range(0, n, batch)]
    shards = [chunks_for_rank(n, batch, world, r) for r in range(world)]
    assert sorted(c for sh in shards for c in sh) == whole                     # disjoint and complete
    for r, sh in enumerate(shards):
        assert sh == whole[r::world]                                          # chunk i on rank i % world
    assert chunks_for_rank(n, batch) == whole == chunks_for_rank(n, batch, 1, 0)


def test_chunks_for_rank_ragged_tail_and_arguments():
    from punet.metrics import chunks_for_rank
    assert chunks_for_rank(5, 2, 2, 0) == [(0, 2), (4, 5)]        # chunks 0 and 2, the last one ragged
    assert chunks_for_rank(5, 2, 2, 1) == [(2, 4)]                # chunk 1
    for bad in ((5, 0, 1, 0), (5, 2, 0, 0), (5, 2, 2, 2), (5, 2, 2, -1), (-1, 2, 1, 0)):
        with pytest.raises(ValueError):
            chunks_for_rank(*bad)


def test_metric_table_keeps_bits_in_one_table():
    """the loss bits (NaN and a set sign bit among them) and the counts through the int64 table"""
    from punet.metrics import MetricTable
    loss = torch.tensor([0.25, float("nan"), -0.0, 3.5e-39, 100.0], dtype=torch.float32)
    loss[1] = torch.tensor([-1], dtype=torch.int32).view(torch.float32)[0]       # all bits set
    counts = torch.arange(5 * 4, dtype=torch.int64).reshape(5, 4) * (1 << 33)
    tab = MetricTable(5, 1, torch.device("cpu"))
    tab.add(3, loss[3:], counts[3:])
    tab.add(0, loss[:3], counts[:3])
    tab.finish()
    assert tab.losses().dtype == np.float32
    assert tab.losses().view(np.int32).tolist() == loss.view(torch.int32).tolist()
    assert tab.agree().tolist() == counts[:, 0].tolist() and tab.tcount().tolist() == counts[:, 1].tolist()
    assert tab.pcount(0).tolist() == counts[:, 2].tolist() and tab.icount(0).tolist() == counts[:, 3].tolist()
    with pytest.raises(ValueError):
        tab.add(4, loss[:2], counts[:2])


# ---- the build
def test_kernel_sets_of_the_build():
    """metrics.hip holds exactly its two kernels, free of scratch and spills; plastic.hip, whose BCE
    code moved into bce_common.h, holds the kernels it held (tests/test_head_matrix.py pins the list)."""
    import build_native
    import head_matrix as M
    from wgrad_matrix import demangle
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    by_source = {}
    for sym, k in d["kernels"].items():
        by_source.setdefault(k["source"], []).append(sym)
    mine = by_source.get("metrics.hip", [])
    assert sorted(demangle(s) for s in mine) == ["seg_metrics_finish_kernel", "seg_metrics_partial_kernel"]
    for sym in mine:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (sym, k)
    plastic = {demangle(s) for s in by_source["plastic.hip"]}
    assert {k for k in plastic if "bce" in k} == {"bce_partial_kernel", "bce_final_kernel", "bce_bwd_kernel"}
    claimed = set().union(*(r.kernels for r in M.CASES))
    assert plastic | {demangle(s) for s in by_source["adam.hip"]} == claimed and len(claimed) == M.KERNEL_COUNT


# ---- the entry points
class _Net:
    """a stand-in model on the CPU: probabilities from the image, the trace ignored"""

    def __init__(self):
        self.batches = []

    def eval(self):
        return self

    def initialZeroHebb(self, B):
        return torch.zeros(B, 1)

    def __call__(self, x, hebb):
        self.batches.append(x.shape[0])
        return torch.sigmoid(8.0 * (x[:, 0] - 0.5)), hebb


def _host_bce(y, t):
    return torch.nn.functional.binary_cross_entropy(y, t)


def _numpy_seg_metrics(calls):
    """kernels.seg_metrics in torch / numpy on the CPU, for the host-side plumbing"""
    def seg_metrics(y, t, thresholds=()):
        calls.append((y.shape[0], len(thresholds)))
        loss = torch.stack([_host_bce(y[b], t[b]) for b in range(y.shape[0])])
        yn, tn = y.numpy(), t.numpy()
        fg = (tn >= 0.5) & (tn <= 1.0)
        cols = [((tn > 0) == (yn > 0.5)).sum(1), fg.sum(1)]
        cols += [(yn.astype(np.float64) > th).sum(1) for th in thresholds]
        cols += [((yn.astype(np.float64) > th) & fg).sum(1) for th in thresholds]
        return loss, torch.from_numpy(np.stack(cols, 1).astype(np.int64))
    return seg_metrics


def _data(n=7, size=12):
    g = np.random.RandomState(4)
    X = g.rand(n, 1, size, size).astype(np.float32)
    Y = (g.rand(n, 1, size, size) > 0.5).astype(np.float32)
    Y[1], Y[2] = 0.0, 1.0
    return X, Y


def test_host_path_never_calls_seg_metrics(monkeypatch):
    ev = _ev()
    from punet import kernels as K
    calls = []
    monkeypatch.setattr(K, "seg_metrics", _numpy_seg_metrics(calls))
    monkeypatch.setattr(ev, "bce_loss", _host_bce)
    X, Y = _data()
    cpu = torch.device("cpu")
    host = ev.eval_net(_Net(), X, Y, cpu, batch=3, metrics="host")
    crit = ev.eval_net(_Net(), X, Y, cpu, criterion=_host_bce, batch=3)
    crit_dev = ev.eval_net(_Net(), X, Y, cpu, criterion=_host_bce, batch=3, metrics="device")
    sweep = ev.iou_sweep(_Net(), X, Y, cpu, LOGIT_TH, batch=3, metrics="host")
    assert calls == []
    assert host == crit == crit_dev
    # ... and with the kernel stood in for on the CPU, the device plumbing gives the host path's bits
    net = _Net()
    assert ev.eval_net(net, X, Y, cpu, batch=3) == host
    assert calls == [(3, 0), (3, 0), (1, 0)] and net.batches == [3, 3, 1]
    del calls[:]
    got = ev.iou_sweep(_Net(), X, Y, cpu, LOGIT_TH, batch=4)
    assert calls == [(4, 31), (3, 31)]
    assert got.dtype == sweep.dtype == np.float32 and got.tobytes() == sweep.tobytes()
    assert ev.score_model_best_iou(_Net(), X, Y, cpu, batch=4) == ev.score_model_best_iou(_Net(), X, Y, cpu, batch=4,
                                                                                          metrics="host")
    # more than 32 thresholds: in groups of 32
    many = np.linspace(-3, 3, 70)
    del calls[:]
    assert ev.iou_sweep(_Net(), X, Y, cpu, many, batch=7).tobytes() == \
        ev.iou_sweep(_Net(), X, Y, cpu, many, batch=7, metrics="host").tobytes()
    assert calls == [(7, 32), (7, 32), (7, 6)]


def test_entry_points_reject_an_unknown_metrics_path():
    ev = _ev()
    X, Y = _data(3)
    for call in (lambda: ev.eval_net(_Net(), X, Y, torch.device("cpu"), metrics="gpu"),
                 lambda: ev.iou_sweep(_Net(), X, Y, torch.device("cpu"), LOGIT_TH, metrics=None)):
        with pytest.raises(ValueError, match="metrics"):
            call()
