"""The device validation metrics on the GPU (csrc/metrics.hip through kernels.seg_metrics, and the
entry points of eval.py on top of it).

Every check is an equality: the counts are integers taken from numpy with the comparisons the host
path makes (an fp32 array against a float64 threshold is compared in fp64), the loss is compared as
bits with kernels.bce_fwd on the sample, and the entry points are compared with their own host path.

Sizes: n = 1, 7 (less than a wave), 255 / 256 / 257 (one block, exactly one, two), 32^2 and 101^2
(validation sizes: 4 and 40 blocks) and 512 * 256 + 257, the first size past the cap of 512 blocks,
where a thread owns two elements.  T = 0 (no threshold loop), 1, 31 (the logit thresholds of
score_model_best_iou) and 32 (the most an entry takes)."""
import datetime
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, PKG, golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F32 = np.float32
NS = [1, 7, 255, 256, 257, 32 * 32, 101 * 101, 512 * 256 + 257]
BS = [1, 3]
LOGIT_TH = np.log(np.linspace(0.3, 0.7, 31) / (1 - np.linspace(0.3, 0.7, 31)))
# 32 ascending ones: below every y, zero, a denormal bound, values fp32 cannot hold, values it can, 1
ANY_TH = np.unique(np.concatenate([[-0.25, 0.0, 1e-300, 0.1, 0.25, 0.5, 1.0 - 2.0 ** -30, 1.0],
                                   np.random.RandomState(8).rand(24)]))
THRESHOLDS = {0: np.zeros(0), 1: LOGIT_TH[20:21], 31: LOGIT_TH, 32: ANY_TH}
assert all(len(v) == k for k, v in THRESHOLDS.items())


def _bound_above(th):
    """the smallest fp32 above th, as the entry forms it"""
    f = F32(th)
    return f if float(f) > th else np.nextafter(f, F32(np.inf))


def _plants():
    """(values of y for every sample, values of y for the one special sample)"""
    every, special = [F32(0), F32(1), F32(0.5), np.nextafter(F32(0.5), F32(1))], [F32(np.nan), F32(np.inf), F32(-np.inf)]
    for th in np.concatenate([LOGIT_TH, ANY_TH]):
        f = _bound_above(th)
        for v in (f, np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf)), F32(th)):
            (every if 0 <= v <= 1 else special).append(v)     # outside [0, 1] the loss is NaN: one sample only
    return every, special


@functools.lru_cache(maxsize=None)
def _data(n, B):
    """y random in [0, 1] and t random {0, 1}, with the planted values at distinct random positions (as
    many as fit, in the order of the lists); sample 0 alone holds NaN, the infinities and every y
    outside [0, 1]"""
    g = np.random.RandomState(1000 * B + n % 997)
    y = g.rand(B, n).astype(F32)
    t = (g.rand(B, n) > 0.5).astype(F32)
    every, special = _plants()
    t_every = [F32(0.5), np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(1), F32(2)), F32(-1), F32(2)]
    for b in range(B):
        ys = (special if b == 0 else []) + every[b % 4:] + every[:b % 4]
        ts = ([F32(np.nan)] if b == 0 else []) + t_every[b % 5:] + t_every[:b % 5]
        for arr, vals in ((y, ys), (t, ts)):
            pos = g.permutation(n)[:len(vals)]
            arr[b, pos] = vals[:len(pos)]
    y.setflags(write=False)
    t.setflags(write=False)
    return y, t


@functools.lru_cache(maxsize=None)
def _want(n, B, T):
    y, t = _data(n, B)
    fg = (t >= 0.5) & (t <= 1.0)
    cols = [((t > 0) == (y > F32(0.5))).sum(1), fg.sum(1)]
    above = [y.astype(np.float64) > th for th in THRESHOLDS[T]]
    cols += [a.sum(1) for a in above] + [(a & fg).sum(1) for a in above]
    return np.stack(cols, 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _got(n, B, T):
    from punet import kernels as K
    y, t = _data(n, B)
    loss, counts = K.seg_metrics(torch.tensor(y, device=DEV), torch.tensor(t, device=DEV), THRESHOLDS[T])
    assert loss.shape == (B,) and loss.dtype == torch.float32 and counts.shape == (B, 2 + 2 * T) and counts.dtype == torch.int64
    return loss.cpu().numpy(), counts.cpu().numpy()


def test_planted_values_are_there():
    y, t = _data(101 * 101, 3)
    every, special = _plants()
    assert np.isnan(y[0]).sum() == 1 and np.isinf(y[0]).sum() == 2 and np.isnan(t[0]).sum() == 1
    assert np.isfinite(y[1:]).all() and y[1:].min() == 0 and y[1:].max() == 1 and np.isfinite(t[1:]).all()
    assert (y[0] < 0).any() and (y[0] > 1).any()
    for b in range(3):
        assert set(np.asarray(every).tolist()) <= set(y[b].tolist())
        assert {0.5, float(np.nextafter(F32(0.5), F32(0))), float(np.nextafter(F32(1), F32(2))), -1.0, 2.0} <= set(t[b].tolist())
    # a bound, the value below it and the threshold itself fall on different sides of the fp64 comparison
    th = LOGIT_TH[20]
    f = _bound_above(th)
    assert float(f) > th >= float(np.nextafter(f, F32(-np.inf)))
    assert _bound_above(1e-300) == np.nextafter(F32(0), F32(1)) and _bound_above(0.5) == np.nextafter(F32(0.5), F32(1))


@pytest.mark.parametrize("T", sorted(THRESHOLDS))
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", NS)
def test_counts_are_exact(n, B, T):
    counts, want = _got(n, B, T)[1], _want(n, B, T)
    assert np.array_equal(counts, want), np.argwhere(counts != want)[:8]
    if n >= 255 and T > 1:
        assert len(np.unique(want[:, 2:2 + T])) > 1       # the thresholds tell the pixels apart


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", NS)
def test_loss_has_the_bits_of_bce_fwd(n, B):
    from punet import kernels as K
    y, t = _data(n, B)
    yd, td = torch.tensor(y, device=DEV), torch.tensor(t, device=DEV)
    want = torch.stack([K.bce_fwd(yd[b], td[b]) for b in range(B)]).cpu().numpy()
    assert np.isnan(want[0])                          # the special sample
    assert np.isfinite(want[1:]).all()
    if B > 1 and n >= 255:
        assert ((y[1:] == 0).any(1) & (y[1:] == 1).any(1)).all()      # both clamps at -100 in a finite loss
    for T in sorted(THRESHOLDS):
        got = _got(n, B, T)[0]
        assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (T, got, want)


@pytest.mark.parametrize("n", [7, 257, 101 * 101, 512 * 256 + 257])
def test_alignment_and_repeatability(n):
    """views one element into a buffer (4-byte aligned pointers) and a second call on the same data"""
    from punet import kernels as K
    B, T = 3, 31
    y, t = _data(n, B)
    loss, counts = _got(n, B, T)
    yo, to = (torch.zeros(B * n + 1, device=DEV) for _ in range(2))
    yo[1:] = torch.tensor(y, device=DEV).reshape(-1)
    to[1:] = torch.tensor(t, device=DEV).reshape(-1)
    yv, tv = yo[1:].view(B, n), to[1:].view(B, n)
    assert yv.data_ptr() % 8 == 4 and tv.data_ptr() % 8 == 4
    for _ in range(2):
        l2, c2 = K.seg_metrics(yv, tv, THRESHOLDS[T])
        assert l2.cpu().numpy().view(np.int32).tolist() == loss.view(np.int32).tolist()
        assert np.array_equal(c2.cpu().numpy(), counts)


def test_any_shape_with_a_leading_batch_axis_and_size_mismatch():
    from punet import kernels as K
    y, t = _data(32 * 32, 3)
    yd, td = torch.tensor(y, device=DEV), torch.tensor(t, device=DEV)
    loss, counts = K.seg_metrics(yd.view(3, 1, 32, 32), td.view(3, 32, 32), THRESHOLDS[1])
    assert loss.cpu().numpy().view(np.int32).tolist() == _got(32 * 32, 3, 1)[0].view(np.int32).tolist()
    assert np.array_equal(counts.cpu().numpy(), _got(32 * 32, 3, 1)[1])
    with pytest.raises(ValueError, match=r"Target size \(\(2, 1024\)\) must be the same as input size \(\(3, 1024\)\)"):
        K.seg_metrics(yd, td[:2])
    with pytest.raises(RuntimeError, match="pu_seg_metrics: thresholds\\[1\\] is not above"):
        K.seg_metrics(yd, td, [0.5, 0.5])


# ---- the entry points
def _eval():
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    import eval as ev
    return ev


def _capture_net():
    """the model of tests/golden/train_capture.npz after its two epochs, as tests/test_entry_gpu.py builds it"""
    from unet import UNetp
    g = golden("train_capture.npz")
    net = UNetp(1, 1, DEV, rule="oja", nbf=32)
    net.load_state_dict({k[6:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("final.")})
    return net, g


class _Calls:
    """kernels.seg_metrics, counting its calls"""

    def __init__(self):
        from punet import kernels as K
        self.K, self.inner, self.calls = K, K.seg_metrics, []

    def __enter__(self):
        self.K.seg_metrics = self
        return self

    def __exit__(self, *exc):
        self.K.seg_metrics = self.inner

    def __call__(self, y, t, thresholds=()):
        self.calls.append((y.shape[0], len(thresholds)))
        return self.inner(y, t, thresholds)


def test_eval_net_is_unchanged():
    """four samples in chunks of three (a ragged tail): the device path returns the host path's floats"""
    ev = _eval()
    net, g = _capture_net()
    X = np.concatenate([g["X_train"], g["X_val"]])
    Y = np.concatenate([g["y_train"], g["y_val"]])
    assert len(X) == 4
    host = ev.eval_net(net, X, Y, DEV, batch=3, metrics="host")
    with _Calls() as rec:
        dev = ev.eval_net(net, X, Y, DEV, batch=3, metrics="device")
        assert rec.calls == [(3, 0), (1, 0)]
        assert ev.eval_net(net, X, Y, DEV, batch=3) == dev            # the default
        assert len(rec.calls) == 4
        assert ev.eval_net(net, X, Y, DEV, batch=3, metrics="host") == host and len(rec.calls) == 4
    print("eval_net device %r host %r" % (dev, host))
    assert dev[0] == host[0] and dev[1] == host[1]
    assert 0.0 < host[0] < 1.0 and 0.0 < host[1] < 10.0


def test_iou_sweep_and_best_threshold_are_unchanged():
    """UNetpRes(nbf=32) with w scaled by 40 (masks away from 0.5, the setup of
    test_start_inference_writes_the_oracles_submission), six samples in chunks of four"""
    import oracle
    from unet import UNetpRes
    ev = _eval()
    N = 32
    torch.manual_seed(17)
    ref = oracle.RefUNetpRes(1, 1, nbf=N)
    with torch.no_grad():
        ref.w.mul_(40.0)
    net = UNetpRes(n_channels=1, n_classes=1, nbf=N, device=DEV)
    net.load_state_dict(ref.state_dict())
    g = np.random.RandomState(5)
    X = g.rand(6, 1, N, N).astype(np.float32)
    Y = (g.rand(6, 1, N, N) > 0.5).astype(np.float32)
    host = ev.iou_sweep(net, X, Y, DEV, LOGIT_TH, batch=4, metrics="host")
    with _Calls() as rec:
        dev = ev.iou_sweep(net, X, Y, DEV, LOGIT_TH, batch=4)
        assert rec.calls == [(4, 31), (2, 31)]
    print("iou_sweep device %s\niou_sweep host   %s" % (dev, host))
    assert dev.dtype == host.dtype == np.float32 and dev.shape == host.shape == (31,)
    assert dev.tobytes() == host.tobytes()
    assert len(np.unique(host)) > 1                               # the sweep moves the score
    th_d, iou_d = ev.score_model_best_iou(net, X, Y, DEV, batch=4)
    th_h, iou_h = ev.score_model_best_iou(net, X, Y, DEV, batch=4, metrics="host")
    assert th_d == th_h == LOGIT_TH[int(np.argmax(host))] and iou_d == iou_h == host.max()


# ---- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _five_samples():
    g = np.random.RandomState(12)
    return g.rand(5, 1, 32, 32).astype(np.float32), (g.rand(5, 1, 32, 32) > 0.5).astype(np.float32)


def _worker(rank, world, port, out_dir):
    ev = _eval()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))      # a stuck rank ends the test
    net, _ = _capture_net()
    X, Y = _five_samples()
    with _Calls() as rec:
        acc, loss = ev.eval_net(net, X, Y, DEV, batch=2)
    torch.save({"acc": acc, "loss": loss, "calls": rec.calls}, os.path.join(out_dir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_the_chunks_and_return_the_single_process_floats(tmp_path, gpu_device):
    ev = _eval()
    net, _ = _capture_net()
    X, Y = _five_samples()
    want = ev.eval_net(net, X, Y, DEV, batch=2)
    assert want == ev.eval_net(net, X, Y, DEV, batch=2, metrics="host")
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(os.path.join(tmp_path, "r%d.pt" % r), weights_only=True) for r in range(2)]
    assert res[0]["calls"] == [(2, 0), (1, 0)] and res[1]["calls"] == [(2, 0)]      # chunks 0 and 2; chunk 1
    for r in res:
        assert (r["acc"], r["loss"]) == want, (r, want)
