"""The device run-length encoding (pu_rle_encode: rle_bits_kernel, rle_count_kernel, rle_emit_kernel)
against utils.encode.  Every check is an equality with encode(np.round(m > thr)) per image: the offsets,
the (start, length) pairs in order, and, through infer.predict, the rows and the CSV bytes.

The shapes are the smallest at which the kernels take another path: a single row and a single column;
63, 64 and 65 rows (one partial word, one whole word, two words per column); 130 rows (three words,
the last partial); 130 columns (three column tiles of the bitmap kernel); 101^2 and 128^2; 1024 x 16
and 1024 x 40 (257 and 641 edge words: the emit kernel walks them in two and three steps of 256 and
carries its scan from one to the next)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from punet import _lib, kernels as K  # noqa: E402
from punet.rle import compare_value, rle_strings  # noqa: E402
import rle_ref as R  # noqa: E402

DEV = torch.device("cuda")
SHAPES = [(1, 1), (1, 7), (7, 1), (63, 3), (64, 3), (65, 3), (130, 5), (5, 130), (101, 101), (128, 128), (1024, 16),
          (1024, 40)]
POISON = -7


def _check(y, thr):
    """kernels.rle_encode(y, compare_value(thr)) == the table of encode(np.round(y[b] > thr))"""
    from utils import encode
    offsets, runs = K.rle_encode(torch.from_numpy(y).to(DEV), compare_value(thr))
    assert offsets.dtype == runs.dtype == torch.int32
    B, h, w = y.shape
    assert offsets.shape == (B + 1,) and runs.shape == (B * ((h * w + 1) // 2), 2)
    offsets, runs = offsets.cpu().numpy(), runs.cpu().numpy()
    want = [encode(np.round(m > thr)) for m in y]
    counts = [len(s.split()) // 2 for s in want]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert rle_strings(offsets, runs) == want
    return counts


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_mask_at_every_shape(h, w):
    masks = R.planted_masks(h, w)
    names = list(masks)
    y = R.maps_of(np.stack([masks[k] for k in names]))
    counts = dict(zip(names, _check(y, 0.5)))                   # one batch of the nine
    n = h * w
    assert counts["empty"] == 0 and counts["full"] == 1 and counts["alternating"] == (n + 1) // 2
    for k in names:                                             # each alone: B = 1
        _check(y[names.index(k)][None], 0.5)
    # ragged offsets, one image without a pair, and the random one last, first and in the middle
    e, f, r = (names.index(k) for k in ("empty", "full", "random 0.50"))
    for order in ((e, f, r), (r, e, f), (f, r, e), (e, e, e)):
        _check(y[list(order)], 0.5)


def test_a_batch_of_32_at_101():
    g = np.random.RandomState(3)
    dens = g.rand(32, 1, 1) ** 2
    dens[5], dens[31], dens[0] = 0.0, 1.0, 0.5
    counts = _check(R.maps_of(g.rand(32, 101, 101) < dens, seed=4), 0.5)
    assert counts[5] == 0 and counts[31] == 1 and counts[0] > 2000


@pytest.mark.parametrize("kind", ["float", "float64"])
@pytest.mark.parametrize("thr", [0.5, -0.8472978603872037, 2.0, 0.3])
def test_planted_values_at_the_threshold(thr, kind):
    """the smallest fp32 that passes and its lower neighbour, NaN and the infinities, at the first and
    last pixels and on both sides of every word boundary; thresholds 0.5, a negative logit threshold
    (every probability is foreground) and 2.0 (none is), each as NumPy compares it for its type"""
    thr = float(thr) if kind == "float" else np.float64(thr)
    h, w = 130, 5
    bound = R.bound_above(compare_value(thr))
    below = np.nextafter(bound, np.float32(-np.inf))
    values = [bound, below, np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    spots = [(0, 0), (h - 1, w - 1), (63, 0), (64, 0), (127, 1), (128, 1), (h - 1, 2), (0, 3), (63, 4), (64, 4)]
    y = np.random.RandomState(9).rand(len(values), h, w).astype(np.float32)
    for b in range(len(values)):
        for s, (i, j) in enumerate(spots):
            y[b, i, j] = values[(b + s) % len(values)]
    m = y > thr
    assert m[0, 0, 0] and not m[1, 0, 0]                        # bound passes, its neighbour does not
    assert not (y[2] > thr)[0, 0] and (y[3] > thr)[0, 0] and not (y[4] > thr)[0, 0]
    _check(y, thr)
    if thr < 0:
        assert np.count_nonzero(~m) == 3 * len(spots)           # below, NaN and -inf only ...
    if thr == 2.0:
        assert np.count_nonzero(m) == 2 * len(spots)            # ... bound and +inf only


def _raw(y, th, runs, cap):
    """pu_rle_encode into a buffer of the caller's: (rc, offsets)"""
    L = _lib.load()
    B, h, w = y.shape
    nbytes = L.pu_rle_encode_workspace_bytes(B, h, w)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
    offsets = torch.full((B + 1,), POISON, dtype=torch.int32, device=DEV)
    rc = L.pu_rle_encode(y.data_ptr(), B, h, w, th, offsets.data_ptr(), runs.data_ptr(), cap, ws.data_ptr(), nbytes,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, offsets.cpu().numpy()


def test_cap_bounds_every_store():
    h, w = 65, 3
    masks = R.planted_masks(h, w)
    y = R.maps_of(np.stack([masks[k] for k in ("random 0.50", "alternating", "empty", "random 0.02")]))
    want_off, want = R.table_of(y, 0.5)
    total = int(want_off[-1])
    assert total > (h * w + 1) // 2
    yd = torch.from_numpy(y).to(DEV)
    for cap in (total + 3, total, total - 1, (h * w) // 2, 1, 0):
        runs = torch.full((total + 8, 2), POISON, dtype=torch.int32, device=DEV)
        rc, off = _raw(yd, 0.5, runs, cap)
        assert rc == 0
        assert off.tolist() == want_off.tolist()                # the true offsets, whatever the cap
        got = runs.cpu().numpy()
        kept = min(cap, total)
        assert np.array_equal(got[:kept], want[:kept])
        assert (got[kept:] == POISON).all()                     # nothing from 2 cap on, nor past the total


def test_repeats_views_and_graph_replay():
    h, w, B = 101, 101, 3
    g = np.random.RandomState(21)
    y = R.maps_of(g.rand(B, h, w) < np.array([0.5, 0.02, 0.9]).reshape(B, 1, 1), seed=22)
    want_off, want = R.table_of(y, 0.5)
    total = int(want_off[-1])
    yd = torch.from_numpy(y).to(DEV)
    tables = [K.rle_encode(yd, 0.5) for _ in range(2)]          # the same call twice: the same bits
    big = torch.zeros(B * h * w + 1, device=DEV)                # a view one float into a buffer
    big[1:] = yd.reshape(-1)
    view = big[1:].view(B, h, w)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    tables.append(K.rle_encode(view, 0.5))
    side = torch.cuda.Stream()                                  # captured, replayed once
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.rle_encode(yd, 0.5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = K.rle_encode(yd, 0.5)
    captured[0].fill_(POISON), captured[1].fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    tables.append(captured)
    for offsets, runs in tables:
        assert offsets.cpu().numpy().tolist() == want_off.tolist()
        assert np.array_equal(runs.cpu().numpy()[:total], want)


def test_wrapper_shapes_and_cap():
    y = torch.rand(2, 9, 5, device=DEV)
    for bad in (y[0], y[None], y[:, :0], y[:0]):
        with pytest.raises(ValueError, match="rle_encode"):
            K.rle_encode(bad, 0.5)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        K.rle_encode(y.transpose(1, 2), 0.5)
    with pytest.raises(RuntimeError, match="pu_rle_encode failed"):
        K.rle_encode(y, float("nan"))
    offsets, runs = K.rle_encode(y, 0.5, cap=0)                 # counting alone
    assert runs.shape == (0, 2) and offsets.cpu().numpy().tolist() == R.table_of(y.cpu().numpy(), 0.5)[0].tolist()


# ---- the entry points
def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _net(N, neurons):
    from unet import UNetpRes
    torch.manual_seed(17)
    net = UNetpRes(n_channels=1, n_classes=1, nbf=N, device=DEV, neurons=neurons)
    with torch.no_grad():
        net.w.mul_(40.0)                                        # masks that are not all near 0.5
    return net


@pytest.mark.parametrize("thr", [0.5, np.float64(0.4999)])
def test_predict_gives_the_host_paths_rows_and_file(tmp_path, thr):
    import infer
    N = 101
    net = _net(N, 8)
    X = np.random.RandomState(5).rand(70, 1, N, N).astype(np.float32)       # chunks of 32, 32 and 6
    ids = ["img%d" % i for i in range(len(X))]
    rows = {}
    for rle in ("device", "host"):
        out = str(tmp_path / rle)
        os.makedirs(out)
        rows[rle] = infer.predict(net, (ids, X), {"device": DEV, "mask_threshold": thr, "out_dir": out}, rle=rle)
    assert rows["device"] == rows["host"] and [r[0] for r in rows["device"]] == ids
    assert _read(str(tmp_path / "device" / "submission.csv")) == _read(str(tmp_path / "host" / "submission.csv"))
    lengths = [len(r[1]) for r in rows["device"]]
    assert max(lengths) > 100                                   # real masks, not 70 empty strings


def test_start_inference_gives_the_same_both_ways(tmp_path):
    import infer
    N = 101
    net = _net(N, 16)                                            # start_inference builds the default width
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    g = np.random.RandomState(6)
    X_valid = g.rand(6, 1, N, N).astype(np.float32)
    # the model's own masks at 0.62 as the truth: the threshold search (an np.float64) ends inside (0, 1)
    y_valid = (infer.predict_masks(net, X_valid, DEV) > 0.62).astype(np.float32)[:, None]
    X = g.rand(40, 1, N, N).astype(np.float32)
    ids = ["t%d" % i for i in range(len(X))]
    rows = {}
    for rle in ("device", "host"):
        out = str(tmp_path / rle)
        rows[rle] = infer.start_inference(sd, (ids, X), X_valid, y_valid, out, N, N, 1, rle=rle)
    assert rows["device"] == rows["host"] and len(rows["device"]) == 40
    assert _read(str(tmp_path / "device" / "submission.csv")) == _read(str(tmp_path / "host" / "submission.csv"))
    assert max(len(r[1]) for r in rows["device"]) > 100
