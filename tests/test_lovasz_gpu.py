"""The device Lovasz loss (pu_lovasz_fwd: lovasz_image_kernel, lovasz_finish_kernel; pu_lovasz_bwd:
lovasz_bwd_kernel) against the numpy restatement of its contract (tests/lovasz_ref.py), and its wiring
into the Trainer and train.py.

D is compared bit for bit: both sides run the same IEEE fp64 operations on the same integer counts and
round once.  loss_per_image and loss are held within 1 fp32 ulp of the fp64 value: only the order of the
sums differs.

The sizes are the smallest at which the kernel takes another path: 1, 2, 3 (one thread, most of its 16
keys padding, no stage through LDS); 63, 64 (P = 64: merges with one and two LDS stages, an odd and a
full last chunk) and 65 (P = 128: three LDS stages in one pass); 1023, 1024 (the 8 KiB kernel full: six
LDS stages, a pass of two and one of four) and 1025 (the 32 KiB kernel, 256 threads: a second wave in the
scan); 4097 (the 128 KiB kernel at half its keys, half its threads idle); 10201 = 101^2 and 16384 = 128^2
(1024 threads, ten LDS stages in three passes); B 32 at 1024."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402
from punet import _lib, kernels as K  # noqa: E402
from punet import LovaszLoss, lovasz_loss, bce_loss, FusedAdam  # noqa: E402
from punet.engine import Trainer  # noqa: E402
from unet import UNetp  # noqa: E402
import lovasz_ref as R  # noqa: E402

DEV = torch.device("cuda")
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097, 10201, 16384]
POISON = 7.0          # no entry of D: |D| <= 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(y, t):
    """kernels.lovasz_fwd on the device against the restatement: D bit for bit, the losses within 1 ulp"""
    B, n = y.shape
    loss, per, D = K.lovasz_fwd(torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV))
    assert loss.shape == () and per.shape == (B,) and D.shape == (B, n)
    assert loss.dtype == per.dtype == D.dtype == torch.float32
    want_loss, want_per, want_D = R.batch(y, t)
    got_D = D.cpu().numpy()
    diff = np.flatnonzero(bits(got_D) != bits(want_D))
    assert diff.size == 0, (diff[:5], got_D.reshape(-1)[diff[:5]], want_D.reshape(-1)[diff[:5]])
    got_per = per.cpu().numpy()
    for b in range(B):
        assert abs(float(got_per[b]) - want_per[b]) <= R.ulp32(want_per[b]), (b, got_per[b], want_per[b])
    assert abs(float(loss.item()) - want_loss) <= R.ulp32(want_loss), (loss.item(), want_loss)
    return want_per


@pytest.mark.parametrize("n", SIZES)
def test_every_mask_and_probability_kind_at_every_size(n):
    for B in (1, 3):
        for mi, mask in enumerate(R.MASKS):
            for pi, prob in enumerate(R.PROBS):
                g = np.random.RandomState(1000 * n % 9973 + 100 * B + 10 * mi + pi)
                y, t = R.probabilities(prob, B, n, g), R.targets(mask, B, n, g)
                per = _check(y, t)
                if mask == "empty":                              # G = 0: the largest probability
                    assert np.array_equal(np.float32(per), y.max(axis=1))


@pytest.mark.parametrize("n", [65, 1025])
def test_negative_zero_ties_with_zero_by_index(n):
    """a background y of -0 is e = -0: it ranks with the e = +0 of a background 0 and a foreground 1, by
    pixel index, not above every other pixel as its bits would"""
    g = np.random.RandomState(n)
    pool = np.array([-0.0, 0.0, 1.0, 0.5, -0.0], dtype=np.float32)
    y = pool[g.randint(0, len(pool), (3, n))]
    t = R.targets("random", 3, n, g)
    assert np.signbit(y[t == 0]).any() and (y[t == 1] == 1).any()
    _check(y, t)
    plus = np.where(y == 0, np.float32(0.0), y)                  # the same maps with +0 for every -0
    D = [K.lovasz_fwd(torch.from_numpy(a).to(DEV), torch.from_numpy(t).to(DEV))[2] for a in (y, plus)]
    assert torch.equal(D[0], D[1])


def test_a_batch_of_32_at_1024():
    g = np.random.RandomState(32)
    B, n = 32, 1024
    for prob in ("uniform", "eighths"):
        y = R.probabilities(prob, B, n, g)
        t = R.targets("random", B, n, g)
        t[5], t[31] = 0.0, 1.0                                   # an empty and a full mask among them
        _check(y, t)


@pytest.mark.parametrize("n", [5, 1024, 10201])
def test_vertices_give_the_jaccard_loss(n):
    """y in {0, 1}: loss_b = 1 - |P and T| / |P or T|, 0 when both are empty"""
    g = np.random.RandomState(n)
    p = g.rand(6, n) < g.rand(6, 1)
    t = g.rand(6, n) < g.rand(6, 1)
    p[0], t[0] = False, False
    p[1], t[1] = True, False
    p[2], t[2] = False, True
    p[3], t[3] = True, True
    _, per, _ = K.lovasz_fwd(torch.from_numpy(p.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.float32)).to(DEV))
    per = per.cpu().numpy()
    for b in range(6):
        union = np.count_nonzero(p[b] | t[b])
        want = 1.0 - np.count_nonzero(p[b] & t[b]) / union if union else 0.0
        assert abs(float(per[b]) - want) <= R.ulp32(want), (b, per[b], want)
    assert per[0] == 0.0 and per[1] == 1.0 and per[2] == 1.0 and per[3] == 0.0


def test_repeats_and_an_offset_view_give_equal_bits():
    B, n = 3, 10201
    g = np.random.RandomState(77)
    y = torch.from_numpy(R.probabilities("eighths", B, n, g)).to(DEV)
    t = torch.from_numpy(R.targets("random", B, n, g)).to(DEV)
    runs = [K.lovasz_fwd(y, t) for _ in range(2)]
    big_y, big_t = torch.zeros(B * n + 1, device=DEV), torch.zeros(B * n + 1, device=DEV)
    big_y[1:], big_t[1:] = y.reshape(-1), t.reshape(-1)
    vy, vt = big_y[1:].view(B, n), big_t[1:].view(B, n)
    assert vy.data_ptr() % 8 == 4 and vy.is_contiguous()
    runs.append(K.lovasz_fwd(vy, vt))
    for loss, per, D in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(per, runs[0][1]) and torch.equal(D, runs[0][2])


@pytest.mark.parametrize("n", [3, 65, 1025, 10201])
def test_poisoned_table_is_overwritten_and_nothing_past_it(n):
    L = _lib.load()
    B, margin = 3, 64
    g = np.random.RandomState(n)
    y = torch.from_numpy(R.probabilities("planted", B, n, g)).to(DEV)
    t = torch.from_numpy(R.targets("random", B, n, g)).to(DEV)
    buf = torch.full((B * n + 2 * margin,), POISON, device=DEV)
    per = torch.full((B + 2,), POISON, device=DEV)
    loss = torch.full((3,), POISON, device=DEV)
    nbytes = L.pu_lovasz_workspace_bytes(B, n)
    ws = torch.empty(B + 2, dtype=torch.float64, device=DEV)
    rc = L.pu_lovasz_fwd(y.data_ptr(), t.data_ptr(), B, n, loss.data_ptr() + 4, per.data_ptr() + 4,
                         buf.data_ptr() + 4 * margin, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    buf, per, loss = buf.cpu().numpy(), per.cpu().numpy(), loss.cpu().numpy()
    assert (buf[:margin] == POISON).all() and (buf[margin + B * n:] == POISON).all()
    inside = buf[margin:margin + B * n]
    assert (np.abs(inside) <= 1.0).all()                         # every cell written
    assert np.array_equal(bits(inside.reshape(B, n)), bits(R.batch(y.cpu().numpy(), t.cpu().numpy())[2]))
    assert per[0] == POISON and per[-1] == POISON and (per[1:-1] != POISON).all()
    assert loss[0] == POISON and loss[2] == POISON and loss[1] != POISON


def test_unsupported_size_raises_with_the_size():
    y = torch.rand(1, 16385, device=DEV)
    with pytest.raises(ValueError, match="16385"):
        K.lovasz_fwd(y, y)
    with pytest.raises(ValueError, match="65536"):
        lovasz_loss(torch.rand(2, 256, 256, device=DEV), torch.rand(2, 256, 256, device=DEV))


@pytest.mark.parametrize("gval", [1.0, 0.37])
def test_backward_is_the_table_times_g_over_b(gval):
    B, n = 3, 10201
    g = np.random.RandomState(3)
    y = torch.from_numpy(R.probabilities("uniform", B, n, g)).to(DEV)
    t = torch.from_numpy(R.targets("random", B, n, g)).to(DEV)
    _, _, D = K.lovasz_fwd(y, t)
    dy = K.lovasz_bwd(D, torch.tensor(gval, device=DEV))
    want = R.backward(D.cpu().numpy(), gval, B)
    assert np.array_equal(bits(dy.cpu().numpy()), bits(want))
    if gval == 1.0:                                              # no grad_loss: 1
        assert torch.equal(K.lovasz_bwd(D, None), dy)
    # ... and through autograd, [B, H, W] and the module
    yy = y.view(B, 101, 101).clone().requires_grad_(True)
    (LovaszLoss()(yy, t.view(B, 101, 101)) * gval).backward()
    assert np.array_equal(bits(yy.grad.cpu().numpy().reshape(B, n)), bits(want))


# ---- wiring
N, BS = 32, 2


def _net(seed=11, **kw):
    torch.manual_seed(seed)
    net = UNetp(1, 1, DEV, rule="oja", nbf=N, depth=3, base_ch=8, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.alpha.copy_(0.5 * torch.rand(net.alpha.shape, generator=g))
        net.w.mul_(20.0)                                        # probabilities that are not all near 0.5
    return net


def _twin(net, **kw):
    twin = UNetp(1, 1, DEV, rule="oja", nbf=N, depth=3, base_ch=8, **kw)
    twin.load_state_dict(net.state_dict())
    return twin


def _data(steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(steps, BS, 1, N, N, generator=g).to(DEV)
    ts = (torch.rand(steps, BS, N, N, generator=g) > 0.6).float().to(DEV)
    H = (0.05 * torch.randn(BS, N, N, generator=g)).to(DEV)
    return xs, ts, H


def _same(net_a, net_b):
    for (k, p), (_, q) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(p, q), k
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), k


@pytest.mark.parametrize("name,weight", [("lovasz", 1.0), ("bce+lovasz", 0.5)])
def test_trainer_step_equals_the_manual_sequence(name, weight):
    net = _net()
    manual = _twin(net)
    xs, ts, H = _data(2)
    tr = Trainer(net, lr=1e-3, steplr=1e5, loss=name, lovasz_weight=weight)
    opt = FusedAdam(manual.parameters(), lr=1e-3)
    h_a, h_b = H, H
    for s in range(2):
        loss_a, h_a = tr.step(xs[s], ts[s], h_a)
        for p in manual.parameters():
            p.grad = None
        y, h_b = manual(xs[s], h_b.detach())
        if name == "lovasz":
            loss_b = lovasz_loss(y, ts[s])
        else:
            loss_b = bce_loss(y, ts[s]) + weight * lovasz_loss(y, ts[s])
        loss_b.backward()
        opt.step()
        assert torch.equal(loss_a, loss_b.detach()) and torch.equal(h_a, h_b.detach())
        _same(net, manual)
    # the loss returned is the one optimised: not the BCE of the same step
    assert not torch.equal(loss_a, bce_loss(y.detach(), ts[1]))


def test_graph_steps_equal_eager_steps():
    res = []
    for graph in (False, True):
        net = _net()
        xs, ts, hebb = _data(4)
        tr = Trainer(net, lr=1e-3, steplr=1e5, loss="lovasz", graph=graph)
        losses = []
        for s in range(4):
            loss, hebb = tr.step(xs[s], ts[s], hebb)
            losses.append(loss.item())
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        res.append((losses, net, hebb.clone()))
    assert res[0][0] == res[1][0] and len(set(res[0][0])) == 4
    _same(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


def test_restatements_dy_gives_the_same_parameter_gradients():
    """The device's own y, dy from the numpy restatement, pushed through y.backward on an identical net:
    the parameter gradients of lovasz_loss(...).backward(), bit for bit"""
    net = _net()
    twin = _twin(net)
    xs, ts, H = _data(1)
    y, _ = net(xs[0], H)
    lovasz_loss(y, ts[0]).backward()
    y2, _ = twin(xs[0], H)
    assert torch.equal(y, y2)
    _, _, D = R.batch(y.detach().cpu().numpy().reshape(BS, -1), ts[0].cpu().numpy().reshape(BS, -1))
    dy = torch.from_numpy(R.backward(D, 1.0, BS)).to(DEV).view_as(y2)
    assert dy.abs().max().item() > 0
    y2.backward(dy)
    _same(net, twin)
    assert net.w.grad.abs().max().item() > 0


def test_episode_of_two_runs_with_finite_gradients():
    net = _net(trace_grad=True)
    with torch.no_grad():
        net.eta.fill_(0.1)
    xs, ts, H = _data(2)
    tr = Trainer(net, lr=1e-3, steplr=100, loss="lovasz")
    losses, h = tr.step_episode(xs, ts, H)
    assert losses.shape == (2,) and torch.isfinite(losses).all() and (losses > 0).all() and (losses <= 1).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert net.eta.grad.abs().item() > 0 and torch.isfinite(h).all()


def test_train_cli_with_the_lovasz_loss_writes_its_checkpoint(tmp_path):
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--loss", "lovasz", "--synthetic", "8", "--img-size", "64",
                        "--model-type", "unetp", "--batch-size", "2", "-e", "1", "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(os.path.join(out, "train_net.pth"))
    with open(os.path.join(out, "train_parameters.dat"), "rb") as f:
        params = pickle.load(f)
    assert params["loss"] == "lovasz" and params["lovasz_weight"] == 1.0
    with np.load(os.path.join(out, "train_data.npz")) as z:
        losses = z["train/all_losses"]
    assert losses.shape == (3,) and np.all(np.isfinite(losses)) and np.all((losses > 0) & (losses <= 1))
