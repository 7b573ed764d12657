"""Gradient clipping by global norm on the device (csrc/clip.hip): pu_grad_norm and pu_adam_multi_clipped
against fp64 and against the unclipped entry, bit for bit where the design promises bits, then
through FusedAdam / Trainer: plain steps, the HIP-graph step, episodes and two data-parallel ranks.

The size lists are those of the Adam rows of tests/head_matrix.py: the smallest at which the 4096-
element chunks, the 32-tensor launches and the tail / alignment paths can go wrong."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from conftest import ROOT, PKG  # noqa: E402
from unet import UNetp  # noqa: E402
from punet import dp, kernels as K  # noqa: E402
from punet.engine import Trainer  # noqa: E402
import oracle  # noqa: E402

DEV = torch.device("cuda")

SIZES = {
    "sizes": (1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 5),
    "empty between": (4096, 0, 5),
    "33 tensors": tuple(range(1, 34)),
    "65 tensors": tuple(7 + i % 5 for i in range(65)),
    "g + 4 B": (4097, 9),
}
MIS = {"g + 4 B": 0}        # the tensor of the list whose pointer is moved by 4 bytes


def place(values, mis=False):
    """values on the device in storage of their own, 16-byte aligned or 4 bytes past that"""
    n = values.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device=DEV)
    base = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    out = base[1:n + 1] if mis else base[:n]
    out.copy_(values)
    return out


def grad_values(numels, seed=0):
    """seeded normal values, each tensor times its own scale from 1e-3 to 1e3"""
    g = torch.Generator().manual_seed(seed)
    k = max(len(numels) - 1, 1)
    return [torch.randn(n, generator=g) * 10.0 ** (-3 + 6 * i / k) for i, n in enumerate(numels)]


def host_norm(values):
    """sqrt(sum g.double()^2) on the host, rounded to fp32"""
    return np.float32(math.sqrt(sum((v.double() ** 2).sum().item() for v in values)))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def torch_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient in fp32 tensors: clamp(max_norm / (total_norm + 1e-6), max=1)"""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------ 1. norm against fp64
@pytest.mark.parametrize("name", list(SIZES))
def test_norm_against_fp64(name):
    """The squares are exact in fp64 and a fp64 sum of n <= 2^24 terms has relative error
    <= n 2^-53 << 2^-24: only the final rounding to fp32 can differ, so the bar is 1 ulp."""
    vals = grad_values(SIZES[name])
    grads = [place(v, MIS.get(name) == i) for i, v in enumerate(vals)]
    out = K.grad_norm(grads, 1.0).cpu()
    ref = host_norm(vals)
    print(name, "norm", out[0].item(), "host fp64", ref, "ulps", ulps(out[0].item(), ref))
    assert ulps(out[0].item(), ref) <= 1
    for g, v in zip(grads, vals):
        assert torch.equal(g.cpu(), v)          # read only


def test_norm_of_zeros_and_of_nothing():
    zeros = [place(torch.zeros(n)) for n in SIZES["sizes"]]
    assert K.grad_norm(zeros, 2.5).cpu().tolist() == [0.0, 1.0]
    assert K.grad_norm([place(torch.zeros(0)), place(torch.zeros(0))], 2.5).cpu().tolist() == [0.0, 1.0]


@pytest.mark.parametrize("value", [1e20, 1e-30])
def test_norm_outside_the_range_of_fp32_squares(value):
    """1e20^2 overflows fp32 and 1e-30^2 underflows it: an fp32 accumulation gives inf and 0 here."""
    vals = [torch.full((n,), value) for n in (4097, 9)]
    out = K.grad_norm([place(v) for v in vals], 1.0).cpu()
    ref = host_norm(vals)
    print(value, "norm", out[0].item(), "host fp64", ref)
    assert math.isfinite(ref) and ref > 0 and ulps(out[0].item(), ref) <= 1


def test_norm_over_more_chunks_than_one_round_of_the_finish():
    """2051 + 1 chunks: the finish kernel's eight-loads-at-a-time loop (2048 partials a round) and its
    tail, which the size lists above (at most 12 chunks) never reach; aligned and + 4 B give the same bits."""
    vals = grad_values((2050 * 4096 + 3, 5), seed=6)
    assert sum(v.numel() for v in vals) <= 2 ** 24          # the 1-ulp derivation's n
    a = K.grad_norm([place(v) for v in vals], 1.0)
    b = K.grad_norm([place(v, mis=True) for v in vals], 1.0)
    ref = host_norm(vals)
    print("norm", a[0].item(), "host fp64", ref)
    assert ulps(a[0].item(), ref) <= 1 and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------- 2. bitwise properties
@pytest.mark.parametrize("name", list(SIZES))
def test_norm_bits_do_not_depend_on_alignment_or_call(name):
    vals = grad_values(SIZES[name], seed=1)
    a = K.grad_norm([place(v) for v in vals], 0.5)
    b = K.grad_norm([place(v, mis=True) for v in vals], 0.5)
    c = K.grad_norm([place(v, mis=i % 2 == 0) for i, v in enumerate(vals)], 0.5)
    grads = [place(v) for v in vals]
    d, e = K.grad_norm(grads, 0.5), K.grad_norm(grads, 0.5)
    for other in (b, c, d, e):
        assert torch.equal(bits(a), bits(other)), (a.cpu(), other.cpu())


@pytest.mark.parametrize("name", list(SIZES))
def test_norm_bits_in_a_grad_buffer_and_loose(name):
    vals = grad_values(SIZES[name], seed=2)
    buf = dp.GradBuffer(vals, DEV)
    for view, v in zip(buf.views, vals):
        view.copy_(v)
    a = K.grad_norm(buf.views, 0.5)
    b = K.grad_norm([place(v) for v in vals], 0.5)
    assert torch.equal(bits(a), bits(b)), (a.cpu(), b.cpu())


# ----------------------------------------------------------------------------------- 3. coefficient
def test_coefficient_is_torchs_expression():
    """out[1] against clip_grad_norm_'s expression in fp32 on the returned out[0], bit for bit.  The
    expression is evaluated as a division of fp32 tensors, as the kernel divides; Python's
    `float / tensor` is reciprocal() * float in torch, two roundings, and stays within 2 ulps of it."""
    vals = grad_values(SIZES["sizes"], seed=3)
    grads = [place(v) for v in vals]
    norm = K.grad_norm(grads, 1.0).cpu()[0]
    for max_norm in (1e-3 * norm.item(), 0.37 * norm.item(), norm.item(), 1e3 * norm.item(), float("inf")):
        out = K.grad_norm(grads, max_norm).cpu()
        assert torch.equal(bits(out[0]), bits(norm))
        want = torch_coef(out[0], max_norm)
        print("max_norm", max_norm, "coef", out[1].item(), "torch", want.item())
        assert torch.equal(bits(out[1]), bits(want)), (max_norm, out[1].item(), want.item())
        assert ulps(out[1].item(), torch.clamp(max_norm / (out[0] + 1e-6), max=1.0).item()) <= 2
        if max_norm > 1.5 * norm.item():
            assert out[1].item() == 1.0
        if max_norm < 0.5 * norm.item():
            assert out[1].item() < 0.5
    # max_norm == norm: just under 1 (the 1e-6), never above
    assert 0.999 < K.grad_norm(grads, norm.item()).cpu()[1].item() <= 1.0


@pytest.mark.parametrize("bad,want", [(float("inf"), (float("inf"), 0.0)), (float("nan"), None)])
def test_coefficient_of_non_finite_gradients(bad, want):
    vals = grad_values(SIZES["sizes"], seed=4)
    vals[4][4000] = bad
    out = K.grad_norm([place(v) for v in vals], 1.0).cpu()
    if want is None:
        assert math.isnan(out[0].item()) and math.isnan(out[1].item())       # as torch: nothing is skipped
    else:
        assert tuple(out.tolist()) == want


# ---------------------------------------------------------------------------------- 4. clipped Adam
HP = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_scalars(step, wd):
    bc1, bc2 = 1 - HP["b1"] ** step, 1 - HP["b2"] ** step
    return HP["b1"], HP["b2"], HP["eps"], wd, HP["lr"] / bc1, math.sqrt(bc2)


ADAM_CASES = [(n, None) for n in SIZES if n != "g + 4 B"] + [("g + 4 B", f) for f in "pgmv"]


@pytest.mark.parametrize("name,mis_field", ADAM_CASES, ids=["%s%s" % (n, " (%s + 4 B)" % f if f else "") for n, f in ADAM_CASES])
def test_clipped_adam_is_adam_on_the_scaled_gradient(name, mis_field):
    """pu_adam_multi_clipped with coefficient c == g.mul_(c) on a copy, then pu_adam_multi, in every bit
    of p, m and v; with c == 1 it is pu_adam_multi on the untouched gradients; g is never written."""
    numels = SIZES[name]
    gen = torch.Generator().manual_seed(5)
    v0 = {f: [torch.randn(n, generator=gen) for n in numels] for f in "pgm"}
    v0["v"] = [torch.rand(n, generator=gen) * 1e-2 for n in numels]

    def tensors():
        return {f: [place(t, mis_field == f and i == 0) for i, t in enumerate(v0[f])] for f in "pgmv"}

    for wd in (0.0, 0.01):
        for step in (1, 1000):
            for c in (0.37, 1.0):
                sc = adam_scalars(step, wd)
                scale = torch.tensor([c], dtype=torch.float32, device=DEV)
                a, b = tensors(), tensors()
                if c != 1.0:
                    for g in a["g"]:
                        g.mul_(scale)           # one fp32 rounding per element, the gradient rewritten
                K.adam_multi(a["p"], a["g"], a["m"], a["v"], *sc)
                K.adam_multi(b["p"], b["g"], b["m"], b["v"], *sc, grad_scale=scale)
                for f in "pmv":
                    for i, (x, y) in enumerate(zip(a[f], b[f])):
                        assert torch.equal(bits(x), bits(y)), (f, i, wd, step, c)
                for i, g in enumerate(b["g"]):
                    assert torch.equal(g.cpu(), v0["g"][i]), (i, wd, step, c)
                assert any(not torch.equal(x.cpu(), y) for x, y in zip(b["p"], v0["p"]) if y.numel())


# ----------------------------------------------------------------------------- 5. Trainer end to end
E2E = dict(depth=3, base_ch=8, nbf=32, batch=2, steps=4, lr=1e-3, max_norm=0.003, scales=(1.0, 1.0, 40.0, 1.0))


def e2e_data():
    """Step 2's input is 40 times the others': its gradient norm stands out, the clipping coefficient
    varies from step to step - the only way clipping shows through Adam's scale invariance."""
    g = torch.Generator().manual_seed(17)
    B, N = E2E["batch"], E2E["nbf"]
    xs = [s * torch.rand(B, 1, N, N, generator=g) for s in E2E["scales"]]
    ts = [(torch.rand(B, N, N, generator=g) > 0.5).float() for _ in E2E["scales"]]
    return xs, ts


def e2e_init():
    torch.manual_seed(3)
    ref = oracle.RefUNetp(1, 1, rule="oja", nbf=E2E["nbf"], depth=E2E["depth"], base_ch=E2E["base_ch"])
    return {k: v.detach().clone() for k, v in ref.state_dict().items()}


def e2e_oracle(dtype, max_norm):
    """oracle.RefUNetp with clip_grad_norm_ (or none) and torch.optim.Adam -> losses, norms, trace, parameters"""
    net = oracle.RefUNetp(1, 1, rule="oja", nbf=E2E["nbf"], depth=E2E["depth"], base_ch=E2E["base_ch"])
    net.load_state_dict(e2e_init())
    net = net.to(dtype)
    opt = torch.optim.Adam(net.parameters(), lr=E2E["lr"])
    xs, ts = e2e_data()
    hebb = net.initialZeroHebb(E2E["batch"]).to(dtype)
    losses, norms = [], []
    for x, t in zip(xs, ts):
        opt.zero_grad()
        y, hn = net(x.to(dtype), hebb.detach())
        loss = oracle.bce_loss(y, t.to(dtype))
        loss.backward()
        params = [p for p in net.parameters() if p.grad is not None]
        if max_norm is None:
            norms.append(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)).item())
        else:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).item())
        opt.step()
        hebb = hn.detach()
        losses.append(loss.item())
    return losses, norms, hebb, {k: v.detach().clone() for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def e2e_refs():
    return (e2e_oracle(torch.float64, E2E["max_norm"]), e2e_oracle(torch.float32, E2E["max_norm"]),
            e2e_oracle(torch.float64, None))


def rel(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip graph"])
def test_trainer_clipped_trajectory_against_fp64(graph):
    """4 clipped steps of Trainer against the fp64 oracle with clip_grad_norm_ and torch's Adam, under
    the bars of test_model_gpu.py's 3-step Adam trajectory: losses within 1e-4, and every parameter's
    and the trace's deviation from the fp64 run at most 4 x the CPU fp32 oracle's own + 2e-7 (rel L2);
    the per-step norms within that file's gradient bar, 2e-4.  graph: steps 3 and 4 replay the
    captured step and the optimiser runs after the replay.  The unclipped fp64 trajectory lies more
    than 10 parameter bars away, so a clipping that does nothing cannot pass."""
    (l64, n64, h64, sd64), (_, _, h32, sd32), (_, n_free, _, sd_free) = e2e_refs()
    m = E2E["max_norm"]
    print("oracle norms", n64, "unclipped run", n_free)
    assert min(n64) < m < max(n64)            # some steps clipped, some not
    net = UNetp(1, 1, DEV, rule="oja", nbf=E2E["nbf"], depth=E2E["depth"], base_ch=E2E["base_ch"])
    net.load_state_dict(e2e_init())
    tr = Trainer(net, lr=E2E["lr"], steplr=1e5, max_grad_norm=m, graph=graph)
    xs, ts = e2e_data()
    hebb = net.initialZeroHebb(E2E["batch"])
    losses, norms, coefs = [], [], []
    for x, t in zip(xs, ts):
        loss, hebb = tr.step(x.to(DEV), t.to(DEV), hebb)
        losses.append(loss)
        norms.append(tr.last_grad_norm)
        coefs.append(tr.opt.clip_coef)
    assert (tr._graph is not None) == graph
    losses, norms, coefs = (torch.stack(v).cpu().tolist() for v in (losses, norms, coefs))
    print("losses", losses, l64, "\nnorms", norms, "\ncoefs", coefs)
    np.testing.assert_allclose(losses, l64, rtol=1e-4)
    np.testing.assert_allclose(norms, n64, rtol=2e-4)
    for n, c in zip(norms, coefs):
        assert c == torch_coef(torch.tensor(n, dtype=torch.float32), m).item()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    bars = {k: 4 * rel(sd32[k], sd64[k]) + 2e-7 for k in sd64}
    errs = {k: rel(sd[k], sd64[k]) for k in sd64}
    far = {k: rel(sd_free[k], sd64[k]) for k in sd64}
    for k in sd64:
        print("%-32s gpu-fp64 %.2e  bar %.2e  unclipped-fp64 %.2e" % (k, errs[k], bars[k], far[k]))
    assert any(far[k] > 10 * bars[k] for k in sd64)
    assert rel(hebb.cpu(), h64) <= 4 * rel(h32, h64) + 2e-7
    for k in sd64:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])


# --------------------------------------------------------------------------------------- 6. episode
def test_episode_norm_includes_eta():
    torch.manual_seed(3)
    N, B, steps = 16, 2, 3
    net = UNetp(1, 1, DEV, rule="oja", nbf=N, depth=3, base_ch=8, trace_grad=True)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        net.alpha.copy_(0.5 * torch.rand(net.alpha.shape, generator=g))
        net.eta.fill_(0.1)
    xs = torch.rand(steps, B, 1, N, N, generator=g).to(DEV)
    ts = (torch.rand(steps, B, N, N, generator=g) > 0.5).float().to(DEV)
    H0 = (0.2 * torch.randn(B, N, N, generator=g)).to(DEV)
    tr = Trainer(net, lr=1e-3, steplr=100, max_grad_norm=1e-3)
    tr.step_episode(xs, ts, H0)
    assert net.eta.grad is not None and net.eta.grad.abs().item() > 0
    grads = [p.grad.detach().cpu() for p in net.parameters()]
    assert all(gr is not None for gr in grads)
    ref = host_norm(grads)
    without_eta = host_norm([p.grad.detach().cpu() for p in net.parameters() if p is not net.eta])
    got = tr.last_grad_norm.item()
    print("episode norm", got, "host fp64", ref, "without eta", without_eta, "coef", tr.opt.clip_coef.item())
    assert ulps(got, ref) <= 1
    assert ulps(ref, without_eta) > 1       # eta's share is visible at this bar
    assert tr.opt.clip_coef.item() == torch_coef(tr.last_grad_norm.cpu(), 1e-3).item()


# -------------------------------------------------------------------------------------------- 7. DP
def _dp_clip_run(lo, hi, dev, max_norm):
    """2 clipped Trainer steps of test_dp_gpu.py's UNetpRes on slots [lo, hi) of its global batch,
    the Dropout2d masks being rows [lo, hi) of the single process's"""
    import test_dp_gpu as D
    torch.manual_seed(0)
    net = D._dp_net("res", dev)
    net.train()
    dp.broadcast_params(net)
    tr = Trainer(net, lr=1e-3, steplr=1e5, bucket_mb=0.05, max_grad_norm=max_norm)
    state = {"step": 0}
    net._trunk_plan().mask_fn = lambda name, B, C, p: D._global_mask(state["step"], name, C, p)[lo:hi].contiguous().to(dev)
    xs, ts = D._dp_data()
    hebb = net.initialZeroHebb(hi - lo)
    out = {"loss": [], "norm": [], "coef": [], "grads0": None}
    for s in range(D.STEPS):
        state["step"] = s
        loss, hebb = tr.step(xs[s][lo:hi].to(dev), ts[s][lo:hi].to(dev), hebb)
        out["loss"].append(loss.item())
        out["norm"].append(tr.last_grad_norm.cpu())
        out["coef"].append(tr.opt.clip_coef.cpu())
        if s == 0:
            out["grads0"] = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if p.grad is not None}
    out["hebb"] = hebb.cpu()
    out["params"] = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    return out


def _dp_clip_worker(rank, world, port, out_dir, max_norm):
    import sys
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_dp_gpu as D
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    lo, hi = rank * D.DP_B // world, (rank + 1) * D.DP_B // world
    out = _dp_clip_run(lo, hi, torch.device("cuda", 0), max_norm)
    torch.save(out, os.path.join(out_dir, "clip%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_identical_bits(tmp_path, gpu_device):
    """World 2 over gloo on one GPU: the norm is taken after the all-reduce, so both ranks hold the
    same gradients and must hold the same bits of norm, coefficient and parameters after 2 steps;
    against one process on the global batch the tolerances are those of test_dp_gpu._check_dp for this
    net (loss 1e-5, gradient and everything derived from it 1e-4 rel L2, trace rtol 1e-3 / atol 1e-5)."""
    import test_dp_gpu as D
    glob = _dp_clip_run(0, D.DP_B, gpu_device, float("inf"))
    max_norm = 0.5 * min(n.item() for n in glob["norm"])          # every step clipped
    glob = _dp_clip_run(0, D.DP_B, gpu_device, max_norm)
    mp.spawn(_dp_clip_worker, args=(2, D._free_port(), str(tmp_path), max_norm), nprocs=2, join=True)
    res = [torch.load(os.path.join(tmp_path, "clip%d.pt" % r), weights_only=True) for r in range(2)]
    for s in range(D.STEPS):
        assert torch.equal(bits(res[0]["norm"][s]), bits(res[1]["norm"][s]))
        assert torch.equal(bits(res[0]["coef"][s]), bits(res[1]["coef"][s]))
        assert res[0]["coef"][s].item() < 1.0
    for n, p in res[0]["params"].items():
        assert torch.equal(bits(p), bits(res[1]["params"][n])), n
    loss_tol, grad_tol = 1e-5, 1e-4
    for s in range(D.STEPS):
        mean_loss = sum(r["loss"][s] for r in res) / 2
        assert abs(mean_loss - glob["loss"][s]) < loss_tol * abs(glob["loss"][s]), (s, mean_loss, glob["loss"][s])
        print("step", s, "norm", res[0]["norm"][s].item(), glob["norm"][s].item(), "coef", res[0]["coef"][s].item(),
              glob["coef"][s].item())
        assert abs(res[0]["norm"][s].item() - glob["norm"][s].item()) < grad_tol * glob["norm"][s].item()
        assert abs(res[0]["coef"][s].item() - glob["coef"][s].item()) < grad_tol * glob["coef"][s].item()
    num = sum(((res[0]["grads0"][n] - g) ** 2).sum().item() for n, g in glob["grads0"].items())
    den = sum((g ** 2).sum().item() for g in glob["grads0"].values())
    assert (num / den) ** 0.5 < grad_tol, (num / den) ** 0.5
    num = sum(((res[0]["params"][n] - p) ** 2).sum().item() for n, p in glob["params"].items())
    den = sum((p ** 2).sum().item() for p in glob["params"].values())
    print("parameters, rel L2 to the global-batch run", (num / den) ** 0.5)
    assert (num / den) ** 0.5 < grad_tol, (num / den) ** 0.5
    torch.testing.assert_close(torch.cat([r["hebb"] for r in res]), glob["hebb"], rtol=1e-3, atol=1e-5)


# -------------------------------------------------------------------------------- train.py's log keys
def test_train_logs_the_norms_only_with_clip_grad(tmp_path):
    """train.train() over 2 steps of 2 slots at 32x32: with clip_grad the saved log holds one norm per
    step under train/grad_norms; without it the keys are those of before."""
    import train
    g = np.random.RandomState(5)
    X = g.rand(4, 1, 32, 32).astype(np.float32)
    Y = (g.rand(4, 1, 32, 32) > 0.5).astype(np.float32)
    keys = {}
    for clip in (0.0, 1e-3):
        torch.manual_seed(4)
        net = UNetp(1, 1, DEV, rule="oja", nbf=32, depth=3, base_ch=8)
        out = tmp_path / ("clip%g" % clip)
        out.mkdir()
        params = {"out_dir": str(out), "device": DEV, "epochs": 1, "stop_time": -1, "lr": 3e-4, "val_every": 100,
                  "save_every": 100, "rollout": 50000, "gamma": 0.666, "steplr": 4, "debug": False, "batch_size": 2,
                  "clip_grad": clip}
        train.train(net, X, X[:2], Y, Y[:2], params)
        with np.load(out / "train_data.npz") as z:
            keys[clip] = set(z.files)
            if clip:
                norms = z["train/grad_norms"]
                assert norms.shape == (2,) and np.all(np.isfinite(norms)) and np.all(norms > 0)
    assert keys[1e-3] - keys[0.0] == {"train/grad_norms"} and keys[0.0] <= keys[1e-3]
    assert keys[0.0] == {"net/w", "net/alpha", "net/eta", "train/all_losses", "validation/train_losses",
                         "validation/test_losses", "validation/accuracies"}
