"""Backpropagation through the plastic trace (trace_grad=True) on the GPU.

Kernel level: pu_plastic_bwd_trace through PlasticHeadFunction / FusedHeadFunction against
oracle.plastic_head left un-detached under autograd, in fp64, next to the CPU fp32 run of the same
graph (the bar of test_precision_gpu.py: error <= max(16 x the CPU fp32 error, 4e-6) of max|ref|).
Model level: episodes of K samples with the trace carried live against the fp64 RefUNetp, the
Trainer's step_episode, the eta update, UNetpRes and a two-rank episode.

The parameters are raised (alpha = 0.5 rand, eta = 0.1): at the default initialisation the trace
path is about 1e-4 of the gradient and every check here would pass with the path missing.  Each
kernel case asserts that itself (the guard): the fp64 gradients with and without the trace path
differ by at least 100 x the tolerance."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from punet import kernels as K  # noqa: E402
from punet.head import PlasticHeadFunction, FusedHeadFunction, RULES, bce_loss  # noqa: E402
from unet import UNetp, UNetpRes  # noqa: E402

DEV = torch.device("cuda")
FACTOR, FLOOR = 16.0, 4e-6          # tests/test_precision_gpu.py report()
SHAPES = [(1, 16), (3, 16), (3, 18), (2, 20), (3, 48), (1, 80), (512, 16)]


def head_inputs(B, N, seed=0):
    g = torch.Generator().manual_seed(1000 * B + N + seed)
    d = {"X": torch.randn(B, N, N, generator=g), "H": 0.2 * torch.randn(B, N, N, generator=g),
         "P": torch.randn(B, N, N, generator=g), "dY": torch.randn(B, N, N, generator=g),
         "w": 0.01 * torch.randn(N, N, generator=g), "alpha": 0.5 * torch.rand(N, N, generator=g),
         "eta": torch.tensor([0.1])}
    return d


def oracle_grads(d, rule, dtype, with_p=True, with_dy=True):
    """(dX, dw, dalpha, dH, deta) of sum(dY Y) + sum(P H') through oracle.plastic_head, H' live."""
    leaves = [d[k].to(dtype).clone().requires_grad_(True) for k in ("X", "w", "alpha", "H", "eta")]
    X, w, al, H, eta = leaves
    Y, Hn = oracle.plastic_head(X, H, w, al, eta, rule)
    obj = 0.0
    if with_dy:
        obj = obj + (Y * d["dY"].to(dtype)).sum()
    if with_p:
        obj = obj + (Hn * d["P"].to(dtype)).sum()
    gr = torch.autograd.grad(obj, leaves, allow_unused=True)
    return [torch.zeros_like(l) if g_ is None else g_ for g_, l in zip(gr, leaves)]


def gpu_grads(d, rule, with_p=True, with_dy=True, want_h=True, trace_grad=True):
    X = d["X"].to(DEV).requires_grad_(True)
    w, al = d["w"].to(DEV).requires_grad_(True), d["alpha"].to(DEV).requires_grad_(True)
    H = d["H"].to(DEV).requires_grad_(want_h)
    eta = d["eta"].to(DEV).requires_grad_(True)
    Y, Hn = PlasticHeadFunction.apply(X, H, w, al, eta, RULES[rule], True, None, trace_grad)
    outs, gos = [], []
    if with_dy:
        outs.append(Y), gos.append(d["dY"].to(DEV))
    if with_p:
        outs.append(Hn), gos.append(d["P"].to(DEV))
    ins = [X, w, al] + ([H] if want_h else []) + [eta]
    gr = list(torch.autograd.grad(outs, ins, gos, allow_unused=True))
    if not want_h:
        gr.insert(3, None)
    return gr


def rel_err(a, ref):
    return (a.detach().double().cpu() - ref.double()).abs().max().item() / ref.double().abs().max().item()


NAMES = ("dX", "dw", "dalpha", "dH", "deta")


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_trace_backward_against_fp64(B, N, rule):
    d = head_inputs(B, N)
    r64 = oracle_grads(d, rule, torch.float64)
    r32 = oracle_grads(d, rule, torch.float32)
    cut = oracle_grads(d, rule, torch.float64, with_p=False)
    got = gpu_grads(d, rule)
    fails = []
    for name, g_, c32, ref, nop in zip(NAMES, got, r32, r64, cut):
        eg, ec = rel_err(g_, ref), rel_err(c32, ref)
        tol = max(FACTOR * ec, FLOOR)
        gap = (nop - ref).abs().max().item() / ref.abs().max().item()
        print("%-7s gpu %.2e  cpu32 %.2e  tol %.2e  trace path %.2e" % (name, eg, ec, tol, gap))
        if name in ("dX", "dw", "dalpha"):
            assert gap >= 100 * tol, ("guard: the trace path is too small to be tested", name, gap, tol)
        if eg > tol:
            fails.append((name, eg, ec))
    assert not fails, fails


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("B,N", [(3, 18), (3, 48)])
def test_trace_backward_without_dy_and_without_dh(B, N, rule):
    d = head_inputs(B, N, seed=1)
    r64 = oracle_grads(d, rule, torch.float64, with_dy=False)
    r32 = oracle_grads(d, rule, torch.float32, with_dy=False)
    got = gpu_grads(d, rule, with_dy=False)
    for name, g_, c32, ref in zip(NAMES, got, r32, r64):
        assert rel_err(g_, ref) <= max(FACTOR * rel_err(c32, ref), FLOOR), name
    # dH not requested: the other four are the same bits, and nothing comes back for H
    full = gpu_grads(d, rule)
    noh = gpu_grads(d, rule, want_h=False)
    assert noh[3] is None
    for i in (0, 1, 2, 4):
        assert torch.equal(full[i], noh[i]), NAMES[i]


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("B,N", [(3, 18), (3, 48), (512, 16)])
def test_trace_backward_is_deterministic(B, N, rule):
    d = head_inputs(B, N, seed=2)
    a, b = gpu_grads(d, rule), gpu_grads(d, rule)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("B,N", [(3, 18), (3, 48), (512, 16)])
def test_no_trace_gradient_is_bitwise_the_detached_backward(B, N, rule):
    """trace_grad on, nothing arriving for H' (the last step of an episode): dX, dw, dalpha are
    bitwise those of the detached node, with and without a gradient wanted for H, and eta gets none."""
    d = head_inputs(B, N, seed=3)
    off = gpu_grads(d, rule, with_p=False, want_h=False, trace_grad=False)
    on = gpu_grads(d, rule, with_p=False, want_h=False)
    onh = gpu_grads(d, rule, with_p=False, want_h=True)
    for i in (0, 1, 2):
        assert torch.equal(off[i], on[i]) and torch.equal(off[i], onh[i]), NAMES[i]
    assert off[4] is None and on[4] is None and onh[4] is None
    ref = oracle_grads(d, rule, torch.float64, with_p=False)[3]
    c32 = oracle_grads(d, rule, torch.float32, with_p=False)[3]
    assert rel_err(onh[3], ref) <= max(FACTOR * rel_err(c32, ref), FLOOR)


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("B,N", [(2, 16), (2, 48)])
def test_fused_head_equals_outconv_then_head_with_trace_grad(B, N, rule):
    C = 8
    d = head_inputs(B, N, seed=4)
    g = torch.Generator().manual_seed(N)
    feat0 = torch.randn(B, N, N, C, generator=g).relu().to(DEV)
    wo0 = (0.3 * torch.randn(1, C, 1, 1, generator=g)).to(DEV)
    bo0 = torch.randn(1, generator=g).to(DEV)
    P, dY = d["P"].to(DEV), d["dY"].to(DEV)

    def leaves():
        return (d["H"].to(DEV).requires_grad_(True), d["w"].to(DEV).requires_grad_(True),
                d["alpha"].to(DEV).requires_grad_(True), d["eta"].to(DEV).requires_grad_(True))

    feat, wo, bo = feat0.clone().requires_grad_(True), wo0.clone().requires_grad_(True), bo0.clone().requires_grad_(True)
    H, w, al, eta = leaves()
    Y, Hn = FusedHeadFunction.apply(feat, wo, bo, H, w, al, eta, RULES[rule], True, None, True)
    fused = torch.autograd.grad((Y, Hn), (feat, wo, bo, H, w, al, eta), (dY, P))

    H, w, al, eta = leaves()
    X = K.outconv_fwd(feat0, wo0.reshape(-1), bo0).requires_grad_(True)
    Y2, Hn2 = PlasticHeadFunction.apply(X, H, w, al, eta, RULES[rule], True, None, True)
    dX, dH, dw, da, deta = torch.autograd.grad((Y2, Hn2), (X, H, w, al, eta), (dY, P))
    dfeat, dwo, dbo = K.outconv_bwd(feat0, wo0.reshape(-1), dX.contiguous(), relu_mask=True)
    assert torch.equal(Y, Y2) and torch.equal(Hn, Hn2)
    for name, a, b in zip(("dfeat", "dwo", "dbo", "dH", "dw", "dalpha", "deta"), fused,
                          (dfeat, dwo.view(1, C, 1, 1), dbo, dH, dw, da, deta)):
        assert torch.equal(a, b), name


class _Ctx:
    """Stand-in for a detached node's ctx: with the switch off H' is marked non-differentiable, so
    autograd never hands its backward a gradient for it; the guard is reached only directly."""
    trace_grad = False
    needs_input_grad = (True,) * 11


def test_switch_off_keeps_the_error_and_eta_without_gradient():
    from punet.head import SequentialHeadFunction
    torch.manual_seed(0)
    net = UNetp(1, 1, DEV, rule="oja", nbf=32, depth=3, base_ch=8)
    assert net.trace_grad is False and "trace_grad" not in net.state_dict()
    x = torch.rand(2, 1, 32, 32, device=DEV)
    t = (torch.rand(2, 32, 32, device=DEV) > 0.5).float()
    y, hn = net(x, net.initialZeroHebb(2).requires_grad_(True))
    assert not hn.requires_grad
    bce_loss(y, t).backward()
    assert net.eta.grad is None and net.w.grad is not None
    g = torch.zeros(2, 32, 32, device=DEV)
    for fn in (PlasticHeadFunction, FusedHeadFunction):
        with pytest.raises(RuntimeError, match="backpropagation through the updated plastic trace is not supported"):
            fn.backward(_Ctx(), g, g)
    with pytest.raises(RuntimeError, match="trace gradients .* need hebb_mode='slots'"):
        SequentialHeadFunction.backward(_Ctx(), g, g)


# ------------------------------------------------------------------------------------- model level
def raise_plasticity(net, seed=7):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.alpha.copy_(0.5 * torch.rand(net.alpha.shape, generator=g))
        net.eta.fill_(0.1)
    return net


def episode_data(K_, B, N, seed=11):
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(K_, B, 1, N, N, generator=g)
    ts = (torch.rand(K_, B, N, N, generator=g) > 0.5).float()
    H0 = 0.2 * torch.randn(B, N, N, generator=g)
    return xs, ts, H0


def ref_episode(ref, xs, ts, H0):
    """fp64 oracle, trace live over the episode: (losses [K], H_K, {name: grad})."""
    ref.zero_grad(set_to_none=True)
    h = H0.double()
    losses = []
    for k in range(xs.shape[0]):
        y, h = ref(xs[k].double(), h)
        losses.append(oracle.bce_loss(y, ts[k].double()))
    (torch.stack(losses).sum() / len(losses)).backward()
    return torch.stack(losses).detach(), h.detach(), {k: p.grad for k, p in ref.named_parameters()}


def gpu_episode(net, xs, ts, H0):
    for p in net.parameters():
        p.grad = None
    h = H0.to(DEV)
    losses = []
    for k in range(xs.shape[0]):
        y, h = net(xs[k].to(DEV), h)
        losses.append(bce_loss(y, ts[k].to(DEV)))
    (torch.stack(losses).sum() / len(losses)).backward()
    return torch.stack(losses).detach(), h.detach()


def check_against(net, grads_ref, losses, losses_ref):
    assert ((losses.double().cpu() - losses_ref).abs() / losses_ref.abs()).max().item() <= 1e-4
    num = den = 0.0
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        r = grads_ref[k]
        dd = (p.grad.double().cpu() - r).norm().item()
        num, den = num + dd * dd, den + r.norm().item() ** 2
        assert dd <= 2e-3 * max(r.norm().item(), 1e-30), (k, dd, r.norm().item())
    assert (num / den) ** 0.5 <= 1e-4, (num / den) ** 0.5


def make_pair(rule, nbf, seed=3):
    torch.manual_seed(seed)
    net = raise_plasticity(UNetp(1, 1, DEV, rule=rule, nbf=nbf, depth=3, base_ch=8, trace_grad=True))
    ref = oracle.RefUNetp(1, 1, rule=rule, nbf=nbf, depth=3, base_ch=8).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return net, ref


@pytest.mark.parametrize("rule,nbf", [("hebb", 16), ("oja", 32)])
def test_episode_gradients_against_fp64_and_trainer(rule, nbf):
    """K = 3, B = 2: plain autograd over the episode vs the fp64 oracle (eta included); then the
    same net through Trainer.step_episode with the flat gradient buffer on - its gradients are
    those of the plain run (K nodes writing one buffer view would sum aliased tensors), and eta
    moves by what an fp64 Adam makes of the oracle's gradient."""
    from punet.engine import Trainer
    net, ref = make_pair(rule, nbf)
    xs, ts, H0 = episode_data(3, 2, nbf)
    losses_ref, h_ref, grads_ref = ref_episode(ref, xs, ts, H0)
    # the trace path matters here: the same episode with the trace cut gives other gradients
    losses, hK = gpu_episode(net, xs, ts, H0)
    check_against(net, grads_ref, losses, losses_ref)
    assert (hK.double().cpu() - h_ref).abs().max().item() <= 1e-4 * h_ref.abs().max().item()
    plain = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    before = {k: p.detach().clone() for k, p in net.named_parameters()}

    lr = 1e-3
    tr = Trainer(net, lr=lr, steplr=100)
    assert tr.gradbuf is not None
    l2, h2 = tr.step_episode(xs.to(DEV), ts.to(DEV), H0.to(DEV))
    assert torch.equal(l2, losses) and torch.equal(h2, hK) and not h2.requires_grad
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, plain[k]), k
    # first Adam step from zero moments, fp64, on the oracle's gradient of eta
    gr = grads_ref["eta"]
    m, v = 0.1 * gr, 0.001 * gr * gr
    upd = lr * (m / 0.1) / ((v / 0.001).sqrt() + 1e-8)
    got = (before["eta"].double() - net.eta.detach().double()).cpu()
    assert (got - upd).abs().max().item() <= 1e-6 * upd.abs().max().item() + 1.2e-7 * before["eta"].abs().max().item()
    assert net.eta.item() != before["eta"].item()


def test_trace_path_is_visible_at_model_level():
    """The oracle's own gradients with the trace cut between the samples differ from the live
    ones by far more than the bars above (so those bars test the path)."""
    net, ref = make_pair("oja", 16)
    xs, ts, H0 = episode_data(3, 2, 16)
    _, _, live = ref_episode(ref, xs, ts, H0)
    live = {k: v.clone() for k, v in live.items()}
    ref.zero_grad(set_to_none=True)
    h = H0.double()
    tot = 0.0
    for k in range(3):
        y, h = ref(xs[k].double(), h.detach())
        tot = tot + oracle.bce_loss(y, ts[k].double()) / 3
    tot.backward()
    assert ref.eta.grad is None
    d = sum((live[k] - p.grad).norm().item() ** 2 for k, p in ref.named_parameters() if k != "eta") ** 0.5
    n = sum(live[k].norm().item() ** 2 for k, _ in ref.named_parameters() if k != "eta") ** 0.5
    assert d / n >= 100 * 1e-4, d / n


def test_unetpres_episode_against_fp64():
    N = 32
    torch.manual_seed(5)
    net = raise_plasticity(UNetpRes(1, 1, DEV, neurons=4, nbf=N, trace_grad=True)).eval()
    ref = oracle.RefUNetpRes(1, 1, neurons=4, nbf=N).double().eval()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    xs, ts, H0 = episode_data(2, 2, N, seed=17)
    losses_ref, _, grads_ref = ref_episode(ref, xs, ts, H0)
    losses, _ = gpu_episode(net, xs, ts, H0)
    check_against(net, grads_ref, losses, losses_ref)


DP_B, DP_N, DP_K = 4, 16, 3


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from punet import dp
    from punet.engine import Trainer
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    net, _ = make_pair("oja", DP_N)
    dp.broadcast_params(net)
    tr = Trainer(net, lr=1e-3, steplr=100)
    assert tr.distributed and tr.reducer is not None
    xs, ts, H0 = episode_data(DP_K, DP_B, DP_N)
    lo, hi = rank * DP_B // world, (rank + 1) * DP_B // world
    losses, h = tr.step_episode(xs[:, lo:hi].to(DEV), ts[:, lo:hi].to(DEV), H0[lo:hi].to(DEV))
    torch.save({"grads": {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()},
                "losses": losses.cpu(), "hebb": h.cpu()}, os.path.join(out_dir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_episode_equals_global_batch(tmp_path):
    """Two gloo ranks on one GPU, each with half of the slots: after step_episode the averaged
    gradients (eta's included) are those of one process on the global batch, the same on both
    ranks, and the traces stay per rank."""
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    net, _ = make_pair("oja", DP_N)
    xs, ts, H0 = episode_data(DP_K, DP_B, DP_N)
    losses, hK = gpu_episode(net, xs, ts, H0)
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(os.path.join(tmp_path, "r%d.pt" % r), weights_only=True) for r in range(2)]
    for k, p in net.named_parameters():
        g_ = p.grad.cpu()
        assert torch.equal(res[0]["grads"][k], res[1]["grads"][k]), k
        torch.testing.assert_close(res[0]["grads"][k], g_, rtol=1e-4, atol=1e-5 * max(g_.abs().max().item(), 1e-30))
    assert res[0]["grads"]["eta"].abs().item() > 0
    mean = (res[0]["losses"] + res[1]["losses"]) / 2
    assert ((mean - losses.cpu()).abs() / losses.cpu().abs()).max().item() < 1e-5
    torch.testing.assert_close(torch.cat([r["hebb"] for r in res]), hK.cpu(), rtol=1e-4, atol=1e-6)
