"""End-to-end parity of the MI355X UNetp (plastic-unet_amd/unet) against the reference's golden
vectors and the CPU oracle, through the drop-in API: net(x, hebb) -> loss.backward() -> step()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from unet import UNetp  # noqa: E402  (the product mirror, plastic-unet_amd/unet)
from punet import FusedAdam, bce_loss  # noqa: E402
import oracle  # noqa: E402
from conftest import golden  # noqa: E402

DEV = torch.device("cuda")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def assert_close(got, ref, rtol=1e-4, atol_rel=1e-5):
    got = got.detach().float().cpu()
    ref = torch.as_tensor(ref).detach().float().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    torch.testing.assert_close(got, ref.reshape(got.shape), rtol=rtol, atol=atol_rel * scale)


def load_prefixed(net, g, prefix):
    net.load_state_dict({k[len(prefix):]: _t(v) for k, v in g.items() if k.startswith(prefix)})


def test_c8_reference_topology_fwd_bwd_golden():
    gi, g = golden("unetp_c8_init.npz"), golden("unetp_c8_step.npz")
    net = UNetp(1, 1, DEV, rule="oja", nbf=64)
    load_prefixed(net, gi, "p.")
    y, hn = net(_t(g["x"]).to(DEV), _t(g["hebb"]).to(DEV))
    assert y.shape == (64, 64) and hn.shape == (64, 64)
    loss = bce_loss(y, _t(g["t"]).to(DEV))
    loss.backward()
    assert_close(y, g["Y"])
    assert_close(hn, g["Hn"])
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    for k, p in net.named_parameters():
        if k == "eta":
            assert p.grad is None
            continue
        assert_close(p.grad, g["g." + k], rtol=2e-4, atol_rel=2e-5)


def _oracle_adam_run(gi, g, dtype):
    net = oracle.RefUNetp(1, 1, rule="oja", nbf=64)
    load_prefixed(net, gi, "p.")
    net = net.to(dtype)
    opt = oracle.ref_adam(net.parameters(), 1e-3)
    sch = oracle.ref_steplr(opt, 2)
    hebb = net.initialZeroHebb().to(dtype)
    losses = []
    for k in range(3):
        loss, _, hebb = oracle.ref_train_step(net, opt, sch, _t(g["xs"][k]).to(dtype), _t(g["ts"][k]).to(dtype), hebb)
        losses.append(loss.item())
    return losses, hebb, net.state_dict()


def test_c8_three_adam_steplr_steps_golden():
    """train.py's hot loop (bs=1, trace carried, Adam + per-sample StepLR) for 3 samples.

    Adam normalises every coordinate (m / sqrt(v)), so after the first step each parameter has
    moved by ~lr whatever its gradient's size and near-zero gradients move by +-lr on rounding
    alone.  The GPU trajectory is therefore judged against an fp64 oracle run: its deviation must
    be of the same size as the CPU fp32 reference's own deviation (the golden vectors)."""
    gi, g = golden("unetp_c8_init.npz"), golden("unetp_c8_adam.npz")
    net = UNetp(1, 1, DEV, rule="oja", nbf=64)
    load_prefixed(net, gi, "p.")
    opt = FusedAdam(net.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.StepLR(opt, gamma=0.666, step_size=2)
    hebb = net.initialZeroHebb()
    losses = []
    for k in range(3):
        opt.zero_grad()
        y, hebb = net(_t(g["xs"][k]).to(DEV), hebb.detach())
        loss = bce_loss(y.view(-1), _t(g["ts"][k]).to(DEV).view(-1))
        losses.append(loss.item())
        loss.backward()
        opt.step()
        sch.step()
    np.testing.assert_allclose(losses, g["losses"], rtol=1e-4)     # north_star: loss within 1e-4
    l64, h64, sd64 = _oracle_adam_run(gi, g, torch.float64)

    def rel(a, b):
        return (a.double() - b).norm().item() / max(b.norm().item(), 1e-30)

    errs = [("hebb", rel(hebb.cpu(), h64), rel(_t(g["hebb"]), h64))]
    sd = net.state_dict()
    for k in sd:
        errs.append((k, rel(sd[k].cpu(), sd64[k]), rel(_t(g["p." + k]), sd64[k])))
    for k, e_g, e_c in errs:
        print("%-36s gpu-fp64 %.2e   cpu32-fp64 %.2e (rel L2)" % (k, e_g, e_c))
    # The GPU's deviation from the fp64 run must be of the CPU fp32 reference's own size (measured:
    # within 1.5x for every tensor).  This bar caught two real defects that a looser one hid: packed
    # conv weights not refreshed after FusedAdam (1e-4 of the fp64 run) and 1-beta2 formed from an
    # fp32-rounded beta2 (1.3e-5 relative in v).
    for k, e_g, e_c in errs:
        assert e_g <= 4 * e_c + 2e-7, (k, e_g, e_c)
    agree, total = 0, 0
    for k in sd:
        if k == "eta":
            continue
        d_gpu = sd[k].cpu().double() - _t(gi["p." + k]).double()
        d_ref = _t(g["p." + k]).double() - _t(gi["p." + k]).double()
        big = d_ref.abs() > 1e-3          # coordinates the reference moved by more than lr
        agree += (torch.sign(d_gpu[big]) == torch.sign(d_ref[big])).sum().item()
        total += big.sum().item()
    assert agree >= 0.98 * total, (agree, total)


def test_depth4_base16_two_slots_golden():
    gi, g = golden("unetp_d4c16_bs2_init.npz"), golden("unetp_d4c16_bs2_out.npz")
    net = UNetp(1, 1, DEV, rule="hebb", nbf=128, depth=4, base_ch=16)
    load_prefixed(net, gi, "p.")
    y, hn = net(_t(g["x"]).to(DEV), _t(g["H"]).to(DEV))
    loss = bce_loss(y, _t(g["t"]).to(DEV))
    loss.backward()
    assert_close(y, g["Y"].reshape(2, 128, 128))
    assert_close(hn, g["Hn"])
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    for k, p in net.named_parameters():
        if k == "eta":
            continue
        assert_close(p.grad, g["g." + k], rtol=2e-4, atol_rel=2e-5)


def test_c64_widths_checksums_golden():
    g = golden("unetp_c64_sum.npz")
    ref = oracle.det_init_(oracle.RefUNetp(1, 1, rule="oja", nbf=32, depth=5, base_ch=64), 31)
    net = UNetp(1, 1, DEV, rule="oja", nbf=32, depth=5, base_ch=64)
    net.load_state_dict(ref.state_dict())
    y, hn = net(_t(g["x"]).to(DEV), _t(g["H"]).to(DEV))
    loss = bce_loss(y, _t(g["t"]).to(DEV))
    loss.backward()
    assert_close(y, g["Y"])
    assert_close(hn, g["Hn"])
    for k, p in net.named_parameters():
        if k == "eta":
            continue
        gg = p.grad.double().cpu()
        np.testing.assert_allclose([gg.abs().sum().item(), gg.norm().item()], g["gsum." + k][1:], rtol=2e-4)


def _c2_pair(B, seed=0):
    torch.manual_seed(seed)
    ref = oracle.RefUNetp(1, 1, rule="oja", nbf=128, depth=5, base_ch=64)
    net = UNetp(1, 1, DEV, rule="oja", nbf=128, depth=5, base_ch=64)
    net.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(B, 1, 128, 128, generator=g)
    t = (torch.rand(B, 128, 128, generator=g) > 0.5).float()
    H = 0.05 * torch.randn(B, 128, 128, generator=g)
    return ref, net, x, t, H


def test_c2_full_width_matches_oracle():
    """Config C2 widths (depth 5, base 64) at 128x128, two slots.

    Loss/logits within 1e-4 of the CPU fp32 oracle (north_star).  Gradients are judged against an
    fp64 run of the oracle: the GPU's error must be within a small factor of the CPU fp32 oracle's
    own error (deep-layer gradients of this freshly initialised net are ~1e-7 and cancel heavily,
    so a fixed relative tolerance would only measure summation order)."""
    ref, net, x, t, H = _c2_pair(2)
    y_r, h_r = ref(x, H)
    loss_r = oracle.bce_loss(y_r, t)
    loss_r.backward()
    ref64 = oracle.RefUNetp(1, 1, rule="oja", nbf=128, depth=5, base_ch=64).double()
    ref64.load_state_dict(ref.state_dict())
    y64, _ = ref64(x.double(), H.double())
    oracle.bce_loss(y64, t.double()).backward()
    y, h = net(x.to(DEV), H.to(DEV))
    loss = bce_loss(y, t.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4 * abs(loss_r.item())
    assert_close(y, y_r)
    assert_close(h, h_r)
    # masks bit-exact except pixels within 1e-5 of the 0.5 threshold
    near = (y_r - 0.5).abs() < 1e-5
    mask_k = (y.cpu() > 0.5)
    mask_r = (y_r > 0.5)
    assert torch.equal(mask_k[~near], mask_r[~near])
    # gradients: relative L2 error vs fp64 (robust to the isolated ReLU-branch flips any fp32
    # implementation shows near zero pre-activations; see tests/test_precision_gpu.py)
    for (k, p), (_, pr), (_, p64) in zip(net.named_parameters(), ref.named_parameters(), ref64.named_parameters()):
        if k == "eta":
            continue
        truth = p64.grad
        nrm = truth.norm().item()
        err_gpu = (p.grad.cpu().double() - truth).norm().item() / nrm
        err_cpu = (pr.grad.double() - truth).norm().item() / nrm
        print("%-36s |g| %.3e  gpu-fp64 %.1e  cpu32-fp64 %.1e (rel L2)" % (k, nrm, err_gpu, err_cpu))
        assert err_gpu <= max(16 * err_cpu, 1e-2), (k, err_gpu, err_cpu)


def test_c2_bs32_slots_independent_and_deterministic():
    """Full C2 batch: each slot's forward equals the slot run alone; two runs are bit-identical."""
    _, net, x, t, H = _c2_pair(32, seed=1)
    xd, Hd, td = x.to(DEV), H.to(DEV), t.to(DEV)
    with torch.no_grad():
        y, h = net(xd, Hd)
        y1, h1 = net(xd[5:6], Hd[5])
    torch.testing.assert_close(y[5].cpu(), y1.cpu(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(h[5].cpu(), h1.cpu(), rtol=1e-6, atol=1e-7)
    grads = []
    for _ in range(2):
        net.zero_grad()
        yy, _ = net(xd, Hd)
        bce_loss(yy, td).backward()
        grads.append([p.grad.clone() for p in net.parameters() if p.grad is not None])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert all(torch.isfinite(a).all() for a in grads[0])


def test_input_validation_matches_reference():
    net = UNetp(1, 1, DEV, rule="oja", nbf=32)
    with pytest.raises(ValueError, match="Only batch size: 1 is supported"):
        net(torch.zeros(2, 1, 32, 32, device=DEV), torch.zeros(32, 32, device=DEV))
    net.rule = "bogus"
    with pytest.raises(ValueError, match="Must select one learning rule"):
        net(torch.zeros(1, 1, 32, 32, device=DEV), torch.zeros(32, 32, device=DEV))


def test_fused_head_model_path_equals_unfused():
    """UNetp with the outconv fused into the head (default) vs the two-launch path: bitwise the
    same Y, H' and every gradient (the backward is the same kernels on bit-identical X)."""
    import punet.head as ph
    res = []
    for fuse in (True, False):
        ph.FUSE_OUTCONV = fuse
        try:
            torch.manual_seed(2)
            net = UNetp(1, 1, DEV, rule="oja", nbf=64, depth=4, base_ch=16)
            g = torch.Generator().manual_seed(6)
            x = torch.rand(3, 1, 64, 64, generator=g).to(DEV)
            t = (torch.rand(3, 64, 64, generator=g) > 0.5).float().to(DEV)
            H = (0.05 * torch.randn(3, 64, 64, generator=g)).to(DEV)
            y, hn = net(x, H)
            bce_loss(y, t).backward()
            res.append((y.detach(), hn.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()
                                                  if p.grad is not None}))
        finally:
            ph.FUSE_OUTCONV = True
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].keys() == res[1][2].keys()
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


def test_teacher_forced_trajectory_step_by_step():
    """The multi-step trajectory with the chaotic part removed: for 6 steps of the reference loop
    (bs=1, trace carried, Adam + per-sample StepLR, train.py:91-112) the oracle is re-seeded with
    the GPU's CURRENT parameters and trace at every step, so each step is judged on its own:
      * loss within 1e-4 relative (north star) and Y / H' within 1e-4 of the fp64 oracle;
      * the gradients at that point within 1e-4 aggregate relative L2 of fp64 (per tensor 2e-3:
        an fp32 pre-activation within noise of 0 may take the other ReLU branch);
      * the optimizer in isolation: FusedAdam's update of every parameter equals an fp64 Adam
        applied to the SAME fp32 gradient and moments to 1e-6 relative, and the learning rate
        follows StepLR exactly - a systematic optimizer bias cannot hide in trajectory noise."""
    gi, g = golden("unetp_c8_init.npz"), golden("unetp_c8_adam.npz")
    net = UNetp(1, 1, DEV, rule="oja", nbf=64)
    load_prefixed(net, gi, "p.")
    opt = FusedAdam(net.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.StepLR(opt, gamma=0.666, step_size=2)
    ref = oracle.RefUNetp(1, 1, rule="oja", nbf=64).double()
    hebb = net.initialZeroHebb()
    gen = torch.Generator().manual_seed(13)
    moments = {}
    b1, b2, eps = 0.9, 0.999, 1e-8
    for step in range(6):
        x = torch.rand(1, 1, 64, 64, generator=gen)
        t = (torch.rand(64, 64, generator=gen) > 0.5).float()
        ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
        ref.zero_grad(set_to_none=True)
        yr, hr = ref(x.double(), hebb.detach().cpu().double())
        lr_ = oracle.bce_loss(yr.reshape(-1), t.double().reshape(-1))
        lr_.backward()
        opt.zero_grad()
        y, hn = net(x.to(DEV), hebb.detach())
        loss = bce_loss(y.view(-1), t.to(DEV).view(-1))
        loss.backward()
        e_loss = abs(loss.item() - lr_.item()) / abs(lr_.item())
        e_y = ((y.double().cpu() - yr).abs().max() / yr.abs().max()).item()
        e_h = ((hn.double().cpu() - hr).abs().max() / max(hr.abs().max().item(), 1e-30)).item()
        print("step %d: loss %.3g  Y %.3g  H' %.3g" % (step, e_loss, e_y, e_h), flush=True)
        assert e_loss <= 1e-4, step
        assert e_y < 1e-4, step
        assert e_h < 1e-4, step
        num = den = 0.0
        for (k, p), (_, pr) in zip(net.named_parameters(), ref.named_parameters()):
            if k == "eta":
                assert p.grad is None and pr.grad is None
                continue
            d = (p.grad.double().cpu() - pr.grad).norm().item()
            num, den = num + d * d, den + pr.grad.norm().item() ** 2
            assert d <= 2e-3 * max(pr.grad.norm().item(), 1e-30), (step, k)
        assert (num / den) ** 0.5 <= 1e-4, (step, (num / den) ** 0.5)
        # the optimizer alone, on the GPU's own gradients
        lr_now = opt.param_groups[0]["lr"]
        assert lr_now == 1e-3 * 0.666 ** (step // 2)
        before = {k: p.detach().double().cpu().clone() for k, p in net.named_parameters()}
        grads = {k: p.grad.double().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
        opt.step()
        sch.step()
        for k, p in net.named_parameters():
            if k not in grads:
                assert torch.equal(p.detach().double().cpu(), before[k])     # eta: no grad, untouched (S3)
                continue
            m, v = moments.get(k, (torch.zeros_like(grads[k]), torch.zeros_like(grads[k])))
            m = b1 * m + (1 - b1) * grads[k]
            v = b2 * v + (1 - b2) * grads[k] ** 2
            moments[k] = (m, v)
            n = step + 1
            upd = lr_now * (m / (1 - b1 ** n)) / ((v / (1 - b2 ** n)).sqrt() + eps)
            got = before[k] - p.detach().double().cpu()
            scale = upd.abs().max().item()
            err = (got - upd).abs()
            i = int(err.argmax())
            assert err.max().item() <= 1e-6 * max(scale, 1e-30) + 2e-7 * before[k].abs().max().item(), (
                step, k, err.max().item(), scale, before[k].abs().max().item(), grads[k].reshape(-1)[i].item(),
                m.reshape(-1)[i].item(), v.reshape(-1)[i].item(), upd.reshape(-1)[i].item(), got.reshape(-1)[i].item())
        hebb = hn.detach()


def test_forward_after_optimizer_step_sees_new_weights():
    """FusedAdam writes parameters through raw pointers; the trunk caches packed / split GEMM
    operands keyed on the parameter's version counter.  After opt.step() the next forward must be
    bit-identical to a fresh model loaded with the updated state (no stale packed weights), and a
    DP broadcast must invalidate the same way."""
    torch.manual_seed(3)
    net = UNetp(1, 1, DEV, rule="oja", nbf=64)
    opt = FusedAdam(net.parameters(), lr=1e-2)
    x = torch.rand(1, 1, 64, 64, device=DEV)
    t = (torch.rand(64, 64, device=DEV) > 0.5).float()
    h0 = net.initialZeroHebb()
    y0, _ = net(x, h0)
    bce_loss(y0.view(-1), t.view(-1)).backward()
    opt.step()
    y1, h1 = net(x, h0)
    fresh = UNetp(1, 1, DEV, rule="oja", nbf=64)
    fresh.load_state_dict(net.state_dict())
    y2, h2 = fresh(x, h0)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, y2) and torch.equal(h1, h2)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c2_side_stream_weight_gradients_bitwise(precision):
    """PU_WSTREAM: the trunk's weight gradients run on a second stream beside the data-gradient
    chain (the default for bf16 trunks, C3).  Three Trainer steps at C2/C3 widths (bs 8) must match
    the one-stream run bit for bit - losses, every gradient and the updated parameters (a missing
    dependency or an allocator reuse race would show up as a difference)."""
    from punet import trunk
    from punet.engine import Trainer
    res = []
    for side in (False, True):
        trunk.set_side_stream(side)
        try:
            _, net, x, t, H = _c2_pair(8, seed=3)
            if precision == "bf16":
                sd = net.state_dict()
                net = UNetp(1, 1, DEV, rule="oja", nbf=128, depth=5, base_ch=64, precision="bf16")
                net.load_state_dict(sd)
            tr = Trainer(net, lr=1e-3, steplr=1e5)
            hebb = H.to(DEV)
            losses, grads = [], []
            for s in range(3):
                xs = torch.roll(x, shifts=s, dims=0).to(DEV)
                loss, hebb = tr.step(xs, t.to(DEV), hebb)
                losses.append(loss.item())
                grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
            torch.cuda.synchronize()
            res.append((losses, grads, {k: p.detach().clone() for k, p in net.named_parameters()}, hebb.clone()))
        finally:
            trunk.set_side_stream("bf16")
    assert res[0][0] == res[1][0]
    for s in range(3):
        assert res[0][1][s].keys() == res[1][1][s].keys()
        for k in res[0][1][s]:
            assert torch.equal(res[0][1][s][k], res[1][1][s][k]), (s, k)
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    assert torch.equal(res[0][3], res[1][3])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_step_bitwise_equals_eager(precision):
    """Trainer(graph=True): two eager steps, then fwd + BCE + bwd captured once as a HIP graph and
    replayed (inputs copied into its static tensors, Adam eager).  Six steps with changing inputs
    and the trace carried must match eager steps bit for bit - losses, gradients, parameters and
    the trace - which also checks that the captured operand packing runs on every replay (stale
    packed weights after the first replay would change the third loss).  An eager step in between
    (bench.py's profiling pass) must not disturb the replays that follow."""
    from punet.engine import Trainer
    res = []
    for graph in (False, True):
        _, net, x, t, H = _c2_pair(8, seed=5)
        if precision == "bf16":
            sd = net.state_dict()
            net = UNetp(1, 1, DEV, rule="oja", nbf=128, depth=5, base_ch=64, precision="bf16")
            net.load_state_dict(sd)
        tr = Trainer(net, lr=1e-3, steplr=1e5, graph=graph)
        hebb = H.to(DEV)
        losses, grads = [], []
        for s in range(6):
            if s == 4:
                tr.graph = False          # one eager step between replays
            xs = torch.roll(x, shifts=s, dims=0).to(DEV)
            loss, hebb = tr.step(xs, t.to(DEV), hebb)
            tr.graph = graph
            losses.append(loss.item())
            grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        res.append((losses, grads, {k: p.detach().clone() for k, p in net.named_parameters()}, hebb.clone()))
    assert res[0][0] == res[1][0]
    for s in range(6):
        assert res[0][1][s].keys() == res[1][1][s].keys()
        for k in res[0][1][s]:
            assert torch.equal(res[0][1][s][k], res[1][1][s][k]), (s, k)
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    assert torch.equal(res[0][3], res[1][3])


def test_lazy_direct_operands_after_optimizer_steps():
    """After an optimizer step the trunk refreshes only the Winograd operand of a layer that has
    only ever run on the Winograd kernel (punet.packs: Packs.refresh); a later call that takes the direct
    kernel (here: Winograd switched off) must repack the direct operand first.  Compared bit for
    bit with fresh models holding the same weights (they pack everything at first use)."""
    from punet import kernels as K
    from punet.engine import Trainer
    torch.manual_seed(4)
    net = UNetp(1, 1, DEV, rule="oja", nbf=64, depth=4, base_ch=32)
    tr = Trainer(net, lr=1e-3, steplr=1e5)
    g = torch.Generator().manual_seed(9)
    hebb = (0.05 * torch.randn(2, 64, 64, generator=g)).to(DEV)
    for _ in range(2):
        x = torch.rand(2, 1, 64, 64, generator=g).to(DEV)
        t = (torch.rand(2, 64, 64, generator=g) > 0.5).float().to(DEV)
        _, hebb = tr.step(x, t, hebb)
    x = torch.rand(2, 1, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        K.set_wino(False)
        try:
            y_direct, h_direct = net(x, hebb)
            ref = UNetp(1, 1, DEV, rule="oja", nbf=64, depth=4, base_ch=32)
            ref.load_state_dict(net.state_dict())
            r_direct, rh_direct = ref(x, hebb)
        finally:
            K.set_wino(True)
        y_wino, _ = net(x, hebb)
        ref2 = UNetp(1, 1, DEV, rule="oja", nbf=64, depth=4, base_ch=32)
        ref2.load_state_dict(net.state_dict())
        r_wino, _ = ref2(x, hebb)
    assert torch.equal(y_direct, r_direct) and torch.equal(h_direct, rh_direct)
    assert torch.equal(y_wino, r_wino)
    assert not torch.equal(y_direct, y_wino)      # the two paths really are different kernels
