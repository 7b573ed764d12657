"""The last three stages of a training step at sizes the model itself never uses: the plastic
head's backward (pu_plastic_bwd) at ragged and degenerate N, in every output mode and on both tile
sizes; the aliased trace output of pu_plastic_fwd; the BCE kernels at odd sizes, on the grid-stride
paths and with an upstream gradient; multi-tensor Adam with weight decay, other betas / eps,
misaligned pointers, empty tensors, chunk-boundary tails and more tensors than one launch holds.

References are plain fp64 restatements on the CPU (einsum, F.binary_cross_entropy and its
autograd, torch.optim.Adam); the bounds are those of the matching tests in test_kernels_gpu.py.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from punet import kernels as K  # noqa: E402
from punet import _lib  # noqa: E402
from punet.optim import FusedAdam  # noqa: E402

DEV = "cuda"


def rnd(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float()


# ------------------------------------------------------------------------------ head backward
# (B, N): HK = 16 is the k chunk, the tile is 32 unless ceil(N/64)^2 B >= 512 (then 64)
HEAD_BWD_CASES = [
    (1, 16),      # one chunk: the prefetch is never taken
    (2, 17),      # the second chunk holds one valid k; both tile guards active
    (5, 3),       # N smaller than a chunk and than one micro-tile
    (3, 50),      # 32-tile, ragged in tile and in chunk
    (2, 200),     # 32-tile, 7 x 7 blocks, last chunk of 8
    (128, 72),    # 2 * 2 * 128 = 512 blocks: the 64-tile; 72 = 64 + 8
    (32, 200),    # 4 * 4 * 32 = 512 blocks: the 64-tile; 200 = 3 * 64 + 8
]


@functools.lru_cache(maxsize=None)
def _head_case(B, N, zero_h=False):
    """Inputs of test_plastic_bwd_against_fp64 with saturated Y entries (G = 0 exactly there), on
    the device, and the fp64 gradients.  Computed once per case and shared; nothing writes to it."""
    g = torch.Generator().manual_seed(B + N)
    X = rnd(B, N, N, g=g, scale=2.0)
    H = rnd(B, N, N, g=g, scale=0.2)
    w = rnd(N, N, g=g, scale=0.05)
    al = torch.rand(N, N, generator=g) * 0.05
    Y = torch.rand(B, N, N, generator=g)
    dY = rnd(B, N, N, g=g)
    Yf = Y.view(-1)
    Yf[::7] = 0.0
    Yf[3::11] = 1.0
    if zero_h:
        H = torch.zeros_like(H)      # the first training step's trace
    Gd = dY.double() * (1 - Y.double()) * Y.double()
    weff = w.double()[None] + al.double()[None] * H.double()
    T = torch.einsum("bik,bij->bkj", X.double(), Gd)
    ref = (torch.einsum("bij,bkj->bik", Gd, weff), T.sum(0), (T * H.double()).sum(0))
    return tuple(t.to(DEV) for t in (X, H, w, al, Y, dY)), ref


def _assert_head_bound(name, got, ref):
    got = got.cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = 1e-5 * ref.abs().max().item() + 1e-6
    print("%s: err %.3e bound %.3e" % (name, err, bound))
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("zero_h", [False, True])
@pytest.mark.parametrize("B,N", HEAD_BWD_CASES)
def test_plastic_bwd_ragged_against_fp64(B, N, zero_h):
    """dX = G Weff^T, dw = sum_b X_b^T G_b, dalpha = sum_b (X_b^T G_b) . H_b, G = dY (1 - Y) Y in
    fp64, at N that is no multiple of the tile or of the k chunk: the range guards of the loaders
    decide and a partial last chunk goes through the register prefetch.  With H = 0 dalpha is
    exactly 0.  (tests/head_matrix.py now holds the branch list of pu_plastic_bwd: these shapes in
    every output form, with per-entry bounds.)"""
    (X, H, w, al, Y, dY), ref = _head_case(B, N, zero_h)
    dx, dw, da = K.plastic_bwd(X, H, w, al, Y, dY)
    for name, got, r in zip(("dx", "dw", "dalpha"), (dx, dw, da), ref):
        _assert_head_bound(name, got, r)
    if zero_h:
        assert torch.count_nonzero(da).item() == 0


@pytest.mark.parametrize("B,N", [(3, 50), (32, 200)])
def test_plastic_bwd_output_modes(B, N):
    """need_dx / need_dw off and out=(dw_view, da_view) - what punet/head.py uses with the flat
    gradient buffer - give the full call's values bit for bit and write nothing else."""
    (X, H, w, al, Y, dY), _ = _head_case(B, N)
    dx, dw, da = K.plastic_bwd(X, H, w, al, Y, dY)
    dx2, dw2, da2 = K.plastic_bwd(X, H, w, al, Y, dY)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(da, da2)

    dxn, dwn, dan = K.plastic_bwd(X, H, w, al, Y, dY, need_dx=False)
    assert dxn is None
    assert torch.equal(dwn, dw) and torch.equal(dan, da)

    dxo, dwo, dao = K.plastic_bwd(X, H, w, al, Y, dY, need_dw=False)
    assert dwo is None and dao is None
    assert torch.equal(dxo, dx)

    # two [N, N] views into one NaN-filled flat buffer: the first at float offset 1 (not 16-byte
    # aligned), one guard float between them and one after the second
    nn = N * N
    flat = torch.full((2 * nn + 3,), float("nan"), device=DEV)
    dw_view = flat[1:1 + nn].view(N, N)
    da_view = flat[2 + nn:2 + 2 * nn].view(N, N)
    assert dw_view.data_ptr() % 16 != 0 and dw_view.is_contiguous() and da_view.is_contiguous()
    dxv, dwv, dav = K.plastic_bwd(X, H, w, al, Y, dY, out=(dw_view, da_view))
    assert dwv is dw_view and dav is da_view
    assert torch.equal(dxv, dx) and torch.equal(dw_view, dw) and torch.equal(da_view, da)
    guards = flat[[0, 1 + nn, 2 + 2 * nn]]
    assert torch.isnan(guards).all(), guards


@pytest.mark.parametrize("B,N", [(128, 72), (32, 200)])
def test_plastic_bwd_slots_and_tiles_bitwise(B, N):
    """The batched call takes the 64-tile, a B = 1 call on one slot the 32-tile.  Every output is
    one k-ordered fmaf chain in both (zero padding leaves the chain unchanged), the one-slot
    reduce forms 0 + t and 0 + t H, the batched reduce adds slots 0..B-1 in order: dx per slot and
    the slot-ordered fp32 sum of the one-slot dw / dalpha equal the batched results bit for bit."""
    (X, H, w, al, Y, dY), _ = _head_case(B, N)
    dx, dw, da = K.plastic_bwd(X, H, w, al, Y, dY)
    acc_w = torch.zeros(N, N, device=DEV)
    acc_a = torch.zeros(N, N, device=DEV)
    for b in range(B):
        s = slice(b, b + 1)
        check_dx = b in (0, 1, B - 1)
        dx1, dw1, da1 = K.plastic_bwd(X[s], H[s], w, al, Y[s], dY[s], need_dx=check_dx)
        if check_dx:
            assert torch.equal(dx[b], dx1[0]), b
        acc_w = acc_w + dw1
        acc_a = acc_a + da1
    assert torch.equal(dw, acc_w)
    assert torch.equal(da, acc_a)


# ------------------------------------------------------------------- aliased trace output (fwd)
@pytest.mark.parametrize("B,N", [(3, 50), (2, 128), (32, 200)])
@pytest.mark.parametrize("rule", [0, 1])
def test_plastic_fwd_aliased_trace_output(B, N, rule):
    """pu_plastic_fwd with hebb_out == hebb cannot fuse the update (other blocks still read H): it
    runs the GEMM, then the stand-alone update in place.  Y and the updated buffer equal the
    out-of-place call's bit for bit (scalar update kernel at N = 50, float4 at 128 and 200)."""
    g = torch.Generator().manual_seed(B * 1000 + N)
    X = rnd(B, N, N, g=g, scale=2.0).to(DEV)
    H = rnd(B, N, N, g=g, scale=0.2).to(DEV)
    w = rnd(N, N, g=g, scale=0.05).to(DEV)
    al = (torch.rand(N, N, generator=g) * 0.05).to(DEV)
    eta = torch.tensor([0.0173], device=DEV)
    Y_ref, H_ref = K.plastic_fwd(X, H, w, al, eta, rule, True)
    Hbuf = H.clone()
    Y = torch.empty_like(X)
    a = _lib.PlasticArgs(B, N, X.data_ptr(), Hbuf.data_ptr(), w.data_ptr(), al.data_ptr(), eta.data_ptr(),
                         Y.data_ptr(), Hbuf.data_ptr(), rule)
    _lib.check(_lib.load().pu_plastic_fwd(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
               "pu_plastic_fwd (aliased)")
    assert torch.equal(Y, Y_ref)
    assert torch.equal(Hbuf, H_ref)


# ----------------------------------------------------------------------------------------- BCE
# (y, t) written into the first eight elements: saturated, clamped (log >= -100, denominator
# >= 1e-12) and just-not-clamped values
BCE_EDGES = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (1e-30, 0.0), (1.0 - 2.0 ** -24, 0.0),
             (1e-12, 1.0), (2e-12, 1.0)]
BCE_UPSTREAM = 2.5


@functools.lru_cache(maxsize=None)
def _bce_case(n):
    g = torch.Generator().manual_seed(n)
    y = torch.rand(n, generator=g)
    y[y == 0] = 0.5                     # uniform in the open interval
    t = (torch.rand(n, generator=g) > 0.5).float()
    if n >= 255:
        for i, (yy, tt) in enumerate(BCE_EDGES):
            y[i], t[i] = yy, tt
    y64 = y.double().requires_grad_(True)
    loss = F.binary_cross_entropy(y64, t.double())
    (BCE_UPSTREAM * loss).backward()
    return y.to(DEV), t.to(DEV), loss.item(), y64.grad


# 131073 = 512 * 256 + 1: the forward's grid-stride loop runs a second, partial pass;
# 2101249 = 8192 * 256 + 4097: the backward's does
@pytest.mark.parametrize("n", [1, 255, 257, 131073, 2101249])
def test_bce_kernels_against_fp64(n):
    y, t, loss_ref, dy_ref = _bce_case(n)
    loss = K.bce_fwd(y, t)
    rel = abs(loss.item() - loss_ref) / abs(loss_ref)
    print("loss %.9g ref %.9g rel %.3e" % (loss.item(), loss_ref, rel))
    assert rel <= 1e-6, (loss.item(), loss_ref)
    assert torch.equal(K.bce_fwd(y, t), loss)       # fixed-order reduction: bit-equal run to run

    dy = K.bce_bwd(y, t, torch.tensor(BCE_UPSTREAM, device=DEV))
    got = dy.cpu().double()
    # element-wise relative: the clamped elements are ~1e6 times the others and would swallow an
    # absolute term scaled by the maximum
    err = (got - dy_ref).abs()
    nz = dy_ref != 0
    print("dy worst relative error %.3e" % (err[nz] / dy_ref[nz].abs()).max().item())
    assert bool((err <= 1e-6 * dy_ref.abs()).all()), (err / dy_ref.abs().clamp_min(1e-300)).max()
    if n >= 255:
        assert dy[0].item() == 0.0 and dy[1].item() == 0.0      # y == t at 0 and at 1

    assert torch.equal(K.bce_bwd(y, t, None), K.bce_bwd(y, t, torch.tensor(1.0, device=DEV)))


# ---------------------------------------------------------------------------------------- Adam
def _adam_steps(ref, dev, o_ref, o_dev, steps, g, grad_views=None, zero_step=None):
    """Step torch's Adam (fp64, CPU) and FusedAdam on the same gradients; every step starts from
    the kernel's own fp32 parameters and its update is held to test_fused_adam_matches_torch_adam's
    bound, 1e-6 of the reference update's size plus one ulp of the parameter."""
    grad_views = grad_views or {}
    for step in range(steps):
        before = []
        for i, (a, b) in enumerate(zip(ref, dev)):
            p0 = b.detach().cpu().clone()
            before.append(p0)
            a.data.copy_(p0.double())
            gr = rnd(*a.shape, g=g)
            if step == zero_step:
                gr.view(-1)[::3] = 0.0
            a.grad = gr.double()
            if i in grad_views:
                grad_views[i].copy_(gr)
                b.grad = grad_views[i]
            else:
                b.grad = gr.to(DEV)
        o_ref.step()
        o_dev.step()
        for a, b, p0 in zip(ref, dev, before):
            assert b.shape == a.shape
            if a.numel() == 0:
                continue
            du_ref = a.detach() - p0.double()
            du_dev = b.detach().cpu().double() - p0.double()
            err = (du_dev - du_ref).abs().max().item()
            bound = 1e-6 * du_ref.abs().max().item() + 1.2e-7 * p0.abs().max().item()
            assert err <= bound, (step, tuple(a.shape), err, bound)


@pytest.mark.parametrize("betas,eps,wd,lr", [((0.9, 0.999), 1e-8, 0.01, 3e-3),
                                             ((0.8, 0.99), 1e-6, 0.1, 1e-2),
                                             ((0.0, 0.5), 1e-8, 0.0, 1e-3)])
def test_fused_adam_settings_and_layouts(betas, eps, wd, lr):
    """Weight decay, non-default betas / eps; tails that sit at a 4096-element chunk boundary
    (4097, 4096 + 4095), one element, a parameter and gradient at float offset 1 of their buffers
    (the scalar path) and an empty parameter, all in one FusedAdam."""
    g = torch.Generator().manual_seed(11)
    shapes = [(4097,), (4096 + 4095,), (1,), (1000, 33)]
    host = [rnd(*s, g=g) for s in shapes]
    dev = [torch.nn.Parameter(h.to(DEV)) for h in host]
    # the misaligned parameter: a view one float into a larger buffer
    n_mis = 4099
    h_mis = rnd(n_mis, g=g)
    pbuf = rnd(n_mis + 4, g=g).to(DEV)
    pbuf[1:1 + n_mis].copy_(h_mis)
    pbuf0 = pbuf.clone()
    gbuf = torch.zeros(n_mis + 4, device=DEV)
    i_mis = len(dev)
    dev.append(torch.nn.Parameter(pbuf[1:1 + n_mis]))
    host.append(h_mis)
    gview = gbuf[1:1 + n_mis]
    assert dev[i_mis].data_ptr() == pbuf.data_ptr() + 4 and dev[i_mis].data_ptr() % 16 != 0
    assert gview.data_ptr() % 16 != 0
    # the empty parameter
    dev.append(torch.nn.Parameter(torch.empty(0, device=DEV)))
    host.append(torch.empty(0))
    ref = [torch.nn.Parameter(h.double()) for h in host]
    o_ref = torch.optim.Adam(ref, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    o_dev = FusedAdam(dev, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    _adam_steps(ref, dev, o_ref, o_dev, 5, g, grad_views={i_mis: gview}, zero_step=2)
    # the floats around the misaligned view are untouched, the view itself moved
    assert torch.equal(pbuf[:1], pbuf0[:1])
    assert torch.equal(pbuf[1 + n_mis:], pbuf0[1 + n_mis:])
    assert not torch.equal(pbuf[1:1 + n_mis], pbuf0[1:1 + n_mis])
    assert dev[-1].numel() == 0


def test_fused_adam_more_tensors_than_one_launch():
    """40 small parameters of mixed odd sizes: more than the 32 one launch holds."""
    g = torch.Generator().manual_seed(12)
    sizes = [(13 * i + 1) % 61 + 1 for i in range(40)]
    assert len(set(sizes)) > 20 and any(s % 4 for s in sizes)
    host = [rnd(s, g=g) for s in sizes]
    ref = [torch.nn.Parameter(h.double()) for h in host]
    dev = [torch.nn.Parameter(h.to(DEV)) for h in host]
    _adam_steps(ref, dev, torch.optim.Adam(ref), FusedAdam(dev), 2, g)
