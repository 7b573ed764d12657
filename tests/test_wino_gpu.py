"""Winograd F(2x2,3x3) path of the fp32 3x3 convolutions (csrc/winograd.hip) against fp64.

The Winograd kernel does not reproduce the direct kernel's summation order, so it is judged the
way tests/test_precision_gpu.py judges every conv kernel: its max error relative to max|ref|
against the fp64 result, next to ATen's CPU fp32 error on the same op (bound: max(16 x CPU, 4e-6)),
plus rtol 1e-4 parity with CPU fp32 and bitwise run-to-run determinism.  Cases cover the epilogue
variants the U-Net uses (bias + ReLU, residual, ReLU masks, the concat split of the data
gradient, accumulate), the skip concat as two sources, partial tile blocks, non-square and
many-image grids, and the split-K plan of the 8x8 / 16x16 levels."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from punet import kernels as K  # noqa: E402
from punet import trunk as T  # noqa: E402

DEV = "cuda"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_err(got, ref):
    got = got.detach().double().cpu()
    return (got - ref).abs().max().item() / ref.abs().max().item()


def check(name, got, cpu32, ref64):
    eg, ec = rel_err(got, ref64), rel_err(cpu32, ref64)
    print("%-34s wino %.2e  cpu32 %.2e" % (name, eg, ec))
    assert eg <= max(16 * ec, 4e-6), (name, eg, ec)
    torch.testing.assert_close(got.detach().float().cpu(), cpu32.float(), rtol=1e-4,
                               atol=1e-5 * cpu32.abs().max().item())


CASES = [
    # B, H, W, c0, c1, cout
    (2, 16, 16, 64, 0, 64),       # one block of 64 tiles x 2 images
    (3, 10, 14, 128, 0, 128),     # 105 tiles: a ragged second tile block, 2 channel blocks, non-square
    (2, 8, 8, 64, 64, 64),        # concat (two sources), every tile on an image edge; wide-item dgrad
    (1, 32, 16, 128, 0, 192),     # 3 channel blocks, 8 chunks
    (4, 8, 8, 512, 0, 512),       # split-K (bottom level shape): 64 tiles, 8 channel blocks
    (2, 16, 16, 256, 256, 256),   # split-K with two sources (the 16x16 up level)
    (1, 2, 2, 32, 0, 64),         # a single 2x2 tile
    # many items of wino4_x6_kernel (one per block): more blocks than CUs, so the XCD-aware item
    # order wraps
    (5, 128, 128, 64, 0, 64),     # 320 items of 64 x 64
    (3, 96, 80, 128, 0, 192),     # 270 items (not a multiple of the 8 XCDs), 3 channel blocks
    # n % 128 == 0 shapes: 64 x 64 items when C >= 128, wide (32-tile x 128-channel) items when C < 128
    (2, 16, 16, 128, 0, 256),     # 4 channel blocks of 64
    (5, 128, 128, 64, 0, 128),    # 64 -> 128 forward on wide items: 640 items
    (7, 96, 80, 128, 0, 128),     # 420 items (420 % 8 = 4), 2 channel blocks
    (2, 24, 24, 64, 64, 64),      # its data gradient 64 -> 128 split at 64 (the top concat layer): wide
                                  # items whose two 32-channel block pairs go to different destinations
    (2, 24, 24, 128, 128, 128),   # concat forward on 64 x 64 items; data gradient 128 -> 256 split at 128
    (3, 16, 16, 64, 0, 128),      # wide items forward (6 items of 32 tiles); data gradient 128 -> 64
]


@pytest.mark.parametrize("B,H,W,c0,c1,cout", CASES)
def test_wino_fwd_dgrad_vs_fp64(B, H, W, c0, c1, cout):
    g = torch.Generator().manual_seed(B * 131 + H * 7 + W + c0 + 3 * c1 + cout)
    C = c0 + c1
    x = torch.randn(B, C, H, W, generator=g).relu()
    w = torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    dz = torch.randn(B, cout, H, W, generator=g) * (torch.rand(B, cout, H, W, generator=g) > 0.5).float()
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.detach().to(dt).clone().requires_grad_(True)
        z = F.conv2d(xr, w.to(dt), b.to(dt), padding=1)
        z.backward(dz.to(dt))
        ref[dt] = (torch.relu(z).detach(), (xr.grad * (x > 0).to(dt)).detach())
    prev = K.set_wino(True)
    try:
        pk = T._Packs()
        xk = nhwc(x).to(DEV)
        x0, x1 = (xk[..., :c0].contiguous(), xk[..., c0:].contiguous()) if c1 else (xk, None)
        wk = w.to(DEV)
        assert (pk.get(wk, 0, K.round16(9 * C), K.cgroup_for(c0, c1)).wino is not None) \
            == K.wino_wanted(wk, 0)
        y = T.conv3x3(x0, wk, b.to(DEV), pk, x1=x1, relu=True)
        check("wino fwd %dx%dx%d %d+%d->%d" % (B, H, W, c0, c1, cout), nchw(y), ref[torch.float32][0],
              ref[torch.float64][0])
        y2 = T.conv3x3(x0, wk, b.to(DEV), pk, x1=x1, relu=True)
        assert torch.equal(y, y2), "Winograd forward is not deterministic"
        dzk = nhwc(dz).to(DEV)
        d0, d1 = T.conv3x3_dgrad(dzk, wk, pk, split=c0 if c1 else None, mask0=x0, mask1=x1)
        dx = torch.cat([d0, d1], 3) if c1 else d0
        assert (pk.get(wk, 1, K.round16(9 * cout), K.cgroup_for(cout)).wino is not None) \
            == K.wino_wanted(wk, 1)
        check("wino dgrad", nchw(dx), ref[torch.float32][1], ref[torch.float64][1])
    finally:
        K.set_wino(prev)


def _wino_plan(B, H, W, C, N, x, packed, k_pad, dst, bias=None, resid=None, relu=False, accum=False):
    """(mode, item channels, ksplit) pu_conv_igemm_tile reports for the call K.igemm makes with
    these operands (mode 6 = the Winograd kernel), with the split-K workspace K.igemm would pass."""
    import ctypes
    from punet import _lib
    flags = (_lib.PU_EPI_RELU if relu else 0) | (_lib.PU_EPI_ACCUM if accum else 0) | \
        (_lib.PU_EPI_RESID if resid is not None else 0)
    a = _lib.ConvArgs(B, H, W, H, W, 3, 3, 1, 1, x.data_ptr(), C, None, 0, packed.direct.data_ptr(), k_pad,
                      K.cgroup_for(C), N, None if bias is None else bias.data_ptr(), dst.data_ptr(), N, None,
                      None, None, flags, None, 0, None if resid is None else resid.data_ptr())
    a.weight6 = packed.planes.data_ptr()
    a.wino = packed.wino.data_ptr()
    L = K.lib()
    nbytes = L.pu_conv_igemm_workspace_bytes(ctypes.byref(a))
    if nbytes:      # planning only reads the pointer's presence and the size
        a.workspace, a.ws_bytes = dst.data_ptr(), nbytes
    bm, bn, mode, ks = (ctypes.c_int() for _ in range(4))
    assert L.pu_conv_igemm_tile(ctypes.byref(a), *(ctypes.byref(v) for v in (bm, bn, mode, ks))) == 0
    return mode.value, bn.value, ks.value


def _resid_and_accumulate(B, H, W, C, N, item_n, split):
    """RESID (the residual add before the ReLU) and ACCUM through the Winograd kernel's general
    epilogue (the FULL instantiations) or, with split, through the split-K finish: against fp64
    next to ATen's CPU fp32 error, and against the direct kernel on the same layer (both within
    fp32 rounding of each other).  Each call really takes the Winograd kernel with item_n-channel
    items."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(N, C, 3, 3, generator=g) * 0.05
    b = torch.randn(N, generator=g)
    r = torch.randn(B, H, W, N, generator=g)
    acc0 = torch.randn(B, H, W, N, generator=g)
    ref = {}
    for dt in (torch.float32, torch.float64):
        z = F.conv2d(nchw(x).to(dt), w.to(dt), None, padding=1)
        ref[dt] = (torch.relu(z + b.to(dt).view(1, N, 1, 1) + nchw(r).to(dt)), nchw(acc0).to(dt) + z)
    x, w, b, r, acc0 = (t.to(DEV) for t in (x, w, b, r, acc0))
    outs = {}
    for on in (True, False):
        prev = K.set_wino(on)
        try:
            pk = T._Packs()
            k_pad = K.round16(9 * C)
            packed = pk.get(w, 0, k_pad, K.cgroup_for(C))
            assert (packed.wino is not None) == on
            o1 = torch.empty(B, H, W, N, device=DEV)
            o2 = acc0.clone()
            if on:
                for plan in (_wino_plan(B, H, W, C, N, x, packed, k_pad, o1, bias=b, resid=r, relu=True),
                             _wino_plan(B, H, W, C, N, x, packed, k_pad, o2, accum=True)):
                    assert plan[:2] == (6, item_n), plan
                    assert (plan[2] >= 2) == split, plan
            K.igemm(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, src0=x, c0=C, weight=packed,
                    k_pad=k_pad, n=N, bias=b, dst0=o1, relu=True, resid=r, cgroup=K.cgroup_for(C))
            K.igemm(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, src0=x, c0=C, weight=packed,
                    k_pad=k_pad, n=N, dst0=o2, accum=True, cgroup=K.cgroup_for(C))
            outs[on] = (o1.cpu(), o2.cpu())
        finally:
            K.set_wino(prev)
    shape = "%dx%dx%d %d->%d" % (B, H, W, C, N)
    for i, name in enumerate(("wino resid+relu " + shape, "wino accumulate " + shape)):
        check(name, nchw(outs[True][i]), ref[torch.float32][i], ref[torch.float64][i])
    for a, bb in zip(outs[True], outs[False]):
        torch.testing.assert_close(a, bb, rtol=1e-5, atol=2e-5 * bb.abs().max().item())


def test_wino_resid_and_accumulate_epilogues():
    """wino4_x6_kernel<true, 2>: one 64 x 64 item, 48 of its 64 tiles."""
    _resid_and_accumulate(2, 12, 8, 64, 64, 64, False)


@pytest.mark.parametrize("B,H,W,C,N,item_n,split", [
    (1, 4, 4, 64, 128, 128, False),    # <true, 4>: one ragged wide item of 4 tiles
    (2, 16, 8, 64, 128, 128, False),   # <true, 4>: two full wide items
    (1, 8, 8, 256, 64, 64, True),      # 16 tiles, 16 chunks: a 2-way K split, so the residual and the
                                       # ReLU run in igemm_splitk_epilogue_kernel
])
def test_wino_resid_and_accumulate_epilogues_wide_and_split_k(B, H, W, C, N, item_n, split):
    _resid_and_accumulate(B, H, W, C, N, item_n, split)


def test_pack_wino_is_G_g_Gt_split_exactly():
    """pu_pack_wino: each (position, n, c) is G g G^T formed in fp64, rounded to fp32, split into
    hi/mid/lo bf16 that sum back to it exactly; forward and the flipped/transposed dgrad kernel."""
    g = torch.Generator().manual_seed(3)
    cout, cin = 64, 32
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64).float()
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    for dgrad in (0, 1):
        n, c = (cout, cin) if not dgrad else (cin, cout)
        gk = w.double() if not dgrad else w.double().transpose(0, 1).flip(2, 3)   # [n][c][3][3]
        U = torch.einsum("ar,ncrs,bs->abnc", G, gk, G).reshape(16, n, c).float()
        out = torch.empty(K.lib().pu_wino_bytes(n, c) // 2, dtype=torch.bfloat16, device=DEV)
        K.pack_wino([(w.to(DEV), out, dgrad)])
        planes = out.cpu().float().reshape(c // 16, 16, 3, n, 16)       # [chunk][xi][plane][n][c16]
        got = planes.permute(1, 2, 3, 0, 4).reshape(16, 3, n, c)
        assert torch.equal(got[:, 0] + got[:, 1] + got[:, 2], U), dgrad
        assert torch.equal(got[:, 0], U.bfloat16().float())


WGRAD_CASES = [
    # B, H, W, c0, c1, cout
    (2, 16, 16, 64, 0, 64),       # one channel block; 8x8 tile grid (a 16-tile stage spans 2 tile rows)
    (3, 10, 14, 128, 0, 128),     # 105 tiles: a ragged last stage, 2 x 2 channel blocks, non-square
    (2, 8, 8, 64, 64, 64),        # concat (two sources), every tile on an image edge
    (1, 32, 16, 128, 0, 192),     # 3 output blocks
    (4, 8, 8, 512, 0, 512),       # 64 channel blocks x 4 splits (the bottom level)
    (2, 16, 16, 256, 256, 256),   # two 256-channel sources, 8 x 4 blocks
    (8, 64, 64, 64, 0, 64),       # 256 splits of 32 tiles (the top level's shape at bs 8)
    (1, 2, 2, 64, 0, 64),         # a single tile
]


@pytest.mark.parametrize("B,H,W,c0,c1,cout", WGRAD_CASES)
def test_wino_wgrad_vs_fp64(B, H, W, c0, c1, cout):
    """wgrad_wino_x6_kernel (dW = G^T [sum_tiles (A e A^T)(.)(B^T d B)] G, bias as dZ column sums)
    against fp64, next to ATen's CPU fp32 error; bitwise run-to-run determinism; and the kernel
    really is the one dispatched (pu_wgrad_tile kind 5)."""
    g = torch.Generator().manual_seed(B * 17 + H * 5 + W + c0 + 7 * c1 + cout)
    C = c0 + c1
    x = torch.randn(B, C, H, W, generator=g).relu()
    dz = torch.randn(B, cout, H, W, generator=g) * (torch.rand(B, cout, H, W, generator=g) > 0.3).float()
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt] = (torch.nn.grad.conv2d_weight(x.to(dt), (cout, C, 3, 3), dz.to(dt), padding=1),
                   dz.to(dt).sum((0, 2, 3)))
    xk = nhwc(x).to(DEV)
    x0, x1 = (xk[..., :c0].contiguous(), xk[..., c0:].contiguous()) if c1 else (xk, None)
    dzk = nhwc(dz).to(DEV)
    assert K.wgrad_kind(batch=B, hw=(H, W), n=cout, c0=c0, c1=c1) == 5
    dw, db = T.conv3x3_wgrad(dzk, x0, x1)
    check("wino wgrad %dx%dx%d %d+%d->%d" % (B, H, W, c0, c1, cout), dw, ref[torch.float32][0], ref[torch.float64][0])
    check("wino bias grad", db, ref[torch.float32][1], ref[torch.float64][1])
    dw2, db2 = T.conv3x3_wgrad(dzk, x0, x1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "Winograd weight gradient is not deterministic"
