"""Column form of the Winograd-domain weight gradient (csrc/wgrad.hip: wgrad_wino_cols_x6_kernel and
wgrad_finish_cols_kernel) against fp64.

A block of the column plan owns one position column j of a 128 x 128 channel block and writes
R[r][j] = sum_a G[a][r] M[a][j]; phase 2 finishes G^T M G per split and sums the splits.  The plan
is taken for c0 % 128 == c1 % 128 == n % 128 == 0 and at least T_MIN tiles (WWR_MIN_TILES in wgrad.hip).

Judged by the rule of tests/test_wino_gpu.py::check (restated here): max error relative to
max|ref| against fp64 at most max(16 x ATen's CPU fp32 error, 4e-6), rtol 1e-4 parity with CPU fp32,
the bias likewise, and two calls bitwise equal.  Every case first asserts, through pu_wgrad_tile,
the plan it is for (columns: kind 5, 128 x 384; fall-backs: kind 5, 64 x 576).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from punet import kernels as K  # noqa: E402

DEV = "cuda"
T_MIN = 512


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_err(got, ref):
    got = got.detach().double().cpu()
    return (got - ref).abs().max().item() / ref.abs().max().item()


def check(name, got, cpu32, ref64):
    eg, ec = rel_err(got, ref64), rel_err(cpu32, ref64)
    print("%-40s cols %.2e  cpu32 %.2e" % (name, eg, ec))
    assert eg <= max(16 * ec, 4e-6), (name, eg, ec)
    torch.testing.assert_close(got.detach().float().cpu(), cpu32.float(), rtol=1e-4,
                               atol=1e-5 * cpu32.abs().max().item())


def plan(B, H, W, c0, c1, n, bias_mode=1):
    """(bn, bk, kind, splits) of pu_wgrad_tile for the 3x3 same-size weight gradient."""
    a = K.wgrad_args(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, rows=16, n=n, src0=16, c0=c0,
                     src1=16 if c1 else None, c1=c1, bias_mode=bias_mode, dweight=16, dbias=16 if bias_mode else None)
    v = [ctypes.c_int() for _ in range(4)]
    K.check(K.lib().pu_wgrad_tile(ctypes.byref(a), *(ctypes.byref(x) for x in v)), "pu_wgrad_tile")
    return tuple(x.value for x in v)


def operands(B, H, W, c0, c1, n):
    """Seeded x (post-ReLU), dZ (30 % zeros), and the CPU fp32 / fp64 weight and bias gradients."""
    g = torch.Generator().manual_seed(B * 17 + H * 5 + W + c0 + 7 * c1 + n)
    C = c0 + c1
    x = torch.randn(B, C, H, W, generator=g).relu()
    dz = torch.randn(B, n, H, W, generator=g) * (torch.rand(B, n, H, W, generator=g) > 0.3).float()
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt] = (torch.nn.grad.conv2d_weight(x.to(dt), (n, C, 3, 3), dz.to(dt), padding=1), dz.to(dt).sum((0, 2, 3)))
    xk = nhwc(x).to(DEV)
    x0, x1 = (xk[..., :c0].contiguous(), xk[..., c0:].contiguous()) if c1 else (xk, None)
    return x0, x1, nhwc(dz).to(DEV), ref


def run(B, H, W, c0, c1, n, x0, x1, dz, bias_mode=1, dw=None, db=None, accumulate=False):
    if dw is None:
        dw = torch.full((n, c0 + c1, 3, 3), float("nan"), device=DEV)
    if db is None:
        db = torch.full((n,), float("nan"), device=DEV)
    K.wgrad(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, rows=dz, n=n, src0=x0, c0=c0, src1=x1, c1=c1,
            bias_mode=bias_mode, dweight=dw, dbias=db if bias_mode else None, accumulate=accumulate)
    return dw, db


COL_CASES = [
    # B, H, W, c0, c1, n
    (2, 32, 32, 128, 0, 128),     # gate edge: exactly T_MIN tiles, 32 tile splits of one stage each
    (3, 24, 30, 128, 0, 128),     # 540 tiles: a ragged last stage (12 tiles); 15-tile rows, so stages span tile rows
    (2, 32, 32, 128, 128, 128),   # two sources, gx = 2
    (2, 32, 32, 128, 0, 256),     # two output channel blocks
    (32, 8, 8, 256, 0, 256),      # every tile touches an image edge; 2 x 2 channel blocks (the bottom level's
                                  # geometry at a quarter of its channels), 2 stages per block
    (16, 32, 32, 128, 0, 128),    # 4 stages per block: the column reloads and both slots
]


@pytest.mark.parametrize("B,H,W,c0,c1,n", COL_CASES)
def test_cols_wgrad_vs_fp64(B, H, W, c0, c1, n):
    assert B * (H // 2) * (W // 2) >= T_MIN
    assert plan(B, H, W, c0, c1, n)[:3] == (128, 384, 5)
    x0, x1, dz, ref = operands(B, H, W, c0, c1, n)
    dw, db = run(B, H, W, c0, c1, n, x0, x1, dz)
    name = "%dx%dx%d %d+%d->%d" % (B, H, W, c0, c1, n)
    check("cols wgrad " + name, dw, ref[torch.float32][0], ref[torch.float64][0])
    check("cols bias grad " + name, db, ref[torch.float32][1], ref[torch.float64][1])
    dw2, db2 = run(B, H, W, c0, c1, n, x0, x1, dz)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "column weight gradient is not deterministic"


def test_cols_wgrad_without_bias_and_accumulate():
    """bias_mode 0 leaves dbias alone; accumulate onto seeded gradients is one fp32 add per entry,
    bitwise torch.add of the plain result."""
    B, H, W, c0, c1, n = 2, 32, 32, 128, 0, 128
    assert plan(B, H, W, c0, c1, n, bias_mode=0)[:3] == (128, 384, 5)
    x0, x1, dz, ref = operands(B, H, W, c0, c1, n)
    dw, db = run(B, H, W, c0, c1, n, x0, x1, dz, bias_mode=0)
    check("cols wgrad, no bias", dw, ref[torch.float32][0], ref[torch.float64][0])
    assert bool(db.isnan().all()), "bias_mode 0 wrote dbias"
    dwb, dbb = run(B, H, W, c0, c1, n, x0, x1, dz)
    assert torch.equal(dw, dwb), "the bias column changed the weight gradient"
    g = torch.Generator().manual_seed(5)
    seed_w, seed_b = torch.randn(n, c0, 3, 3, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    aw, ab = run(B, H, W, c0, c1, n, x0, x1, dz, dw=seed_w.clone(), db=seed_b.clone(), accumulate=True)
    assert torch.equal(aw, torch.add(seed_w, dwb)) and torch.equal(ab, torch.add(seed_b, dbb))


@pytest.mark.parametrize("B,H,W,c0,c1,n", [
    (2, 32, 32, 128, 0, 192),     # n is no multiple of 128
    (2, 32, 32, 64, 64, 128),     # 64-channel sources
])
def test_fallback_keeps_the_64x64_kernel(B, H, W, c0, c1, n):
    assert B * (H // 2) * (W // 2) >= T_MIN
    assert plan(B, H, W, c0, c1, n)[:3] == (64, 576, 5)
    x0, x1, dz, ref = operands(B, H, W, c0, c1, n)
    dw, db = run(B, H, W, c0, c1, n, x0, x1, dz)
    check("fall-back wgrad", dw, ref[torch.float32][0], ref[torch.float64][0])
    check("fall-back bias grad", db, ref[torch.float32][1], ref[torch.float64][1])


@pytest.mark.parametrize("B,H,W,C,n,cut", [
    (2, 32, 32, 128, 128, 64),      # two reduction groups in the 64 x 64 plan
    (3, 24, 30, 128, 128, 64),      # 34 splits, ragged last stage
    (32, 8, 8, 256, 256, 192),      # one group; image edges
    (2, 32, 32, 256, 128, 64),      # 64 + 192
])
def test_cols_wgrad_is_bitwise_the_64x64_kernels(B, H, W, C, n, cut):
    """The same layer with its input handed over as two sources cut off a 128-channel boundary takes
    wgrad_wino_x6_kernel with the same tile splits: the column plan must reproduce it bit for bit
    (same operations in the same order per value)."""
    assert plan(B, H, W, C, 0, n)[:3] == (128, 384, 5)
    assert plan(B, H, W, cut, C - cut, n)[:3] == (64, 576, 5)
    assert plan(B, H, W, C, 0, n)[3] == 4 * plan(B, H, W, cut, C - cut, n)[3]
    g = torch.Generator().manual_seed(B + H + C + n)
    x = torch.randn(B, H, W, C, generator=g).relu().to(DEV)
    dz = (torch.randn(B, H, W, n, generator=g) * (torch.rand(B, H, W, n, generator=g) > 0.3).float()).to(DEV)
    dw, db = run(B, H, W, C, 0, n, x, None, dz)
    dw2, db2 = run(B, H, W, cut, C - cut, n, x[..., :cut].contiguous(), x[..., cut:].contiguous(), dz)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
