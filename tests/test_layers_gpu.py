"""punet.layers' 3x3 helpers serve both trunks: the dtype-aware (UNetp, bf16) and the resid /
chan_scale-aware (UNetpRes) callers go through one conv3x3 / conv3x3_dgrad / conv3x3_wgrad.

fp32 against torch fp64 at test_res_gpu.py's tolerances (rtol 1e-4, atol 1e-5 of the largest
reference value); bf16 against fp64 on the bf16-rounded operands at test_bf16_gpu.py's (activations
rtol 8e-3 / atol 2e-3, fp32 weight gradients rtol 2e-4 / atol 2e-5).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from punet import layers as L  # noqa: E402
from punet.packs import Packs  # noqa: E402

DEV = torch.device("cuda")
BF = torch.bfloat16


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(got, ref, rtol, atol_rel):
    got = got.detach().double().cpu()
    ref = ref.detach().double()
    scale = max(ref.abs().max().item(), 1e-30)
    torch.testing.assert_close(got, ref.reshape(got.shape), rtol=rtol, atol=atol_rel * scale)


@pytest.mark.parametrize("extras", [True, False], ids=["resid_chan_scale", "plain"])
def test_conv3x3_helpers_fp32_two_sources_split_masks(extras):
    """B=2, 8x8, [16 | 16] -> 16 channels.  Forward over two sources (+ resid); the data gradient
    split over the two sources with mask1 (* chan_scale); the unsplit data gradient with mask0
    (+ resid, * chan_scale) - the residual epilogue needs an unsplit output (plastic_unet.h);
    the weight gradient over both sources."""
    B, H, c0, c1, cout = 2, 8, 16, 16, 16
    g = torch.Generator().manual_seed(11)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale        # noqa: E731
    x0, x1 = r(B, c0, H, H).relu(), r(B, c1, H, H).relu()
    w, b = r(cout, c0 + c1, 3, 3, scale=0.2), r(cout)
    res = r(B, cout, H, H).relu()
    pk = Packs()
    dev = lambda t: t.to(DEV)                                              # noqa: E731
    # forward
    y = F.conv2d(torch.cat([x0, x1], 1).double(), w.double(), b.double(), padding=1)
    y = torch.relu(y + res.double() if extras else y)
    yk = L.conv3x3(dev(nhwc(x0)), dev(w), dev(b), pk, x1=dev(nhwc(x1)), resid=dev(nhwc(res)) if extras else None)
    assert yk.dtype == torch.float32
    close(nchw(yk), y, 1e-4, 1e-5)
    # split data gradient: [0,16) -> d0, [16,32) -> d1 masked by the second source
    dz = r(B, cout, H, H)
    m = (torch.rand(B, c0 + c1, generator=g) >= 0.5).float() * 2.0
    dx = F.conv_transpose2d(dz.double(), w.double(), padding=1)
    ref0, ref1 = dx[:, :c0], dx[:, c0:] * (x1 > 0)
    if extras:
        ref0, ref1 = ref0 * m[:, :c0, None, None], ref1 * m[:, c0:, None, None]
    d0, d1 = L.conv3x3_dgrad(dev(nhwc(dz)), dev(w), pk, split=c0, mask1=dev(nhwc(x1)),
                             chan_scale=dev(m) if extras else None)
    close(nchw(d0), ref0, 1e-4, 1e-5)
    close(nchw(d1), ref1, 1e-4, 1e-5)
    # unsplit data gradient of a 16 -> 16 conv: (+ resid) . mask0 (* chan_scale)
    w2 = r(cout, cout, 3, 3, scale=0.2)
    gskip = r(B, cout, H, H)
    ref = F.conv_transpose2d(dz.double(), w2.double(), padding=1)
    ref = (ref + gskip.double() if extras else ref) * (x0 > 0)
    if extras:
        ref = ref * m[:, :cout, None, None]
    dk, none = L.conv3x3_dgrad(dev(nhwc(dz)), dev(w2), pk, mask0=dev(nhwc(x0)),
                               resid=dev(nhwc(gskip)) if extras else None,
                               chan_scale=dev(m[:, :cout].contiguous()) if extras else None)
    assert none is None
    close(nchw(dk), ref, 1e-4, 1e-5)
    # weight and bias gradient over [x0 | x1]
    xc = torch.cat([x0, x1], 1).double()
    wd = w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    F.conv2d(xc, wd, bd, padding=1).backward(dz.double())
    dw, db = L.conv3x3_wgrad(dev(nhwc(dz)), dev(nhwc(x0)), dev(nhwc(x1)))
    close(dw, wd.grad, 1e-4, 1e-5)
    close(db, bd.grad, 1e-4, 1e-5)


def test_conv3x3_helpers_bf16():
    """B=2, 8x8, [32 | 32] -> 32 channels in bf16: the same functions pick the bf16 K padding, K
    order and operand from the input's dtype; weight gradients stay fp32."""
    B, H, c, cout = 2, 8, 32, 32
    g = torch.Generator().manual_seed(12)
    rb = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).float()   # noqa: E731
    x0, x1 = rb(B, c, H, H).relu(), rb(B, c, H, H).relu()
    w, b = rb(cout, 2 * c, 3, 3, scale=0.05), torch.randn(cout, generator=g)
    pk = Packs()
    k0, k1 = nhwc(x0).to(DEV).to(BF), nhwc(x1).to(DEV).to(BF)
    y = torch.relu(F.conv2d(torch.cat([x0, x1], 1).double(), w.double(), b.double(), padding=1))
    yk = L.conv3x3(k0, w.to(DEV), b.to(DEV), pk, x1=k1)
    assert yk.dtype == BF
    close(nchw(yk), y, 8e-3, 2e-3)
    dz = rb(B, cout, H, H) * (y > 0)                       # bf16-exact: rounded values, 0/1 mask
    dzk = nhwc(dz).to(DEV).to(BF)
    dx = F.conv_transpose2d(dz.double(), w.double(), padding=1)
    d0, d1 = L.conv3x3_dgrad(dzk, w.to(DEV), pk, split=c, mask0=k0, mask1=k1)
    assert d0.dtype == BF and d1.dtype == BF
    close(nchw(d0), dx[:, :c] * (x0 > 0), 8e-3, 2e-3)
    close(nchw(d1), dx[:, c:] * (x1 > 0), 8e-3, 2e-3)
    wd = w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    F.conv2d(torch.cat([x0, x1], 1).double(), wd, bd, padding=1).backward(dz.double())
    dw, db = L.conv3x3_wgrad(dzk, k0, k1)
    assert dw.dtype == torch.float32
    close(dw, wd.grad, 2e-4, 2e-5)
    close(db, bd.grad, 2e-4, 2e-5)
