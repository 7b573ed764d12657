"""The layer ops of every trunk: each a thin schedule of one or two punet.kernels launches over
NHWC activations, with its packed weight taken from a punet.packs.Packs cache.

These are the only definitions; punet.trunk and punet.res_trunk import them (and keep the names
importable from there).  The activation dtype - fp32, or bf16 for the C3 trunk - is the input's:
it picks the K padding, the K order of the packed operand and the operand's cache key.
"""
import torch

from . import kernels as K
from ._lib import (PU_PACK_CONV_FWD, PU_PACK_CONV_DGRAD, PU_PACK_CONVT_FWD, PU_PACK_CONVT_DGRAD,
                   PU_PACK_CONVT3_FWD)


def _kp(k, dt):
    """K padded to the kernel's stage: 16 fp32 or 32 bf16 values."""
    return K.round16(k) if dt == torch.float32 else (k + 31) // 32 * 32


def _cg(dt, c0, c1=0):
    """K order of a packed operand: the fp32 kernels' 16/32-channel groups, or 32 for bf16."""
    if dt == torch.float32:
        return K.cgroup_for(c0, c1)
    if c0 % 32 or c1 % 32:
        raise RuntimeError("bf16 convolutions need channel counts that are multiples of 32 (got %d, %d)" % (c0, c1))
    return 32


# ------------------------------------------------------------------------------- 3x3 conv
def conv3x3(x0, w, b, packs, x1=None, relu=True, resid=None, out_dtype=None):
    """3x3/p1 conv over the channel concat [x0 | x1] (NHWC) + bias (+ resid) (then ReLU).
    out_dtype bf16 with an fp32 single-channel x0: the stem writes the bf16 trunk's first
    activation directly."""
    B, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[3]
    cout = w.shape[0]
    dt = x0.dtype
    k_pad = _kp(9 * (c0 + c1), dt)
    g = _cg(dt, c0, c1)
    out = torch.empty(B, H, W, cout, dtype=out_dtype or dt, device=x0.device)
    K.igemm(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, src0=x0, c0=c0, src1=x1, c1=c1,
            weight=packs.get(w, PU_PACK_CONV_FWD, k_pad, g, dt), k_pad=k_pad, n=cout, bias=b, dst0=out, relu=relu,
            cgroup=g, resid=resid)
    return out


def conv3x3_dgrad(dz, w, packs, split=None, mask0=None, mask1=None, resid=None, chan_scale=None):
    """dX = conv(dZ, flipped W^T) (+ resid) (. mask) (* chan_scale[b, c]: the Dropout2d backward);
    optional channel split [0,split) -> d0, rest -> d1."""
    B, H, W, cout = dz.shape
    cin = w.shape[1]
    dt = dz.dtype
    k_pad = _kp(9 * cout, dt)
    g = _cg(dt, cout)
    n0 = cin if split is None else split
    d0 = torch.empty(B, H, W, n0, dtype=dt, device=dz.device)
    d1 = None if split is None else torch.empty(B, H, W, cin - n0, dtype=dt, device=dz.device)
    K.igemm(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, src0=dz, c0=cout,
            weight=packs.get(w, PU_PACK_CONV_DGRAD, k_pad, g, dt), k_pad=k_pad, n=cin, dst0=d0, n0=n0, dst1=d1,
            mask0=mask0, mask1=mask1, cgroup=g, resid=resid, chan_scale=chan_scale)
    return d0, d1


def conv3x3_wgrad(dz, x0, x1=None, out=None):
    B, H, W, cout = dz.shape
    c0 = x0.shape[3]
    c1 = 0 if x1 is None else x1.shape[3]
    if out is None:
        dw = torch.empty(cout, c0 + c1, 3, 3, dtype=torch.float32, device=dz.device)
        db = torch.empty(cout, dtype=torch.float32, device=dz.device)
    else:
        dw, db = out
    K.wgrad(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, rows=dz, n=cout, src0=x0, c0=c0,
            src1=x1, c1=c1, bias_mode=1, dweight=dw, dbias=db)
    return dw, db


# ------------------------------------------------------------------- 1x1 conv (CoordConv stem)
def conv1x1(x, w, b, packs, relu=True):
    """1x1 conv + bias (then ReLU), fp32."""
    B, H, W, cin = x.shape
    cout = w.shape[0]
    k_pad = K.round16(cin)
    out = torch.empty(B, H, W, cout, dtype=torch.float32, device=w.device)
    K.igemm(batch=B, in_hw=(H, W), out_hw=(H, W), k=1, stride=1, pad=0, src0=x, c0=cin,
            weight=packs.get(w, PU_PACK_CONV_FWD, k_pad), k_pad=k_pad, n=cout, bias=b, dst0=out, relu=relu)
    return out


def conv1x1_wgrad(dz, x, out=None):
    B, H, W, cout = dz.shape
    cin = x.shape[3]
    if out is None:
        dw = torch.empty(cout, cin, 1, 1, dtype=torch.float32, device=dz.device)
        db = torch.empty(cout, dtype=torch.float32, device=dz.device)
    else:
        dw, db = out
    K.wgrad(batch=B, in_hw=(H, W), out_hw=(H, W), k=1, stride=1, pad=0, rows=dz, n=cout, src0=x, c0=cin,
            bias_mode=1, dweight=dw, dbias=db)
    return dw, db


# ------------------------------------------------------------- ConvTranspose2d(2, stride=2)
def convT2x2(x, w, b, packs):
    """ConvTranspose2d(cin, cout, 2, stride=2): GEMM [B*h*w, cin] x [cin, 4*cout] + pixel shuffle."""
    B, h, wd, cin = x.shape
    cout = w.shape[1]
    dt = x.dtype
    k_pad = _kp(cin, dt)
    out = torch.empty(B, 2 * h, 2 * wd, cout, dtype=dt, device=x.device)
    K.igemm(batch=B, in_hw=(h, wd), out_hw=(h, wd), k=1, stride=1, pad=0, src0=x, c0=cin,
            weight=packs.get(w, PU_PACK_CONVT_FWD, k_pad, 0, dt), k_pad=k_pad, n=4 * cout, bias=b, dst0=out,
            shuffle=True)
    return out


def convT2x2_dgrad(du, w, packs, mask):
    """dX[b,h,w,:] = sum_(i,j) dU[b,2h+i,2w+j,:] W[:, :, i, j]^T, times (mask > 0)."""
    B, H2, W2, cout = du.shape
    cin = w.shape[0]
    dt = du.dtype
    k_pad = _kp(4 * cout, dt)
    g = _cg(dt, cout)
    dx = torch.empty(B, H2 // 2, W2 // 2, cin, dtype=dt, device=du.device)
    K.igemm(batch=B, in_hw=(H2, W2), out_hw=(H2 // 2, W2 // 2), k=2, stride=2, pad=0, src0=du, c0=cout,
            weight=packs.get(w, PU_PACK_CONVT_DGRAD, k_pad, g, dt), k_pad=k_pad, n=cin, dst0=dx, mask0=mask,
            cgroup=g)
    return dx


def convT2x2_wgrad(x, du, out=None):
    B, h, wd, cin = x.shape
    cout = du.shape[3]
    if out is None:
        dw = torch.empty(cin, cout, 2, 2, dtype=torch.float32, device=x.device)
        db = torch.empty(cout, dtype=torch.float32, device=x.device)
    else:
        dw, db = out
    K.wgrad(batch=B, in_hw=(2 * h, 2 * wd), out_hw=(h, wd), k=2, stride=2, pad=0, rows=x, n=cin, src0=du,
            c0=cout, bias_mode=2, dweight=dw, dbias=db)
    return dw, db


# ------------------------------------------------- ConvTranspose2d(3, stride=2) + crop (fp32)
def _crop(h, out_h):
    crop = 2 * h + 1 - out_h
    if crop not in (0, 1):
        raise RuntimeError("ConvTranspose2d(3, s=2) output %d cannot be padded to the skip size %d "
                           "(unet_p_res.py:215-217 only ever crops one row)" % (2 * h + 1, out_h))
    return crop


def _fusable(m):
    """A Dropout2d mask the conv epilogue can apply (float4 rows: width % 4 == 0, 16-byte aligned
    contiguous rows), else None (a separate pu_channel_scale pass)."""
    if m is None or m.shape[1] % 4 or not m.is_contiguous() or m.data_ptr() % 16:
        return None
    return m


def convT3x3(x, w, b, packs, out_hw, chan_scale=None):
    """ConvTranspose2d(cin, cout, 3, stride=2, padding=0) + crop to out_hw (NHWC); chan_scale
    [B, >= cout] (row stride = its width): per-(image, channel) factors (the Dropout2d of up())."""
    B, h, wd, cin = x.shape
    cout = w.shape[1]
    H2, W2 = out_hw
    crop = _crop(h, H2)
    if _crop(wd, W2) != crop:
        raise RuntimeError("non-square crop")
    k_pad = K.round16(4 * cin)
    out = torch.empty(B, H2, W2, cout, dtype=torch.float32, device=x.device)
    K.igemm(batch=B, in_hw=(h, wd), out_hw=(h + 1, wd + 1), k=2, stride=1, pad=1, src0=x, c0=cin,
            weight=packs.get(w, PU_PACK_CONVT3_FWD, k_pad), k_pad=k_pad, n=4 * cout, bias=b, dst0=out,
            shuffle=True, shuf=(H2, W2, crop), chan_scale=chan_scale)
    return out


def convT3x3_dgrad(du, w, packs, in_hw, mask):
    """dX[i] = sum_r W[:, :, r] dU_full[2i + r] (dU_full[o] = du[o - crop]), times (mask > 0)."""
    B, H2, W2, cout = du.shape
    cin = w.shape[0]
    h, wd = in_hw
    crop = _crop(h, H2)
    k_pad = K.round16(9 * cout)
    g = K.cgroup_for(cout)
    dx = torch.empty(B, h, wd, cin, dtype=torch.float32, device=du.device)
    K.igemm(batch=B, in_hw=(H2, W2), out_hw=(h, wd), k=3, stride=2, pad=crop, src0=du, c0=cout,
            weight=packs.get(w, PU_PACK_CONVT_DGRAD, k_pad, g), k_pad=k_pad, n=cin, dst0=dx, mask0=mask, cgroup=g)
    return dx


def convT3x3_wgrad(x, du, out=None):
    """dW[i][o][r][s] = sum_p x[p][i] dU_full[2p + (r, s)][o] ; db[o] = sum over du pixels."""
    B, h, wd, cin = x.shape
    _, H2, W2, cout = du.shape
    crop = _crop(h, H2)
    if out is None:
        dw = torch.empty(cin, cout, 3, 3, dtype=torch.float32, device=x.device)
        db = torch.empty(cout, dtype=torch.float32, device=x.device)
    else:
        dw, db = out
    K.wgrad(batch=B, in_hw=(H2, W2), out_hw=(h, wd), k=3, stride=2, pad=crop, rows=x, n=cin, src0=du, c0=cout,
            bias_mode=0, dweight=dw)
    K.column_sum(du.view(-1, cout), out=db)
    return dw, db


def as_nhwc_input(x):
    """Model input [B,C,H,W] -> NHWC.  C == 1 is already NHWC in memory."""
    x = x.contiguous()
    if x.shape[1] == 1:
        B, _, H, W = x.shape
        return x.view(B, H, W, 1)
    return K.nchw_to_nhwc(x)
