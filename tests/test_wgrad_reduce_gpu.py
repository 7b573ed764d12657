"""Phase 2 of the weight gradients (csrc/wgrad.hip: wgrad_reduce) against the slab it reads.

Phase 1 of pu_wgrad / pu_wgrad_bf16 leaves `splits` partial [Nr][Kcp] tiles in the workspace;
phase 2 sums them in fp64 in a fixed order and stores the fp32 result as dweight[n][c][kh][kw]
(+ dbias).  Each case runs phase 1 once, reads the slab back and checks phase 2 against the slab's
own fp64 sum, so the test does not depend on the GEMM kernels' arithmetic.

Tolerance (derived, not measured): the kernel and torch each sum at most 1024 fp32 values in fp64,
in different orders; each order is off the exact sum by at most (count - 1) * 2^-53 * sum|x|, so
the two differ by less than 2^-42 * sum|x|, and 2^-40 leaves a factor of four.  The kernel's
fp32 result may then sit one fp32 rounding away from the rounded reference:
    |got - float32(ref)| <= ulp32(ref) + 2^-40 * sum_z |slab_z|      for every entry.
accumulate = 1 is one fp32 addition per entry, so it equals torch.add bit for bit.

The cases name the finisher each plan takes (wide one-launch kernel, transposed finisher, quad
finisher; on the fp32 slab when the plan has one reduction group, on the fp64 partials of
wgrad_sum_splits4_kernel when it has several) and assert the plan, so a planner change that moves
a case off its kernel fails here instead of silently testing something else.  Every wide plan has
N * Kcp a multiple of 16 (n % 4 == 0 and Kcp % 4 == 0), so the wide kernel's last 16-entry block
is never partial and no case can make it so.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from punet import kernels as K  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def same(B, H, W, c0, c1, n, k=3):
    """k x k / stride 1 / 'same' padding conv: rows = dZ [B,H,W,n], sources [B,H,W,c]."""
    return dict(batch=B, in_hw=(H, W), out_hw=(H, W), k=k, stride=1, pad=(k - 1) // 2, n=n, c0=c0, c1=c1)


def convT(B, h, cin, cout):
    """ConvT 2x2 / stride 2: rows = x [B,h,h,cin], source = dU [B,2h,2h,cout], bias from row N."""
    return dict(batch=B, in_hw=(2 * h, 2 * h), out_hw=(h, h), k=2, stride=2, pad=0, n=cin, c0=cout, c1=0)


# name: (geometry, bf16, bias_mode, dweight one float off alignment, loader kind, splits, groups)
# kind: pu_wgrad_tile's loader kind, or pu_wgrad_bf16_tile's halo flag for the bf16 cases
CASES = {
    # wide kernel, direct plans.  270 splits over 64 lanes: lanes 0..13 sum 5 (4-round + 1), the rest 4
    "wide_small_270": (same(5, 129, 161, 4, 0, 4), False, 1, False, 2, 270, 16),
    "wide_small_4": (same(1, 20, 36, 8, 0, 8), False, 0, False, 2, 4, 1),          # < 64 splits, no bias column
    "wide_pointwise": (same(3, 40, 56, 3, 0, 8, k=1), False, 1, False, 6, 27, 4),
    "wide_stem": (same(2, 37, 70, 1, 0, 16), False, 1, False, 4, 12, 2),
    # wide kernel, GEMM plans of at most 16384 entries
    "wide_gemm_b1": (same(2, 16, 16, 32, 0, 32), False, 1, False, 1, 2, 1),
    "wide_gemm_b0": (same(2, 16, 16, 32, 0, 32), False, 0, False, 1, 2, 1),
    "wide_gemm_bf16_b1": (same(2, 16, 16, 32, 0, 32), True, 1, False, 0, 1, 1),
    "wide_gemm_bf16_b0": (same(2, 16, 16, 32, 0, 32), True, 0, False, 0, 1, 1),
    # transposed finisher on the slab: 6 splits = one 4-round + 2
    "t_slab_6": (same(3, 8, 16, 128, 0, 256), False, 1, False, 5, 6, 1),
    # sum_splits4 + transposed finisher: 44 splits in 6 groups of 8, 8, 7, 7, 7, 7
    "t_groups_wino": (same(11, 16, 16, 64, 0, 64), False, 1, False, 5, 44, 6),
    "t_groups_halo_bf16": (same(11, 16, 16, 64, 0, 64), True, 1, False, 1, 176, 8),   # 8 groups of 22
    # quad finisher, ConvT (bias mode 2: the bias is row N summed over the taps)
    "q_convT_2": (convT(2, 16, 16, 16), False, 2, False, 1, 2, 1),    # bias: 8 terms, one 8-round
    "q_convT_3": (convT(3, 16, 16, 16), False, 2, False, 1, 3, 1),    # bias: 12 terms, 8-round + 4 on chain 0
    "q_convT_9": (convT(9, 16, 16, 16), False, 2, False, 1, 9, 2),    # sum_splits4 (5, 4) + 2 partials
    # quad finisher on a dweight the transposed finisher refuses (a view into a flat gradient)
    "q_view_b1": (same(2, 9, 13, 64, 64, 64), False, 1, True, 1, 1, 1),
    "q_view_b0": (same(2, 9, 13, 64, 64, 64), False, 0, True, 1, 1, 1),
    "q_view_groups": (same(20, 9, 13, 64, 64, 64), False, 1, True, 1, 10, 2),       # 2 groups of 5
    "q_view_slab_14": (same(7, 8, 16, 128, 0, 256), False, 1, True, 5, 14, 1),     # 8-round + 4-round + 2
}


def _int():
    return ctypes.c_int()


@functools.lru_cache(maxsize=None)
def reduced(name):
    """Run the case once: the plan, the slab of phase 1, phase 2 into NaN-filled outputs and phase 2
    with accumulate onto seeded outputs (all read back to the CPU)."""
    geo, bf16, bias_mode, view, _, _, _ = CASES[name]
    B, (Hi, Wi), (Ho, Wo) = geo["batch"], geo["in_hw"], geo["out_hw"]
    n, c0, c1, k = geo["n"], geo["c0"], geo["c1"], geo["k"]
    C, taps = c0 + c1, k * k
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    dt = torch.bfloat16 if bf16 else torch.float32
    rows = torch.randn(B, Ho, Wo, n, generator=g).to(DEV, dt)
    src0 = torch.randn(B, Hi, Wi, c0, generator=g).to(DEV, dt)
    src1 = torch.randn(B, Hi, Wi, c1, generator=g).to(DEV, dt) if c1 else None
    seed_w = torch.randn(n * C * taps, generator=g)
    seed_b = torch.randn(C if bias_mode == 2 else n, generator=g)

    L = K.lib()
    tile, ws_bytes, phase = ((L.pu_wgrad_bf16_tile, L.pu_wgrad_bf16_workspace_bytes, L.pu_wgrad_bf16_phase) if bf16
                             else (L.pu_wgrad_tile, L.pu_wgrad_workspace_bytes, L.pu_wgrad_phase))
    nw = n * C * taps
    off = 1 if view else 0

    def outputs(fill_w, fill_b):
        buf = torch.full((nw + 8,), NAN, device=DEV)           # torch allocations are 16-byte aligned
        buf[off:off + nw] = fill_w.to(DEV) if torch.is_tensor(fill_w) else fill_w
        db = torch.full((len(seed_b),), NAN, device=DEV)
        db[:] = fill_b.to(DEV) if torch.is_tensor(fill_b) else fill_b
        return buf, db

    def args(buf, db, accumulate):
        return K.wgrad_args(rows=rows.data_ptr(), src0=src0.data_ptr(), src1=None if src1 is None else src1.data_ptr(),
                            bias_mode=bias_mode, dweight=buf.data_ptr() + 4 * off,
                            dbias=db.data_ptr() if bias_mode else None, accumulate=accumulate,
                            math=0 if bf16 else None, **geo)

    buf, db = outputs(NAN, NAN)
    a = args(buf, db, False)
    assert (buf.data_ptr() + 4 * off) % 16 == 4 * off
    bn, bk, kind, splits = _int(), _int(), _int(), _int()
    K.check(tile(ctypes.byref(a), ctypes.byref(bn), ctypes.byref(bk), ctypes.byref(kind), ctypes.byref(splits)), "tile")
    nbytes = ws_bytes(ctypes.byref(a))
    Nr = n + (bias_mode == 2)
    Kc = taps * C + (bias_mode == 1)
    Kcp = (Kc + 3) // 4 * 4
    slab_floats = splits.value * Nr * Kcp
    # the workspace is the slab (to 256 bytes) plus, for G > 1 groups, G fp64 [Nr][Kcp] partials
    part_bytes = nbytes - (4 * slab_floats + 255) // 256 * 256
    assert part_bytes % (8 * Nr * Kcp) == 0
    groups = part_bytes // (8 * Nr * Kcp) or 1

    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    K.check(phase(ctypes.byref(a), ws.data_ptr(), nbytes, 1, K._stream()), "phase 1")
    slab = ws[:slab_floats].view(splits.value, Nr, Kcp).cpu()
    K.check(phase(ctypes.byref(a), ws.data_ptr(), nbytes, 2, K._stream()), "phase 2")
    buf_acc, db_acc = outputs(seed_w, seed_b)
    a_acc = args(buf_acc, db_acc, True)
    K.check(phase(ctypes.byref(a_acc), ws.data_ptr(), nbytes, 2, K._stream()), "phase 2, accumulate")
    torch.cuda.synchronize()
    # bitwise: the pad columns Kc .. Kcp keep the NaN fill (no kernel may read them into a result)
    assert torch.equal(ws[:slab_floats].cpu().view(torch.int32), slab.view(torch.int32).view(-1)), "phase 2 wrote into the slab"
    return dict(kind=kind.value, splits=splits.value, groups=groups, slab=slab, Nr=Nr, Kcp=Kcp, K=taps * C,
                buf=buf.cpu(), db=db.cpu(), buf_acc=buf_acc.cpu(), db_acc=db_acc.cpu(), seed_w=seed_w, seed_b=seed_b,
                off=off, nw=nw)


def expected(name, r):
    """(reference, sum of magnitudes) in fp64 for dweight (flat [n][c][kh][kw]) and dbias, from the slab."""
    geo, _, bias_mode, _, _, _, _ = CASES[name]
    n, C, taps = geo["n"], geo["c0"] + geo["c1"], geo["k"] ** 2
    s = r["slab"].double()
    out = []
    for t in (s.sum(0), s.abs().sum(0)):
        # dweight[n][c][r][ss] is entry [n][tap * C + c] of the summed slab, tap = r * kw + ss
        w = t[:n, :r["K"]].reshape(n, taps, C).permute(0, 2, 1).reshape(-1)
        if bias_mode == 1:
            b = t[:n, r["K"]]
        elif bias_mode == 2:
            b = t[n, :r["K"]].reshape(taps, C).sum(0)
        else:
            b = None
        out.append((w, b))
    return out


def ulp32(ref32):
    a = ref32.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def assert_sum(got, ref, mag, what):
    ref32 = ref.float()
    err = (got.double() - ref32.double()).abs()
    bound = ulp32(ref32) + 2.0 ** -40 * mag
    ok = err <= bound                                       # a NaN in got fails this
    print("%s: %d entries, max err / bound = %.3g" % (what, got.numel(), (err / bound).nan_to_num(nan=1e30).max()))
    assert bool(ok.all()), "%s: %d of %d entries off the slab's sum (first %d)" % (
        what, int((~ok).sum()), ok.numel(), int((~ok).nonzero()[0]))


@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_one_the_case_is_for(name):
    _, _, _, _, kind, splits, groups = CASES[name]
    r = reduced(name)
    assert (r["kind"], r["splits"], r["groups"]) == (kind, splits, groups)
    assert 1 <= r["splits"] <= 1024


@pytest.mark.parametrize("name", list(CASES))
def test_reduction_equals_the_slab_sum(name):
    """Every dweight / dbias entry against the fp64 sum of the slab phase 2 read; the words around a
    misaligned dweight view stay NaN."""
    bias_mode = CASES[name][2]
    r = reduced(name)
    (w_ref, b_ref), (w_mag, b_mag) = expected(name, r)
    off, nw = r["off"], r["nw"]
    assert_sum(r["buf"][off:off + nw], w_ref, w_mag, name + " dweight")
    assert bool(r["buf"][:off].isnan().all()) and bool(r["buf"][off + nw:].isnan().all()), "guard words written"
    if bias_mode:
        assert_sum(r["db"], b_ref, b_mag, name + " dbias")
    else:
        assert bool(r["db"].isnan().all())


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_is_one_fp32_add(name):
    """accumulate = 1 onto seeded gradients equals torch.add(seed, the plain result) bit for bit."""
    bias_mode = CASES[name][2]
    r = reduced(name)
    off, nw = r["off"], r["nw"]
    assert torch.equal(r["buf_acc"][off:off + nw], torch.add(r["seed_w"], r["buf"][off:off + nw]))
    assert bool(r["buf_acc"][:off].isnan().all()) and bool(r["buf_acc"][off + nw:].isnan().all())
    if bias_mode:
        assert torch.equal(r["db_acc"], torch.add(r["seed_b"], r["db"]))
    else:
        assert torch.equal(r["db_acc"], r["seed_b"])
