"""Phase 2 of the column plans (csrc/wgrad.hip: wgrad_finish_cols_kernel) against the slab it reads,
in the manner of tests/test_wgrad_reduce_gpu.py.

Phase 1 leaves `splits` = 4 x (tile splits) pages [Nr][Kcp] in the workspace, Kc = 3 C (+ 1 bias
column); page 4 z + j holds R[r][j] = sum_a G[a][r] M[a][j] of tile split z at column r C + c.
Phase 2 finishes the transform per split in fp32, in wgrad_wino_x6_kernel's order,
    P0 = (R0 + R1 / 2, R1 / 2, R1 / 2),  P1 = (R2 / 2, -R2 / 2, R2 / 2 + R3),  dW_z[r][s] = P0[s] + P1[s],
sums the splits in fp64 and rounds once; dbias[n] is the sum of column 1's column 3 C.  Each case
runs phase 1 once, reads the slab back, forms dW_z in torch fp32 (the same IEEE operations) and
sums it in fp64.

Tolerance (derived in tests/test_wgrad_reduce_gpu.py): kernel and torch sum the same fp32 values in
fp64 in different orders, so
    |got - float32(ref)| <= ulp32(ref) + 2^-40 * sum_z |dW_z|,
valid while no chain sums more than 1024 values; the longest here sums 32.

The workspace is NaN-filled before phase 1, so every column no block writes (the pad columns
Kc .. Kcp of every page, and the bias column of the pages of columns 0, 2 and 3) is NaN when
phase 2 runs: a finite result shows that nothing unwritten is read into it.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from punet import kernels as K  # noqa: E402

DEV = "cuda"
NAN = float("nan")

# name: ((B, H, W, c0, c1, n), bias_mode, dweight one float off alignment, splits, workspace bytes beyond the slab)
# The finisher follows the reduction groups of the 64 x 64 plan of the same call: one group for the
# cases whose 64 x 64 slab page has 262144 entries or more, two (splits z = 0, 2, ... and 1, 3, ...) for 128 -> 128.
CASES = {
    "cols_g1": ((2, 32, 32, 512, 0, 256), 1, False, 32, 0),         # one group: 8 splits per entry
    "cols_g1_cat": ((2, 32, 32, 128, 128, 128), 1, False, 128, 0),  # one group of 32 splits, two sources
    "cols_g2": ((2, 32, 32, 128, 0, 128), 1, False, 128, 0),        # two groups of 16
    "cols_g2_odd": ((3, 24, 30, 128, 0, 128), 1, False, 136, 0),    # 34 splits: two groups of 17 (4-rounds + 1)
    "cols_g2_b0": ((2, 32, 32, 128, 0, 128), 0, False, 128, 0),     # no bias column
    "cols_view_g2": ((2, 32, 32, 128, 0, 128), 1, True, 128, 0),    # scalar stores: a view into a flat gradient
    "cols_view_g1": ((2, 32, 32, 512, 0, 256), 0, True, 32, 0),
}


@functools.lru_cache(maxsize=None)
def reduced(name):
    (B, H, W, c0, c1, n), bias_mode, view, _, _ = CASES[name]
    C = c0 + c1
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rows = torch.randn(B, H, W, n, generator=g).to(DEV)
    src0 = torch.randn(B, H, W, c0, generator=g).to(DEV)
    src1 = torch.randn(B, H, W, c1, generator=g).to(DEV) if c1 else None
    nw = n * C * 9
    seed_w, seed_b = torch.randn(nw, generator=g), torch.randn(n, generator=g)
    off = 1 if view else 0

    def outputs(fill_w, fill_b):
        buf = torch.full((nw + 8,), NAN, device=DEV)
        buf[off:off + nw] = fill_w.to(DEV) if torch.is_tensor(fill_w) else fill_w
        db = torch.full((n,), NAN, device=DEV)
        db[:] = fill_b.to(DEV) if torch.is_tensor(fill_b) else fill_b
        return buf, db

    def args(buf, db, accumulate):
        return K.wgrad_args(batch=B, in_hw=(H, W), out_hw=(H, W), k=3, stride=1, pad=1, rows=rows.data_ptr(), n=n,
                            src0=src0.data_ptr(), c0=c0, src1=None if src1 is None else src1.data_ptr(), c1=c1,
                            bias_mode=bias_mode, dweight=buf.data_ptr() + 4 * off,
                            dbias=db.data_ptr() if bias_mode else None, accumulate=accumulate)

    L = K.lib()
    buf, db = outputs(NAN, NAN)
    a = args(buf, db, False)
    bn, bk, kind, splits = (ctypes.c_int() for _ in range(4))
    K.check(L.pu_wgrad_tile(ctypes.byref(a), *(ctypes.byref(v) for v in (bn, bk, kind, splits))), "tile")
    assert (bn.value, bk.value, kind.value) == (128, 384, 5), "not a column plan"
    nbytes = L.pu_wgrad_workspace_bytes(ctypes.byref(a))
    Kc = 3 * C + (bias_mode == 1)
    Kcp = (Kc + 3) // 4 * 4
    slab_floats = splits.value * n * Kcp
    extra = nbytes - (4 * slab_floats + 255) // 256 * 256

    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    K.check(L.pu_wgrad_phase(ctypes.byref(a), ws.data_ptr(), nbytes, 1, K._stream()), "phase 1")
    slab = ws[:slab_floats].view(splits.value // 4, 4, n, Kcp).cpu()
    K.check(L.pu_wgrad_phase(ctypes.byref(a), ws.data_ptr(), nbytes, 2, K._stream()), "phase 2")
    buf_acc, db_acc = outputs(seed_w, seed_b)
    a_acc = args(buf_acc, db_acc, True)
    K.check(L.pu_wgrad_phase(ctypes.byref(a_acc), ws.data_ptr(), nbytes, 2, K._stream()), "phase 2, accumulate")
    torch.cuda.synchronize()
    assert torch.equal(ws[:slab_floats].cpu().view(torch.int32), slab.view(torch.int32).view(-1)), "phase 2 wrote into the slab"
    # what phase 1 must have written, and nothing else
    assert bool(slab[..., :3 * C].isfinite().all()), "unwritten R entries"
    assert bool(slab[..., Kc:].isnan().all()), "pad columns written"
    if bias_mode:
        assert bool(slab[:, 1, :, 3 * C].isfinite().all()) and bool(slab[:, (0, 2, 3), :, 3 * C].isnan().all())
    return dict(splits=splits.value, extra=extra, slab=slab, C=C, n=n, buf=buf.cpu(), db=db.cpu(),
                buf_acc=buf_acc.cpu(), db_acc=db_acc.cpu(), seed_w=seed_w, seed_b=seed_b, off=off, nw=nw)


def expected(r, bias_mode):
    """(reference, sum of magnitudes) in fp64 for dweight (flat [n][c][r][s]) and dbias."""
    n, C = r["n"], r["C"]
    s = r["slab"]                                                          # [z][j][n][Kcp] fp32
    R = s[..., :3 * C].reshape(-1, 4, n, 3, C)                             # [z][j][n][r][c]
    R0, R1, R2, R3 = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
    h1, h2 = 0.5 * R1, 0.5 * R2                                            # fp32, as the kernel
    dwz = torch.stack([(R0 + h1) + h2, h1 + (-0.5 * R2), h1 + (h2 + R3)], -1)   # [z][n][r][c][s]
    assert dwz.dtype == torch.float32
    dwz = dwz.permute(0, 1, 3, 2, 4).double()                              # [z][n][c][r][s]
    out = []
    for mag in (False, True):
        w = (dwz.abs() if mag else dwz).sum(0).reshape(-1)
        b = None
        if bias_mode:
            col = s[:, 1, :, 3 * C].double()
            b = (col.abs() if mag else col).sum(0)
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
    assert bool(ok.all()), "%s: %d of %d entries off the slab's combination (first %d)" % (
        what, int((~ok).sum()), ok.numel(), int((~ok).nonzero()[0]))


@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_one_the_case_is_for(name):
    _, _, _, splits, extra = CASES[name]
    r = reduced(name)
    assert (r["splits"], r["extra"]) == (splits, extra)
    assert r["splits"] // 4 <= 1024


@pytest.mark.parametrize("name", list(CASES))
def test_reduction_equals_the_finished_slab(name):
    bias_mode = CASES[name][1]
    r = reduced(name)
    (w_ref, b_ref), (w_mag, b_mag) = expected(r, bias_mode)
    off, nw = r["off"], r["nw"]
    assert_sum(r["buf"][off:off + nw], w_ref, w_mag, name + " dweight")
    assert bool(r["buf"][:off].isnan().all()) and bool(r["buf"][off + nw:].isnan().all()), "guard words written"
    if bias_mode:
        assert_sum(r["db"], b_ref, b_mag, name + " dbias")
    else:
        assert bool(r["db"].isnan().all())


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_is_one_fp32_add(name):
    bias_mode = CASES[name][1]
    r = reduced(name)
    off, nw = r["off"], r["nw"]
    assert torch.equal(r["buf_acc"][off:off + nw], torch.add(r["seed_w"], r["buf"][off:off + nw]))
    assert bool(r["buf_acc"][:off].isnan().all()) and bool(r["buf_acc"][off + nw:].isnan().all())
    if bias_mode:
        assert torch.equal(r["db_acc"], torch.add(r["seed_b"], r["db"]))
    else:
        assert torch.equal(r["db_acc"], r["seed_b"])
