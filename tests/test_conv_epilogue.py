"""CPU checks of the conv epilogue matrix (tests/conv_epilogue.py; the GPU run is
test_conv_epilogue_gpu.py).

1. Plans: every row of the case table lands on the kernel it was written for - the library's
   planning queries (stand-in pointers that nothing dereferences) report the pinned plan for every
   form of the row, split with exactly the scratch the workspace query asks for and unsplit without
   it - and the rows together cover every kernel the matrix names.
2. Pair count: the (case, form) pairs are the table's product minus the explicitly excluded pairs.
3. The fp64 reference and the three bounds against ATen's own CPU arithmetic: fp32 convolution and
   epilogue, and the bf16 round-to-nearest store.  A mistake in the reference fails here.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue as E

NAMES = [c.name for c in E.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_row_plans_the_kernel_it_names(name):
    c = E.CASE[name]
    forms = [(f, ops) for f, ops in E.FORMS[c.layout].items() if E.excluded(c, ops) is None]
    assert forms
    bm, bn, mode, ks = c.plan
    M = c.B * E.geometry(c)[0][0] * E.geometry(c)[0][1]
    for fname, ops in forms:
        ptr = E.standin_ptrs(c)
        plan, need = E.plan_of(c, E.conv_args(c, ops, ptr))
        assert plan == (bm, bn, mode, 1), (fname, "no scratch", plan)
        assert need == (ks * M * c.n * 4 if ks > 1 else 0), (fname, need)
        if ks > 1:
            ws = 0x7000000
            assert E.plan_of(c, E.conv_args(c, ops, ptr, (ws, need))) == (c.plan, need), (fname, "exact scratch")
            assert E.plan_of(c, E.conv_args(c, ops, ptr, (ws, need - 1)))[0] == (bm, bn, mode, 1), (fname, "one byte short")
    if c.entry == "f32" and mode == 4:
        assert c.kernel.startswith("x6 lean") == bool(E.expect_lean(c)), "mode 4 reports x6 and x6-lean alike"
    if c.kernel.endswith("elem"):
        # vec_epi == 0 (csrc/igemm.hip vec_epilogue): an odd split column, or one operand off 16 bytes
        assert c.mis is not None or c.n0 % 4 or c.n % 4


def test_rows_cover_every_kernel_of_the_matrix():
    assert {c.kernel for c in E.CASES} == E.KERNELS
    f32 = {(c.plan[2], s) for c in E.CASES if c.entry == "f32" for s in E.splits(c)}
    assert {m for m, _ in f32} == set(range(8))
    for mode in (0, 4, 6):                               # the kernels with a split-K finish: both ways
        assert (mode, True) in f32 and (mode, False) in f32
    lean = {(c.kernel, s) for c in E.CASES if c.kernel.startswith("x6 lean") for s in E.splits(c)}
    for tile in ("128x64", "128x128", "256x128"):
        assert ("x6 lean " + tile, True) in lean and ("x6 lean " + tile, False) in lean
    b16 = {(c.plan[2], s) for c in E.CASES if c.entry == "bf16" for s in E.splits(c)}
    assert {k for k, _ in b16} == {0, 1, 2, 3}
    for kind in (0, 1):
        assert (kind, True) in b16 and (kind, False) in b16
    for entry in ("f32", "bf16"):
        assert {c.layout for c in E.CASES if c.entry == entry} == {"one", "split", "shuf"}
    # the gates of the batched epilogues (csrc/igemm.hip epilogue<>): N % 32 == 0 with a partial
    # last column block and the split inside one block; N % 32 != 0; the batched and the general shuffle
    x6 = [c for c in E.CASES if c.entry == "f32" and c.plan[2] == 4 and not c.kernel.endswith("elem")]
    assert any(c.n % 32 == 0 and c.n % c.plan[1] and c.n0 % 32 == 0 and c.n0 < c.plan[1] for c in x6)
    assert any(c.n % 32 and c.layout == "split" for c in x6)
    assert any(c.op == "convT2" and (c.n // 4) % 32 == 0 for c in x6) and any(c.op == "convT2" and (c.n // 4) % 32 for c in x6)
    assert {c.crop for c in E.CASES if c.op == "convT3"} == {0, 1}
    assert {c.mis for c in E.CASES} == {None, "bias", "dst0", "mask0"}


def test_pair_count():
    product = sum(len(E.FORMS[c.layout]) * len(E.splits(c)) for c in E.CASES)
    left_out = [(c.name, f, s) for c in E.CASES for f, ops in E.FORMS[c.layout].items() if E.excluded(c, ops)
                for s in E.splits(c)]
    pairs = E.pairs()
    assert len(pairs) == len(set(pairs)) == product - len(left_out)
    assert not set(pairs) & set(left_out)
    # what is left out, by rule: chan_scale on the bf16 entry, and the forms of a misaligned-operand
    # row that do not pass the operand; RESID never meets a split or SHUFFLE2 in the form lists
    assert all(E.CASE[n].entry == "bf16" or E.CASE[n].mis in ("bias", "mask0") for n, _, _ in left_out)
    assert not any("resid" in ops for lay in ("split", "shuf") for ops in E.FORMS[lay].values())
    assert len(E.FORMS["one"]) == 11 and len(E.FORMS["split"]) == 9 and len(E.FORMS["shuf"]) == 7


# ---- the reference and the bounds against ATen's CPU arithmetic
def _aten_epilogue32(z32, o):
    """the epilogue in fp32, one ATen operation (one rounding) per step, in the documented order"""
    f = lambda t: None if t is None else t.float()      # noqa: E731
    y = z32
    if o["bias"] is not None:
        y = y + f(o["bias"])
    if o["resid"] is not None:
        y = y + f(o["resid"])
    if o["relu"]:
        y = torch.relu(y)
    if o["mask"] is not None:
        y = torch.where(f(o["mask"]) > 0, y, torch.zeros_like(y))
    if o["scale"] is not None:
        y = y * f(o["scale"])
    if o["seed"] is not None:
        y = y + f(o["seed"])
    return y


def _aten_conv32(c, v):
    x = v["x0"] if v["x1"] is None else torch.cat([v["x0"], v["x1"]], 3)
    x = x.permute(0, 3, 1, 2)
    if c.op == "conv":
        z = F.conv2d(x, v["w"], padding=(c.k - 1) // 2)
    else:
        z = F.conv_transpose2d(x, v["w"], stride=2)[:, :, c.crop:, c.crop:]
    return z.permute(0, 2, 3, 1).contiguous()


# K = 27 ... 2304, every layout, both entries, every operand present
SELF = ["scalar loader 3->32", "x6 lean 128x64 64->64", "x6 lean 256x128 256->160 n0 96", "x6 ConvT3 32->4x16 crop1",
        "x6 ConvT2 64->4x48", "bf16 lean 64->64", "bf16 lean 128+128->64", "bf16 halo 32+32->128 n0 64",
        "bf16 ConvT2 64->4x32"]


@pytest.mark.parametrize("name", SELF)
def test_reference_and_bounds_hold_for_aten(name):
    c = E.CASE[name]
    v, ref = E.values(name), E.reference(name)
    z32 = _aten_conv32(c, v)
    worst = {}
    forms = [(f, ops) for f, ops in E.FORMS[c.layout].items() if E.excluded(c, ops) is None]
    for fname, ops in forms:
        o = E.operands(c, ops)
        y32 = _aten_epilogue32(z32, o)
        if c.entry == "f32":
            worst["gemm"] = E.gemm_ratio(z32, ref)
            worst["epilogue"] = max(worst.get("epilogue", 0.0), E.epilogue_ratio(y32, z32, o))
            E.check_exact(y32, o)
            # the identity values leave the accumulators as they are
            assert torch.equal(_aten_epilogue32(z32, E.operands(c, ops, neutral=True)), z32)
        else:
            got = y32.to(E.BF).float()                  # one round-to-nearest-even bf16 store
            worst["bf16"] = max(worst.get("bf16", 0.0), E.bf16_ratio(got, E.epilogue64(ref, o)))
            E.check_exact(got, o)
    print(name, worst)
    assert worst and all(r <= 1.0 for r in worst.values()), worst
    if c.entry == "bf16":
        assert worst["bf16"] > 0.5, "the half-ulp case of the bf16 store is reached: the bound is a tight one"


def test_bounds_reject_small_errors():
    """Each bound fails for the errors it exists to catch: a bias one channel off, a swapped mask
    element, a scale row stride of its default, an output that is one fp32 / bf16 ulp too far."""
    c = E.CASE["x6 lean 128x64 32->48 n0 16"]
    ops = E.FORMS["split"]["all"]
    o = E.operands(c, ops)
    z32 = _aten_conv32(c, E.values(c.name))
    good = _aten_epilogue32(z32, o)
    assert E.epilogue_ratio(good, z32, o) <= 1.0
    bad = dict(o, bias=o["bias"].roll(1))
    assert E.epilogue_ratio(_aten_epilogue32(z32, bad), z32, o) > 1.0
    bad = dict(o, mask=o["mask"].roll(1, 3))
    assert E.epilogue_ratio(_aten_epilogue32(z32, bad), z32, o) > 1.0
    with pytest.raises(AssertionError):
        E.check_exact(_aten_epilogue32(z32, bad), o)
    bad = dict(o, scale=E.values(c.name)["cscale"].double().reshape(-1)[:c.B * c.n].reshape(c.B, 1, 1, c.n))
    assert E.epilogue_ratio(_aten_epilogue32(z32, bad), z32, o) > 1.0
    step = torch.nextafter(good, torch.full_like(good, float("inf")))
    for _ in range(4):
        step = torch.nextafter(step, torch.full_like(good, float("inf")))
    assert E.epilogue_ratio(step, z32, o) > 1.0                   # 5 ulps of the result: past 4 roundings
    assert E.gemm_ratio(z32 * (1 + 3e-4), z32) > 1.0 and E.gemm_ratio(z32, z32.double()) == 0.0
    ref = E.reference("bf16 lean 64->64")
    rounded = ref.float().to(E.BF)
    assert E.bf16_ratio(rounded.float(), ref) <= 1.0
    up = torch.nextafter(rounded, torch.full_like(rounded, float("inf")))
    down = torch.nextafter(rounded, torch.full_like(rounded, float("-inf")))
    far = torch.where(ref > rounded.double(), down, up)             # one bf16 step away from the nearest
    assert E.bf16_ratio(far.float(), ref) > 1.0


def test_transposed_references_equal_the_conv_gradient():
    """F.conv_transpose2d is the data gradient of the strided convolution: the ConvT rows' reference
    against torch.nn.grad.conv2d_input (an independent route to the same sums)."""
    for name in ("x6 ConvT2 64->4x32", "x6 ConvT3 32->4x16 crop0", "smallx6 ConvT3 16->4x8 crop1"):
        c = E.CASE[name]
        v = E.values(name)
        x = v["x0"].double().permute(0, 3, 1, 2)
        kk = 2 if c.op == "convT2" else 3
        full = (c.B, c.n // 4, 2 * c.H + (kk - 2), 2 * c.W + (kk - 2))
        g = torch.nn.grad.conv2d_input(full, v["w"].double(), x, stride=2)     # the conv whose O x I is w's [in][out]
        g = g[:, :, c.crop:, c.crop:].permute(0, 2, 3, 1)
        assert torch.allclose(g, E.reference(name), rtol=1e-12, atol=1e-12)
