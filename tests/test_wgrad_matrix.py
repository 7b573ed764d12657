"""CPU checks of the weight-gradient matrix (tests/wgrad_matrix.py; the GPU run is
test_wgrad_matrix_gpu.py).

1. Plans: every row lands on the kernel it was written for - the library's planning queries
   (stand-in pointers that nothing dereferences) report the pinned plan and workspace for every form
   of the row, and the launcher's rule turns that plan into the instantiation the row claims.
2. Coverage: the rows claim exactly the wgrad_* GEMM instantiations of the build's resource report
   (the reducers belong to the reduction tests).  Removing a row, or adding a launch branch without
   a row, fails here.
3. Pair count: the (case, form) pairs are the table's product minus the pairs excluded by a rule.
4. The fp64 reference against ATen's own fp32 gradients (conv2d_weight, conv_transpose2d autograd).
5. Sensitivity: five mutants of the reference - the last pixel row of the last image dropped, one
   pixel counted twice at a split boundary of the plan, one tap shifted by a column, the last
   channel of src1 dropped, the bias omitted - fall outside every row's bound, while the reference
   rounded to fp32 passes it.  A mutant of one pixel changes an entry by one product of two normal
   variates, which is arbitrarily small at a few entries of a large table, so "outside" is asserted
   for the worst entry and for the majority of the entries the mutant touches, and the share is printed.
"""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))

import wgrad_matrix as W  # noqa: E402

NAMES = [c.name for c in W.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_row_plans_the_kernel_it_claims(name):
    c = W.CASE[name]
    fs = W.forms(c)
    assert fs and {f.bias for _, f in fs} == set(W.PLANS[name])
    for fname, f in fs:
        plan = W.plan_of(c, W.wgrad_args(c, f, W.standin_ptrs(f)))
        assert plan == W.PLANS[name][f.bias], (fname, plan)
        assert W.kernel_of(c, f.bias) == c.kernel, (fname, W.kernel_of(c, f.bias))
        L, Lt = W.split_len(c, f.bias)
        assert 1 <= L <= W.pixels(c) and (Lt is None or 1 <= Lt <= W.pixels(c) // 4)
    # the identity the query does not report
    if "dma" in c.kernel:
        assert c.kernel.endswith(",1>") == (c.math == 1 and W.fq(c)) and (",3,1,4," in c.kernel) == (c.math == 1)
    if c.math == 2:
        assert c.kernel.startswith("wgrad_stem_kernel") and c.kernel.endswith(",1>")


def _built():
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    return {W.demangle(sym) for sym in d["kernels"] if "wgrad_" in sym}


def test_rows_claim_every_wgrad_kernel_of_the_build():
    built = _built()
    assert W.REDUCERS <= built, "reducers missing from the build: %s" % sorted(W.REDUCERS - built)
    gemm = built - W.REDUCERS
    claimed = {c.kernel for c in W.CASES}
    assert not gemm - claimed, "kernels in the build that no row reaches: %s" % sorted(gemm - claimed)
    assert not claimed - gemm, "rows claim kernels the build lacks: %s" % sorted(claimed - gemm)
    assert len(gemm) >= 55


def test_rows_cover_the_forms_of_each_family():
    """what the issue's table asks of the rows beyond one per instantiation"""
    by = lambda pre: [c for c in W.CASES if c.kernel.startswith(pre)]      # noqa: E731
    # stem: fp32 rows under math 0 and 1, bf16 rows under math 2, more than one 16 x 64 tile each way
    assert {c.math for c in by("wgrad_stem")} == {0, 1, 2}
    assert all(any(c.H > 16 and c.W > 64 for c in by("wgrad_stem") if (c.math == 2) == b) for b in (False, True))
    # small: every C through one source and, where it can be split in 4-multiples, through two
    for C in (8, 12, 16):
        assert {bool(c.c1) for c in by("wgrad_small_kernel<%d," % C)} == {False, True}
    # dma: the five tiles in three forms, 128 x 256 in two; non-FQ through all four geometries
    for bn, bk in ((64, 64), (64, 128), (32, 128), (64, 192), (128, 128), (128, 256)):
        want = {W.dma(bn, bk, 1, True), W.dma(bn, bk, 1, False)} | ({W.dma(bn, bk, 0)} if bk != 256 and bn != 32 else set())
        assert want <= {c.kernel for c in W.CASES}, (bn, bk)
    nofq = [c for c in by("wgrad_dma") if c.math == 1 and not W.fq(c)]
    assert {c.op for c in nofq} == {"conv", "T2", "T3c0", "T3c1"} and any(c.op == "conv" and c.W < 4 for c in nofq)
    # register-staged: c0 % 4 != 0, c0 % 4 == 0 with c1 % 4 != 0, a ConvT row with bias row N
    reg = by("wgrad_kernel<")
    assert any(c.c0 % 4 for c in reg) and any(c.c0 % 4 == 0 and c.c1 % 4 for c in reg)
    assert any(c.op == "T2" and 2 in W.PLANS[c.name] for c in reg)
    # halo: odd heights on the fp32 entry, two sources, and a row whose ring wraps (>= 4 stages per split)
    for pre in ("wgrad_halo_x6_kernel", "wgrad_halo_bf16_kernel"):
        rows = by(pre)
        assert any(c.c1 for c in rows)
        assert any(W.split_len(c, 1)[0] >= 64 for c in rows), pre
    assert all(c.H % 2 and c.W % 16 == 0 for c in by("wgrad_halo_x6_kernel"))
    # Winograd: one tile, a ragged last stage, two sources; the column form at its gate
    wino = by(W.WINO)
    assert any(W.pixels(c) == 4 for c in wino) and any((W.pixels(c) // 4) % 16 for c in wino) and any(c.c1 for c in wino)
    assert any((c.B, c.H, c.W, c.c0, c.c1, c.n) == (2, 32, 32, 128, 0, 128) for c in by(W.COLS)) and any(c.c1 for c in by(W.COLS))
    # ragged edges of the tiled GEMM kernels: a partial last stage, a partial last split, K % BK, n % BN
    for pre, stage in (("wgrad_dma", 16), ("wgrad_kernel<", 16), ("wgrad_bf16_kernel", 32)):
        rows = [(c, W.PLANS[c.name][max(W.PLANS[c.name])]) for c in by(pre)]
        assert any(W.pixels(c) % stage for c, _ in rows), pre
        assert any(p[3] > 1 and W.pixels(c) % W.split_len(c, max(W.PLANS[c.name]))[0] for c, p in rows), pre
        assert any((W.geometry(c)[2] ** 2 * (c.c0 + c.c1)) % p[1] for c, p in rows), pre
        assert any(c.n % p[0] for c, p in rows), pre
    # no row is larger than the column plan's gate in pixels but the two whose ring must wrap
    assert all(W.pixels(c) <= 2048 or "ring wrap" in c.name for c in W.CASES)


def test_pair_count():
    product = sum(len(W.FORMS[c.layout]) for c in W.CASES)
    left_out = [(c.name, nm, W.excluded(c, f)) for c in W.CASES for nm, f in W.FORMS[c.layout].items() if W.excluded(c, f)]
    pairs = W.pairs()
    assert len(pairs) == len(set(pairs)) == product - len(left_out) == W.PAIR_COUNT
    assert all(isinstance(why, str) and why for _, _, why in left_out)          # every exclusion cites its rule
    assert not set(pairs) & {(n, f) for n, f, _ in left_out}
    assert len(W.FORMS["conv"]) == 6 and len(W.FORMS["convT"]) == 6
    # both paths of every reducer with two are run
    paths = {W.reducer(W.CASE[n], W.FORMS[W.CASE[n].layout][f].bias, W.FORMS[W.CASE[n].layout][f].view) for n, f in pairs}
    assert paths == {"wide", "transposed", "quad", "cols vec", "cols scalar"}


# ---- the reference against ATen's fp32 gradients
SELF = ["stem 1->8", "pw 4->8", "small 8+4->16", "wino 64+64->128, 30 tiles", "halo<2> 64+64->128", "dma 64x64 out_w 3",
        "dma 64x64 ConvT2", "dma 128x256 ConvT2 64->128", "dma 64x128 ConvT3 crop 0", "dma 32x128 ConvT3 crop 1",
        "reg 64x64 ConvT2 6->64", "reg 64x256 8+6->40 m0", "bf16 32+24->40", "bf16 ConvT3 crop 1"]


@pytest.mark.parametrize("name", SELF)
def test_reference_equals_aten(name):
    c = W.CASE[name]
    v = W.values(name)
    (ih, iw), (oh, ow), k, st, pad = W.geometry(c)
    C = c.c0 + c.c1
    src = (v["src0"] if v["src1"] is None else torch.cat([v["src0"], v["src1"]], 3)).permute(0, 3, 1, 2).contiguous()
    rows = v["rows"].permute(0, 3, 1, 2).contiguous()
    bias = max(W.PLANS[name])
    ref = W.reference(name, bias)
    if c.layout == "conv":
        dw = torch.nn.grad.conv2d_weight(src, (c.n, C, k, k), rows, stride=st, padding=pad)
        db = rows.sum((0, 2, 3))
    else:
        w = torch.zeros(c.n, C, k, k, requires_grad=True)
        b = torch.zeros(C, requires_grad=True)
        F.conv_transpose2d(rows, w, b, stride=2)[:, :, pad:pad + ih, pad:pad + iw].backward(src)
        dw, db = w.grad, b.grad
    cc = W.pixels(c) + 2                    # ATen's order is its own: one fp32 chain over all M pixels
    r = W.ratio(dw, ref.dw, ref.mag_w, cc).max().item()
    print(name, "dweight %.3g of the bound" % r)
    assert r <= 1.0
    if bias:
        rb = W.ratio(db, ref.db, ref.mag_b, (9 if bias == 2 else 1) * W.pixels(c) + 2).max().item()
        assert rb <= 1.0, rb


def test_winograd_magnitude_bounds_the_plain_one():
    """|G|^T [...] |G| over absolute values is no smaller than sum |P| |X|: G^T (A . A^T) (.) (B^T . B) G
    reproduces every product of the direct sum, and with absolute values nothing cancels."""
    for name in ("wino one tile", "wino 64+64->128, 30 tiles"):
        c = W.CASE[name]
        rows, src = W.operands64(c)
        plain = W._grads(c, rows.abs(), src.abs(), 0)[0].reshape(-1)
        assert bool((W.reference(name, 0).mag_w >= plain * (1 - 1e-12)).all())
        # and the signed expression is the gradient itself
        signed = W._wino_signed(c, rows, src).reshape(-1)
        assert torch.allclose(signed, W.reference(name, 0).dw, rtol=1e-10, atol=1e-10)


# ---- sensitivity
def _applies(c, bias, mutant):
    return not (mutant == "drop_src1" and not c.c1) and not (mutant == "no_bias" and not bias)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_reject_the_mutants(name):
    c = W.CASE[name]
    bias = max(W.PLANS[name])
    ref = W.reference(name, bias)
    cw, cb = W.bound_c(c, bias), W.bias_c(c, bias)
    assert W.ratio(ref.dw.float(), ref.dw, ref.mag_w, cw).max().item() <= 1.0
    if bias:
        assert W.ratio(ref.db.float(), ref.db, ref.mag_b, cb).max().item() <= 1.0
    for mutant in W.MUTANTS:
        if not _applies(c, bias, mutant):
            continue
        dw, db = W.mutated(name, bias, mutant)
        if mutant == "no_bias":
            got, exact, mag, cc = db, ref.db, ref.mag_b, cb
        else:
            got, exact, mag, cc = dw, ref.dw, ref.mag_w, cw
        touched = (got.reshape(-1) - exact.reshape(-1)).abs() > 1e-9 * mag.reshape(-1)
        assert bool(touched.any()), mutant
        r = W.ratio(got.float(), exact, mag, cc)[touched]
        share = (r > 1.0).double().mean().item()
        print("%s | %s: %d entries touched, worst %.3g x the bound, %.1f %% outside" % (name, mutant, int(touched.sum()),
                                                                                      r.max().item(), 100 * share))
        assert r.max().item() > 1.0 and share > 0.5, (mutant, r.max().item(), share)
