"""CPU checks of the layer matrix (tests/layer_matrix.py; the GPU run is test_layer_matrix_gpu.py).

1. Plans: every row lands on the kernels it was written for - the launcher's rule (kernel_of) applied
   to the row's arguments gives the instantiations the row claims, and the BatchNorm split count, the
   outconv block counts and the workspace sizes are those the library's queries report.
2. Coverage: the rows claim exactly the kernels of csrc/norm.hip and csrc/elementwise.hip in the
   build's resource report, the weight packers aside.  Removing a row, or adding a launch branch
   without a row, fails here.
3. Pair count: the (row, form) pairs are the table's product minus the pairs excluded by a rule.
4. The references against ATen on the CPU wherever ATen defines the operation: BatchNorm2d slot by
   slot (forward, running statistics, backward), F.interpolate and its autograd, F.max_pool2d and its
   autograd (the NaN and -inf rows included), F.conv2d 1x1 and its autograd.
5. Sensitivity: every mutant of MUTANTS falls outside the bound on every (row, form) it applies to,
   while the reference rounded to the output's type passes it.  A mutant can touch an entry by
   arbitrarily little (a tie that routes the same gradient, a product of two small variates), so
   "outside" is asserted for at least one touched entry per pair; the worst ratio and the share of
   touched entries outside are printed.
"""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))

import layer_matrix as M  # noqa: E402
from wgrad_matrix import demangle  # noqa: E402

NAMES = [r.name for r in M.CASES]
F64 = torch.float64


@pytest.mark.parametrize("name", NAMES)
def test_row_launches_the_kernels_it_claims(name):
    r = M.CASE[name]
    assert M.forms(r)
    assert M.kernel_of(r) == r.kernels, sorted(M.kernel_of(r))
    if M.pinned(r) is not None:
        assert M.plan_of(r) == M.pinned(r), M.plan_of(r)
    p = r.p
    if r.entry in ("bn_fwd", "bn_bwd"):
        assert M.bn_plan(p.B, p.hw, p.C)[1] == p.S and p.ws == 16 * p.S * p.B * p.C + 8 * p.B * p.C
    if r.entry == "oc_bwd":
        assert p.ws == 4 * M.OC_BLOCKS * (p.C + 1)
    if r.entry == "colsum":
        assert p.ws == 8 * p.nb * p.cols


def _built():
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    return {demangle(sym) for sym, k in d["kernels"].items() if k["source"] in M.SOURCES}


def test_rows_claim_every_kernel_of_the_two_files():
    built = _built()
    assert M.PACKERS <= built, "packers missing from the build: %s" % sorted(M.PACKERS - built)
    layer = built - M.PACKERS
    claimed = set().union(*(r.kernels for r in M.CASES))
    assert not layer - claimed, "kernels in the build that no row reaches: %s" % sorted(layer - claimed)
    assert not claimed - layer, "rows claim kernels the build lacks: %s" % sorted(claimed - layer)
    assert len(layer) == 42


def test_rows_cover_the_branches():
    """the branches of the launchers beyond one row per instantiation"""
    by = lambda e: [r for r in M.CASES if r.entry == e]      # noqa: E731
    bn = by("bn_fwd")
    assert {12, 24, 48} <= {r.p.C for r in bn} and all(256 % c for c in (12, 24, 48))      # idle tail threads
    assert any(r.p.C > 64 and r.p.C % 64 for r in bn)                                      # a partial channel block
    assert any(r.p.S == 64 for r in bn) and any(r.p.S > 1 and r.p.hw % r.p.S for r in bn)
    assert any(r.p.hw == 1 for r in bn) and any(r.p.data == "edge" for r in bn)
    assert {(r.p.B, r.p.hw, r.p.C) for r in by("bn_bwd")} == {(r.p.B, r.p.hw, r.p.C) for r in bn}
    assert all(r.p.B > 1 for r in by("bn_eval"))                                           # [C], not [B, C]
    for e in ("up_fwd", "up_bwd"):
        hw = {(r.p.h, r.p.w) for r in by(e)}
        assert any(h == 1 and w == 1 for h, w in hw) and any(h == 1 < w for h, w in hw) and any(w == 1 < h for h, w in hw)
        assert any(h == 2 for h, w in hw) and any(h > 2 and w > 2 for h, w in hw)
    for e in ("pool_fwd", "pool_bwd"):
        for dt in ("f32", "bf16"):
            rows = [r for r in by(e) if r.p.dt == dt]
            assert any(r.p.special and r.p.H % 2 == 0 for r in rows) and any(r.p.special and r.p.H % 2 for r in rows)
        assert any(r.p.dt == "bf16" and r.p.C % 8 for r in by(e)) and any(r.p.dt == "bf16" and r.p.H % 2 for r in by(e))
    assert {r.p.mis for r in by("pool_fwd")} >= {"x", "y", "scale"} and {r.p.mis for r in by("pool_bwd")} >= {"x", "dy", "dx"}
    ob = by("oc_bwd")
    for dt in ("f32", "bf16"):
        for L in (2, 4, 8):           # every narrow kernel: under the block cap, and more than one sweep of it
            rows = [r for r in ob if r.p.dt == dt and r.p.C == 4 * L]
            assert any(r.p.blocks < M.OC_BLOCKS for r in rows)
            assert any(r.p.rows > M.OC_BLOCKS * (256 // L) and r.p.rows % (256 // L) for r in rows), (dt, L)
        assert any(r.p.dt == dt and r.p.C == 96 for r in ob) and any(r.p.dt == dt and r.p.C == 64 for r in ob)
    second = [r for r in ob if r.p.C in (8, 16, 32) and r.p.rows > M.OCN_U * M.OC_BLOCKS * (1024 // r.p.C)]
    assert {r.p.C for r in second} == {8, 32}                                              # the unroll's second trip
    assert any(r.p.C not in (8, 16, 32) and r.p.rows > 16 * M.OC_BLOCKS for r in ob)
    of = by("oc_fwd")
    assert {r.p.mis for r in of if r.p.C % 4 == 0} >= {"x", "w", None} and any(r.p.C == 96 for r in of)
    sc = by("scale")
    assert any(r.p.B >= 65536 for r in sc) and any(r.p.mis for r in sc) and any(r.p.C % 4 for r in sc)
    cs = by("colsum")
    assert any(r.p.cols > 1024 and r.p.cols % 4 == 0 for r in cs) and any(r.p.cols > 256 and r.p.cols % 4 for r in cs)
    assert any(r.p.rows > 1 << 20 for r in cs) and any(r.p.mis and r.p.cols % 4 == 0 for r in cs)
    co = by("coords")
    assert any(r.p.c == 1 and r.p.with_r and r.p.mis for r in co) and any(r.p.c == 1 and r.p.with_r and not r.p.mis for r in co)
    # the rows above a megabyte are the cap rows
    big = [r.name for r in M.CASES if sum(t.numel() for t in M.values(r.name).values()) * 4 > 1 << 20]
    assert all(any(w in n for w in ("second trip", "one sweep", "cap", "65536")) for n in big), big


def test_pair_count():
    product = sum(len(M.FORMS[r.entry]) for r in M.CASES)
    left_out = [(r.name, nm, M.excluded(r, f)) for r in M.CASES for nm, f in M.FORMS[r.entry].items() if M.excluded(r, f)]
    pairs = M.pairs()
    assert len(pairs) == len(set(pairs)) == product - len(left_out) == M.PAIR_COUNT
    assert all(isinstance(why, str) and why for _, _, why in left_out)
    assert not set(pairs) & {(n, f) for n, f, _ in left_out}


# ---- the references against ATen
def _within(got, ref, bound, factor=1.0):
    r = M.ratio(got, ref, bound * factor).max().item()
    print("ATen against the reference: %.3g of the bound" % r)
    assert r <= 1.0, r
    return r


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "bn_fwd" and 1 < M.CASE[n].p.hw < 4096])  # ATen refuses one value per channel)
def test_batchnorm_reference_equals_aten_slot_by_slot(name):
    """BatchNorm2d on each slot as a batch of one, in slot order: forward, running statistics and the
    autograd backward.  ATen evaluates (x - mean) invstd gamma + beta - fewer roundings than the
    kernel's expression - and its own backward expression; four times the bound covers either."""
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    f = M.FORMS["bn_fwd"]["plain"]
    ref = M.bn_fwd_ref(p, f, v, True, sum_unit=M.U)           # ATen may sum a slot in fp32
    bn = torch.nn.BatchNorm2d(p.C, eps=1e-5, momentum=0.1)
    with torch.no_grad():
        bn.weight.copy_(v["gamma"]), bn.bias.copy_(v["beta"]), bn.running_mean.copy_(v["rm"]), bn.running_var.copy_(v["rv"])
    fb = M.FORMS["bn_bwd"]["plain"]
    # ... and its backward reads its own saved statistics, the reference's backward the reference's
    mu, var, m1, m2 = M.bn_stats64(v["z"].double())
    rstd = (var + M.EPS) ** -0.5
    dmean, drel = (p.hw + 2) * M.U * m1, 0.5 * rstd ** 2 * (2 * p.hw + 6) * M.U * (m2 + mu * mu) + M.U
    bref = M.bn_bwd_ref(p, fb, v, sum_unit=M.U, stat_err=(dmean, drel))
    ys, dzs = [], []
    for b in range(p.B):
        z = v["z"][b].t().reshape(1, p.C, p.hw, 1).clone().requires_grad_(True)
        y = bn(z)
        y.backward(v["g"][b].t().reshape(1, p.C, p.hw, 1))
        ys.append(y.detach().reshape(p.C, p.hw).t())
        dzs.append(z.grad.reshape(p.C, p.hw).t())
    _within(torch.stack(ys), *ref["y"], factor=4)
    _within(bn.running_mean, *ref["running_mean"], factor=4)
    _within(bn.running_var, *ref["running_var"], factor=4)
    if p.hw > 1:
        # the backward reference takes the saved statistics rounded to fp32; ATen's are its own
        _within(torch.stack(dzs), *bref["dz"], factor=4)
        # ATen sums a slot's gradients in its own order and .grad adds the slots in fp32: one fp32 chain at most
        sm, sr = M.bn_saved(p, v)
        g64, d64 = v["g"].double().abs(), (v["z"].double() - sm.double()[:, None, :]).abs()
        chain = (p.hw + p.B + 8) * M.U
        own = ((g64.sum(1) * dmean + (d64 * g64).sum(1) * drel) * sr.double()).sum(0)
        _within(bn.weight.grad, bref["dgamma"][0], chain * (d64 * g64 * sr.double()[:, None, :]).sum((0, 1)) + own)
        _within(bn.bias.grad, bref["dbeta"][0], chain * g64.sum((0, 1)))


@pytest.mark.parametrize("name", ["bn eval C 12", "bn eval C 96"])
def test_batchnorm_eval_reference_equals_aten(name):
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    ref = M.bn_fwd_ref(p, M.FORMS["bn_eval"]["relu"], v, False)
    y = F.relu(F.batch_norm(v["z"].permute(0, 2, 1), v["rm"].clone(), v["rv"].clone(), v["gamma"], v["beta"], False, 0.1, 1e-5))
    _within(y.permute(0, 2, 1), *ref["y"], factor=4)


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "up_bwd"])
def test_upsample_reference_equals_aten_and_exact_coordinates(name):
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    plain = M.FORMS["up_bwd"]["plain"]
    x = v["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    y.backward(v["dy"].permute(0, 3, 1, 2))
    fwd, bwd = M.up_ref(p, plain, v, False), M.up_ref(p, plain, v, True)
    _within(y.detach().permute(0, 2, 3, 1), *fwd["y"])
    _within(x.grad.permute(0, 2, 3, 1), *bwd["dx"])
    # the float32 coordinate formula against rational coordinates
    for is_bwd, ref in ((False, fwd["y"]), (True, bwd["dx"])):
        exact = M.up_ref(p, plain, v, is_bwd, rule=M.lin_exact)["dx" if is_bwd else "y"]
        _within(ref[0], exact[0], exact[1] + M.up_coordinate_slack(p, v, is_bwd))
    # the backward reference is the transpose of the forward one
    lhs = (fwd["y"][0] * v["dy"].double()).sum()
    rhs = (bwd["dx"][0] * v["x"].double()).sum()
    assert abs(lhs - rhs) <= 1e-12 * (fwd["y"][0].abs() * v["dy"].double().abs()).sum()


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "pool_bwd"])
def test_maxpool_reference_equals_aten(name):
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    plain = M.FORMS["pool_bwd"]["plain"]
    x = v["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(x, 2)
    y.backward(v["dy"].permute(0, 3, 1, 2))
    fwd = M.pool_ref(p, M.FORMS["pool_fwd"]["plain"], v, False)["y"][0].float()
    bwd = M.pool_ref(p, plain, v, True)["dx"][0].float()
    assert M.ratio(y.detach().permute(0, 2, 3, 1), fwd, torch.zeros_like(fwd)).max().item() == 0
    assert M.ratio(x.grad.permute(0, 2, 3, 1), bwd, torch.zeros_like(bwd)).max().item() == 0
    if p.special:
        assert bool(fwd.isnan().any()) and bool((fwd == float("-inf")).any())


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "oc_bwd" and M.CASE[n].p.rows < 100000])
def test_outconv_reference_equals_aten(name):
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    x = v["x"].t().reshape(1, p.C, p.rows, 1).clone().requires_grad_(True)
    w = v["w"].reshape(1, p.C, 1, 1).clone().requires_grad_(True)
    b = v["b"].clone().requires_grad_(True)
    y = F.conv2d(x, w, b)
    y.backward(v["dy"].reshape(1, 1, p.rows, 1))
    fwd = M.oc_fwd_ref(M.P(p, mis=None), M.FORMS["oc_fwd"]["bias"], v)["y"]
    bwd = M.oc_bwd_ref(p, M.FORMS["oc_bwd"]["no relu"], v)
    chain = lambda n: (n + 2) * M.U                # noqa: E731   ATen's order is its own: one fp32 chain at most
    M_y = v["x"].double().abs() @ v["w"].double().abs() + v["b"].double().abs()
    _within(y.detach().reshape(-1), fwd[0], chain(p.C) * M_y)
    dx = x.grad.reshape(p.C, p.rows).t()
    if p.dt == "f32":
        assert torch.equal(dx, bwd["dx"][0])
    _within(w.grad.reshape(-1), bwd["dw"][0], chain(p.rows) * (v["dy"].double().abs() @ v["x"].double().abs()))
    _within(b.grad, bwd["db"][0], chain(p.rows) * v["dy"].double().abs().sum().reshape(1))


def test_one_liners_equal_aten():
    for name in NAMES:
        r = M.CASE[name]
        p, v = r.p, M.values(name)
        if r.entry == "colsum" and p.rows < 100000:
            ref = M.colsum_ref(p, M.FORMS["colsum"]["plain"], v)["out"]
            _within(v["x"].sum(0), ref[0], (p.rows + 2) * M.U * v["x"].double().abs().sum(0))
        if r.entry == "coords":
            # the layer itself, as the model's AddCoords computes it with torch's elementwise float ops
            B, c, h, w = p.B, p.c, p.h, p.w
            xx = torch.arange(w).repeat(1, h, 1).float() / (h - 1) * 2 - 1
            yy = torch.arange(h).repeat(1, w, 1).transpose(1, 2).float() / (w - 1) * 2 - 1
            parts = [v["x"], xx.repeat(B, 1, 1, 1), yy.repeat(B, 1, 1, 1)]
            if p.with_r:
                parts.append(torch.sqrt(torch.pow(parts[1] - 0.5, 2) + torch.pow(parts[2] - 0.5, 2)))
            want = torch.cat(parts, 1).permute(0, 2, 3, 1).contiguous()
            # torch's own vectorised float ops may round an operation differently from one CPU to the
            # next: five operations on values of at most 3 (the kernel is held to the numpy reference bit for bit)
            got = M.coords_ref(p, None, v)["out"][0]
            assert torch.equal(got[..., :c], want[..., :c]) and float((got - want).abs().max()) <= 5 * M.U * 3, name


# ---- sensitivity
def _stored(val):
    """the reference as a correct kernel would store it"""
    return val if val.dtype != F64 else val.float()


SENSITIVITY = {}


@pytest.mark.parametrize("name", NAMES)
def test_bounds_reject_the_mutants(name):
    r = M.CASE[name]
    for fname, f in M.forms(r):
        ref = M.reference(name, fname)
        for out, (val, bound) in ref.items():
            assert M.ratio(_stored(val), val, bound).max().item() <= 1.0, (fname, out)
        for mutant in M.MUTANTS:
            if not M.applies(r, f, mutant):
                continue
            mut = M.mutated(name, fname, mutant)
            worst, touched_n, outside_n = 0.0, 0, 0
            for out, (val, bound) in ref.items():
                got = mut[out][0]
                rr = M.ratio(_stored(got), val, bound)
                touched = rr > 0
                if val.dtype == F64:
                    touched = (got.double().reshape(-1) - val.reshape(-1)).abs() > 1e-12 * bound.reshape(-1).clamp_min(1e-300) / M.U
                if bool(touched.any()):
                    worst = max(worst, rr[touched].max().item())
                    touched_n += int(touched.sum())
                    outside_n += int((rr[touched] > 1.0).sum())
            print("%s | %s | %s: %d entries touched, worst %.3g x the bound, %.1f %% outside"
                  % (name, fname, mutant, touched_n, worst, 100.0 * outside_n / max(touched_n, 1)))
            assert touched_n > 0 and outside_n > 0, (fname, mutant, touched_n, worst)
            key = SENSITIVITY.setdefault(mutant, [float("inf"), 1.0, 0])
            key[0], key[1], key[2] = min(key[0], worst), min(key[1], outside_n / touched_n), key[2] + 1


def test_sensitivity_summary():
    """per mutant over the pairs run so far in this process: the least worst-entry ratio and the
    least share of touched entries outside the bound (the record in DESIGN.md comes from here)"""
    for mutant in M.MUTANTS:
        if mutant in SENSITIVITY:
            w, s, n = SENSITIVITY[mutant]
            print("sensitivity %-30s %4d pairs, worst entry at least %.3g x the bound, at least %.1f %% outside"
                  % (mutant, n, w, 100 * s))
    assert set(SENSITIVITY) <= set(M.MUTANTS)
