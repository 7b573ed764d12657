"""CPU checks of the head matrix (tests/head_matrix.py; the GPU run is test_head_matrix_gpu.py).

1. Plans: every row lands on the kernels it was written for - the launcher's rule (kernel_of) applied
   to the row's arguments gives the instantiations the row claims, and the pinned L / TPW / R / kc of
   the fused head, the tile, the strip and chunk counts of the trace backward, the block counts and
   every workspace size are those the rule and the library's queries give.
2. Coverage: the rows claim exactly the kernels of csrc/plastic.hip and csrc/adam.hip in the build's
   resource report, in both directions, 74 in all.  One column tile per wave (TPW = 1) with 32-row
   blocks (R = 32) is shown unreachable from the rule itself, over every nbf the entry accepts.
3. Pair count: the (row, form) pairs are the table's product minus the pairs excluded by a rule.
4. The references against the oracle: oracle.ref_cpu.plastic_head in fp64 and torch autograd through
   it (both rules, all five gradients, with and without the trace path), F.binary_cross_entropy and
   its autograd, torch.optim.Adam on float64.
5. Sensitivity: every mutant of MUTANTS falls outside the bound on every (row, form) it applies to
   ("outside" for at least one touched entry per pair; the worst ratio and the share of touched
   entries outside are printed), while the reference rounded to the output's type passes it.
"""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))

import head_matrix as M  # noqa: E402
from oracle import ref_cpu as oracle  # noqa: E402
from wgrad_matrix import demangle  # noqa: E402

NAMES = [r.name for r in M.CASES]
F64 = torch.float64
RULE = ("hebb", "oja")


@pytest.mark.parametrize("name", NAMES)
def test_row_launches_the_kernels_it_claims(name):
    r = M.CASE[name]
    assert M.forms(r)
    assert M.kernel_of(r) == r.kernels, sorted(M.kernel_of(r) ^ r.kernels)
    assert M.plan_of(r) == M.pinned(r), (M.plan_of(r), M.pinned(r))
    if r.entry == "bwdt":
        assert r.p.ws == M.bwdt_ws(r.p.B, r.p.N)


def _built():
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    return {demangle(sym) for sym, k in d["kernels"].items() if k["source"] in M.SOURCES}


def test_rows_claim_every_kernel_of_the_two_files():
    built = _built()
    claimed = set().union(*(r.kernels for r in M.CASES))
    assert not built - claimed, "kernels in the build that no row reaches: %s" % sorted(built - claimed)
    assert not claimed - built, "rows claim kernels the build lacks: %s" % sorted(claimed - built)
    assert len(built) == M.KERNEL_COUNT == 74


def test_one_tile_per_wave_never_meets_32_row_blocks():
    """R = 32 needs nbf >= 256: 16 column tiles or more over 8 waves, two per wave at least.  By the
    rule, over every nbf pu_plastic_head_fwd accepts: the launcher instantiates no <T, L, 1, 32>."""
    plans = {M.head_plan(N, 64)[1:3] for N in range(16, 513, 16)}
    assert (1, 32) not in plans
    assert plans == {(1, 16), (2, 16), (2, 32), (4, 16), (4, 32)}
    assert not [k for k in _built() if k.startswith("head_fused_fwd_kernel") and k.endswith(",1,32>")]


def test_rows_cover_the_branches():
    """the branches of the launchers beyond one row per instantiation"""
    by = lambda e: [r for r in M.CASES if r.entry == e]      # noqa: E731
    head = by("head")
    for dt in ("f32", "bf16"):
        rows = [r for r in head if r.p.dt == dt]
        assert {(r.p.L, r.p.TPW, r.p.R) for r in rows} == {(L, t, R) for L in (1, 2, 4, 8, 16)
                                                           for t, R in ((1, 16), (2, 16), (2, 32), (4, 16), (4, 32))}
        assert {4, 8, 16, 32, 64, 128} <= {r.p.C for r in rows} and {12, 20} & {r.p.C for r in rows}
        pipe = [r for r in rows if r.p.N == 128 and r.p.C >= 64]
        assert {64, 68, 96, 128} <= {r.p.C for r in pipe}
        assert any(r.p.N == 128 and r.p.C == 48 for r in rows)                    # L = 16 but serial
    assert {1, 8, 9} <= {r.p.B for r in head if r.p.N == 128 and r.p.C >= 64}      # the XCD block order
    assert {16, 48, 144, 160, 192, 256, 272, 288, 320, 384, 512} <= {r.p.N for r in head}
    assert {r.p.N: r.p.kc for r in head if r.p.N in (144, 192, 320, 384)} == {144: 72, 192: 64, 320: 40, 384: 32}
    assert {r.p.rule for r in head} == {0, 1} and any(r.p.B == 2 and r.p.R == 32 for r in head)
    assert {(r.p.B, r.p.N) for r in by("fwd")} >= {(1, 1), (5, 3), (1, 16), (2, 17), (3, 50), (512, 16), (128, 72), (32, 200)}
    assert {r.p.tile for r in by("fwd")} == {32, 64}
    tr = by("trace")
    assert any(r.p.N % 4 for r in tr) and {r.p.mis for r in tr if r.p.N % 4 == 0} == {None, "hebb", "hebb_out", "y"}
    bw = by("bwd")
    assert {(r.p.B, r.p.N) for r in bw} == {(1, 16), (2, 17), (5, 3), (3, 50), (2, 200), (128, 72), (32, 200)}
    assert any(r.p.data == "zero_h" for r in bw)
    bt = by("bwdt")
    plain = [r for r in bt if not r.p.mis]
    assert {(r.p.V, r.p.ns) for r in plain} >= {(4, 1), (4, 2), (1, 1), (1, 2)}
    for V, ns in ((4, 1), (4, 2), (1, 1), (1, 2)):
        assert {r.p.rule for r in plain if (r.p.V, r.p.ns) == (V, ns)} == {0, 1}
    assert any(r.p.V == 4 and r.p.N > 128 for r in bt) and any(r.p.N % M.TB_ROWS for r in bt)      # a partial last row chunk
    assert {r.p.mis for r in bt} >= {"dhebb_out", "hebb", "dhebb", "alpha"}
    assert any(r.p.V == 1 and r.p.N % 4 == 0 and r.p.N > 128 for r in bt)         # <1> by misalignment
    assert {r.p.Vh for r in bt} == {1, 4} and any(r.p.Vh == 1 and r.p.N % 4 == 0 for r in bt)
    assert any(r.p.tile == 64 and r.p.N > 64 for r in bt)
    assert any(r.p.B * r.p.N > 1024 * 256 for r in bt)                             # the finish kernel's cap
    assert any(r.p.data == "zero_h" for r in bt)
    for e in ("bce_fwd", "bce_bwd"):
        assert {1, 255, 257} <= {r.p.n for r in by(e)}
    assert any(r.p.blocks < 512 and r.p.n > 257 for r in by("bce_fwd")) and any(r.p.n > 512 * 256 for r in by("bce_fwd"))
    assert any(r.p.n > 8192 * 256 for r in by("bce_bwd"))
    ad = by("adam")
    assert {1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 5} <= set(ad[0].p.numels)
    assert {r.p.mis[1] for r in ad if r.p.mis} == set("pgmv")
    assert any(0 in r.p.numels[1:-1] for r in ad)
    assert {len(r.p.launches) for r in ad} == {1, 2, 3}
    assert {bool(r.p.wd) for r in ad} == {False, True} and any(r.p.step == 1 for r in ad) and any(r.p.step >= 1000 for r in ad)
    # one saturated row per entry point that forms or reads Y: |a| > 88 and 17 < |a| < 88
    for e in ("head", "fwd"):
        sat = [r for r in by(e) if r.p.data == "sat"]
        assert sat
        for r in sat:
            a = M._head_full(r.name, True, None)["a"][0].abs()
            assert bool((a > 88).any()) and bool(((a > 17) & (a < 88)).any())
    assert any(r.p.data == "sat" for r in bw) and any(r.p.data == "sat" for r in bt)
    # the rows with an operand above 12 MB are the XCD-order rows and the finish kernel's cap row
    size = lambda r: max(t.numel() * (2 if k == "feat" and r.p.dt == "bf16" else 4)          # noqa: E731
                         for k, ts in M.values(r.name).items() for t in (ts if isinstance(ts, list) else [ts]))
    assert all(r.p.big for r in M.CASES if size(r) > 12 << 20)


def test_pair_count():
    product = sum(len(M.FORMS[r.entry]) for r in M.CASES)
    left_out = [(r.name, nm, M.excluded(r, f)) for r in M.CASES for nm, f in M.FORMS[r.entry].items() if M.excluded(r, f)]
    pairs = M.pairs()
    assert len(pairs) == len(set(pairs)) == product - len(left_out) == M.PAIR_COUNT
    assert all(isinstance(why, str) and why for _, _, why in left_out)
    assert not set(pairs) & {(n, f) for n, f, _ in left_out}


# ---- the references against the oracle
def _agree(got, ref, bound, share=1e-6):
    """two fp64 evaluations of the same thing: within a millionth of the fp32 bound"""
    q = M.ratio(got, ref, bound).max().item()
    assert q <= share, q


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "fwd"])
def test_head_forward_reference_equals_the_oracle(name):
    r = M.CASE[name]
    v = M.values(name)
    ref = M.head_ref(r, M.FORMS["fwd"]["fused"])
    Y, Hn = oracle.plastic_head(v["X"].double(), v["H"].double(), v["w"].double(), v["al"].double(), v["eta"].double(),
                                RULE[r.p.rule])
    _agree(Y, *ref["Y"])
    _agree(Hn, *ref["Hn"])
    # ... and the float32 expressions of the trace update are ATen's, op for op
    x0, y0 = v["X"][:, 0], torch.rand(r.p.B, r.p.N, generator=torch.Generator().manual_seed(1))
    assert torch.equal(M.trace_np(v["H"], x0, y0, v["eta"], r.p.rule), oracle.trace_update(v["H"], x0, y0, v["eta"], RULE[r.p.rule]))


@pytest.mark.parametrize("name,form", [(r.name, fm) for r in M.CASES if r.entry == "bwdt" and r.p.B < 100
                                       for fm in ("all", "no dy", "no dhebb_out") if not M.excluded(r, M.FORMS["bwdt"][fm])])
def test_head_backward_reference_equals_autograd_through_the_oracle(name, form):
    """dX, dw, dalpha, dH and deta of  sum(Y dY) + sum(H' P)  by autograd through the oracle in fp64,
    with and without the trace path; Y is the oracle's own, handed to the reference in fp64."""
    r = M.CASE[name]
    f = M.FORMS["bwdt"][form]
    v = M.values(name)
    X, H, w, al, eta = (v[k].double().clone().requires_grad_(True) for k in ("X", "H", "w", "al", "eta"))
    Y, Hn = oracle.plastic_head(X, H, w, al, eta, RULE[r.p.rule])
    loss = (Y * v["dY"].double()).sum() * (1 if f.dy else 0) + ((Hn * v["P"].double()).sum() if f.P else 0)
    loss.backward()
    ref = M.bwd_ref(r, f, v=dict(v, Y=Y.detach()))
    for out, t in (("dx", X), ("dw", w), ("dalpha", al), ("dhebb", H)):
        _agree(t.grad, *ref[out])
    if f.P:
        _agree(eta.grad, *ref["deta"])
    else:
        assert "deta" not in ref


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry in ("bce_fwd", "bce_bwd")])
def test_bce_reference_equals_aten(name):
    r = M.CASE[name]
    v = M.values(name)
    y = v["y"].double().clone().requires_grad_(True)
    loss = F.binary_cross_entropy(y, v["t"].double())
    if r.entry == "bce_fwd":
        _agree(loss.detach().reshape(1), *M.bce_fwd_ref(r, M.FORMS["bce_fwd"]["plain"])["loss"])
        return
    (loss * v["g"].double()[0]).backward()
    got = M.bce_bwd_ref(r, M.FORMS["bce_bwd"]["grad_loss"])["dy"][0]
    # five float32 operations against ATen's fp64
    assert M.ratio(got, y.grad, 6 * M.U * y.grad.abs()).max().item() <= 1.0


@pytest.mark.parametrize("name", [n for n in NAMES if M.CASE[n].entry == "adam"])
def test_adam_reference_equals_torch_adam_on_float64(name):
    """torch.optim.Adam on float64 from the same state; the float32 chain of adam_one is bounded by its
    operations: m 3 and a cast, v 4 and a cast, the denominator 3 and a cast, the update 3 and a cast"""
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    hp = M.ADAM_HP
    ps = [torch.nn.Parameter(t.double().clone()) for t in v["p"]]
    opt = torch.optim.Adam(ps, lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=p.wd)
    for q, g, m, vv in zip(ps, v["g"], v["m"], v["v"]):
        q.grad = g.double().clone()
        opt.state[q] = {"step": torch.tensor(float(p.step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": vv.double().clone()}
    opt.step()
    got = M.adam_np(p, v)
    cat = lambda ts: torch.cat([t.detach().double().reshape(-1) for t in ts])      # noqa: E731
    p0, g0, m0, v0 = (cat(v[k]) for k in "pgmv")
    b1, b2, eps, wd, ss, bc = M.adam_scalars(p)
    U = M.U
    g1 = g0 + wd * p0
    bg = 2 * U * (g0.abs() + wd * p0.abs()) if wd else torch.zeros_like(g0)
    m1, v1 = cat(opt.state[q]["exp_avg"] for q in ps), cat(opt.state[q]["exp_avg_sq"] for q in ps)
    bm = 4 * U * (m0.abs() + (1 - b1) * (g1.abs() + m0.abs())) + (1 - b1) * bg
    bv = 5 * U * (v0 * b2 + (1 - b2) * g1 * g1) + (1 - b2) * 2 * g1.abs() * bg
    den = v1.sqrt() / bc + eps
    bden = bv / (2 * v1.sqrt() * bc) + 4 * U * den
    upd = ss * m1 / den
    bp = ss * (bm / den + m1.abs() * bden / den ** 2) + 4 * U * upd.abs() + 2 * U * (p0.abs() + upd.abs())
    for k, ref, b in (("m", m1, bm), ("v", v1, bv), ("p", cat(ps), bp)):
        q = M.ratio(got[k], ref, b).max().item()
        print("%s %s: %.3g of the bound" % (name, k, q))
        assert q <= 1.0, (k, q)


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
                    diff = (got.double().reshape(-1) - val.reshape(-1)).abs().nan_to_num(nan=float("inf"))
                    touched = diff > 1e-12 * bound.reshape(-1).clamp_min(1e-300) / M.U
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
            print("sensitivity %-42s %4d pairs, worst entry at least %.3g x the bound, at least %.1f %% outside"
                  % (mutant, n, w, 100 * s))
    assert set(SENSITIVITY) <= set(M.MUTANTS)
