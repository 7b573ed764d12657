"""Every layer kernel outside the convolutions, in every form it can be given, against fp64 (case
table, references, bounds and runner: tests/layer_matrix.py; their CPU checks: test_layer_matrix.py).

Per (row, form): the call returns PU_OK; every entry of every output lies within its derived bound of
the reference (bound 0: bit for bit); every destination and the workspace - exactly the queried
bytes - keep the sentinel bands around them; no entry the call must write keeps its NaN fill, and the
entries it must not write (BatchNorm eval: [C, B C) of the statistics) keep theirs; an accumulate
call equals seed + the plain call's result bit for bit.  The reductions are bitwise the same on a
second run.  The fused forms equal the separate ones bit for bit (a scaled pool = the pool, then
pu_channel_scale; add_coords4_kernel = add_coords_kernel).  Rejected calls return their status and
write nothing.

Each test prints its error / bound ratio; test_headroom_per_family prints the maximum per kernel
family (the record in DESIGN.md comes from it).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_matrix as M  # noqa: E402

PAIRS = M.pairs()
assert len(PAIRS) == M.PAIR_COUNT
HEADROOM = {}
BF = torch.bfloat16


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _checked(r, fname, res):
    """status, bands, fill and every output against the reference of (row, form)"""
    assert res.rc == M.OK, res.rc
    assert res.intact, "sentinels around a destination or the workspace were overwritten"
    assert not res.kept, "an output keeps part of its NaN fill"
    assert res.extra, "entries the call must not write were written"
    ref = M.reference(r.name, fname)
    assert set(ref) == set(res.outs), (sorted(ref), sorted(res.outs))
    for out, (val, bound) in ref.items():
        q = M.ratio(res.outs[out], val, bound).max().item()
        print("%s [%s | %s] %s: %.3g of the bound" % (r.entry, r.name, fname, out, q))
        assert q <= 1.0, "%s off the reference: %.3g x the bound" % (out, q)
        if bool((bound > 0).any()):
            HEADROOM[r.entry, out] = max(HEADROOM.get((r.entry, out), 0.0), q)
    return res


@pytest.mark.parametrize("name,form", PAIRS, ids=["%s | %s" % p for p in PAIRS])
def test_row_times_form(name, form):
    r = M.CASE[name]
    f = M.FORMS[r.entry][form]
    res = _checked(r, form, M.run(r, f))
    v = M.values(name)
    if f.acc:
        # one addition onto the seed of what the same call gives without accumulate
        plain = M.run(r, M.P(f, acc=None))
        assert plain.rc == M.OK and plain.intact
        out = "dx" if r.entry == "pool_bwd" else "out"
        got, base = res.outs[out], plain.outs[out]
        want = (v["seed"].reshape(-1) + base.float()).to(got.dtype)
        assert torch.equal(_bits(got), _bits(want)), "accumulate is not one fp32 addition onto the seed"
    if r.entry in ("up_fwd", "up_bwd") and form == "plain":
        # the float32 coordinate formula itself: the same output against rational coordinates
        bwd = r.entry == "up_bwd"
        val, bound = M.up_ref(r.p, f, v, bwd, rule=M.lin_exact)["dx" if bwd else "y"]
        q = M.ratio(res.outs["dx" if bwd else "y"], val, bound + M.up_coordinate_slack(r.p, v, bwd)).max().item()
        print("%s against exact coordinates: %.3g of the widened bound" % (name, q))
        assert q <= 1.0, q


REDUCED = {"bn_fwd": ("save_mean", "save_rstd", "running_mean", "running_var"), "bn_bwd": ("dgamma", "dbeta"),
           "oc_bwd": ("dw", "db"), "colsum": ("out",)}


@pytest.mark.parametrize("name", [r.name for r in M.CASES if r.entry in REDUCED])
def test_reductions_are_bitwise_on_a_second_run(name):
    r = M.CASE[name]
    f = M.forms(r)[0][1]
    first, second = M.run(r, f), M.run(r, f)
    assert first.rc == M.OK and second.rc == M.OK and first.intact and second.intact
    for out in REDUCED[r.entry]:
        assert torch.equal(_bits(first.outs[out]), _bits(second.outs[out])), "%s differs between two runs" % out


@pytest.mark.parametrize("name", [r.name for r in M.CASES if r.entry in ("pool_fwd", "pool_bwd") and r.p.dt == "f32"])
def test_scaled_pool_is_pool_then_channel_scale(name):
    """forward: the pooled plane through pu_channel_scale; backward: dy through pu_channel_scale, then
    the plain backward - what the fused kernels promise bit for bit"""
    from punet import kernels as K
    r = M.CASE[name]
    p, v = r.p, M.values(name)
    L = M._lib.load()
    scale = v["scale"].cuda()
    if r.entry == "pool_fwd":
        fused = M.run(r, M.FORMS["pool_fwd"]["scaled"])
        if p.mis == "scale":
            plain = M.run(M.Row(name, r.entry, None, M.P(p, mis=None)), M.FORMS["pool_fwd"]["plain"])
        else:
            plain = M.run(r, M.FORMS["pool_fwd"]["plain"])
        assert fused.rc == M.OK and plain.rc == M.OK
        y = plain.outs["y"].cuda()
        out = torch.full_like(y, float("nan"))
        assert L.pu_channel_scale(y.data_ptr(), scale.data_ptr(), out.data_ptr(), p.B, (p.H // 2) * (p.W // 2), p.C,
                                  K._stream()) == M.OK
        torch.cuda.synchronize()
        assert torch.equal(_bits(fused.outs["y"]), _bits(out.cpu()))
        return
    for form in ("scaled", "scaled+relu+acc"):
        f = M.FORMS["pool_bwd"][form]
        fused = M.run(r, f)
        dy = v["dy"].cuda().reshape(-1)
        sdy = torch.full_like(dy, float("nan"))
        assert L.pu_channel_scale(dy.data_ptr(), scale.data_ptr(), sdy.data_ptr(), p.B, (p.H // 2) * (p.W // 2), p.C,
                                  K._stream()) == M.OK
        x = v["x"].cuda().reshape(-1)
        dx = v["seed"].cuda().reshape(-1).clone() if f.acc else torch.full_like(x, float("nan"))
        assert L.pu_maxpool2_bwd(x.data_ptr(), sdy.data_ptr(), dx.data_ptr(), p.B, p.H, p.W, p.C, int(bool(f.relu)),
                                 int(bool(f.acc)), K._stream()) == M.OK
        torch.cuda.synchronize()
        assert fused.rc == M.OK and torch.equal(_bits(fused.outs["dx"]), _bits(dx.cpu())), form


def test_add_coords4_equals_add_coords():
    r = M.CASE["coords c 1 + r"]
    four = M.run(r, M.FORMS["coords"]["plain"])
    plain = M.run(M.Row(r.name, r.entry, None, M.P(r.p, mis="out")), M.FORMS["coords"]["plain"])
    assert four.rc == M.OK and plain.rc == M.OK and four.intact and plain.intact
    assert torch.equal(_bits(four.outs["out"]), _bits(plain.outs["out"]))


def _rej(base, form, status, name=None, **change):
    """a rejected call: row `base` with parameters replaced (a new name: its own values) or the call
    changed (mis / null: operand names, ws_short, ws_null)"""
    r = M.CASE[base]
    over = {k: change.pop(k) for k in ("mis", "null", "ws_short", "ws_null") if k in change}
    if change:
        r = M.Row(name, r.entry, None, M.P(r.p, **change))
    return r, form, over, status


BNF, BNB, BNE = "bn fwd C 12: idle tail threads", "bn bwd C 12: idle tail threads", "bn eval C 12"
REJECTED = [
    _rej(BNF, "relu", M.INVALID, name="rejected bn fwd C 6", C=6),
    _rej(BNF, "relu", M.INVALID, mis=("z",)),
    _rej(BNF, "relu", M.INVALID, mis=("y",)),
    _rej(BNF, "resid+relu", M.INVALID, mis=("resid",)),
    _rej(BNF, "relu", M.INVALID, null=("running_var",)),                 # one running buffer without the other
    _rej(BNF, "relu", M.INVALID, null=("running_mean",)),
    _rej(BNE, "relu", M.INVALID, null=("running_mean", "running_var")),   # eval without running statistics
    _rej(BNF, "relu", M.WORKSPACE, ws_short=1),
    _rej(BNF, "relu", M.WORKSPACE, ws_null=True),
    _rej(BNB, "plain", M.INVALID, name="rejected bn bwd C 6", C=6),
    _rej(BNB, "plain", M.INVALID, mis=("g",)),
    _rej(BNB, "plain", M.INVALID, mis=("dz",)),
    _rej(BNB, "add+mask", M.INVALID, mis=("add",)),
    _rej(BNB, "add+mask", M.INVALID, mis=("mask",)),
    _rej(BNB, "plain", M.WORKSPACE, ws_short=1),
    _rej(BNB, "plain", M.WORKSPACE, ws_null=True),
    _rej("up fwd 3x5", "plain", M.INVALID, name="rejected up fwd C 6", C=6),
    _rej("up fwd 3x5", "plain", M.INVALID, mis=("x",)),
    _rej("up fwd 3x5", "plain", M.INVALID, mis=("y",)),
    _rej("up bwd 3x5", "plain", M.INVALID, name="rejected up bwd C 6", C=6),
    _rej("up bwd 3x5", "mask", M.INVALID, mis=("dy",)),
    _rej("up bwd 3x5", "mask", M.INVALID, mis=("dx",)),
    _rej("up bwd 3x5", "mask", M.INVALID, mis=("mask",)),
    _rej("outconv bwd f32 C 8", "relu", M.INVALID, name="rejected outconv bwd C 6", C=6),
    _rej("outconv bwd f32 C 8", "relu", M.INVALID, mis=("x",)),
    _rej("outconv bwd f32 C 8", "relu", M.INVALID, mis=("w",)),
    _rej("outconv bwd f32 C 8", "relu", M.INVALID, mis=("dx",)),
    _rej("outconv bwd f32 C 8", "relu", M.WORKSPACE, ws_short=1),
    _rej("outconv bwd f32 C 8", "relu", M.WORKSPACE, ws_null=True),
    _rej("outconv fwd bf16 C 8", "bias", M.INVALID, mis=("x",)),          # 4 bytes off the 8 its bf16 quads need
    _rej("outconv fwd bf16 C 8", "bias", M.INVALID, mis=("w",)),          # 4 bytes off the 16 its float4 needs
    _rej("outconv fwd bf16 C 8", "bias", M.INVALID, name="rejected outconv fwd bf16 C 6", C=6),
    _rej("outconv bwd bf16 C 8", "relu", M.INVALID, mis=("x",)),
    _rej("outconv bwd bf16 C 8", "relu", M.INVALID, mis=("w",)),
    _rej("outconv bwd bf16 C 8", "relu", M.INVALID, mis=("dx",)),
    _rej("outconv bwd bf16 C 64", "relu", M.INVALID, mis=("x",)),
    _rej("outconv bwd bf16 C 8", "relu", M.WORKSPACE, ws_short=1),
    _rej("colsum 300x8", "plain", M.WORKSPACE, ws_short=1),
    _rej("colsum 300x8", "acc", M.WORKSPACE, ws_null=True),
    _rej("pool fwd f32 even", "scaled", M.INVALID, null=("scale",)),
    _rej("pool bwd f32 even", "scaled", M.INVALID, null=("scale",)),
    _rej("pool fwd bf16 even", "plain", M.INVALID, name="rejected pool fwd bf16 C 6", C=6),
    _rej("pool bwd bf16 even", "plain", M.INVALID, name="rejected pool bwd bf16 C 6", C=6),
    _rej("f32 to bf16", "plain", M.INVALID, name="rejected convert n 4002", n=4002),
    _rej("bf16 to f32", "plain", M.INVALID, name="rejected convert back n 4002", n=4002),
]


@pytest.mark.parametrize("r,form,over,status", REJECTED,
                         ids=["%s | %s" % (r.name, ",".join("%s=%s" % kv for kv in o.items()) or "shape") for r, _, o, _ in REJECTED])
def test_rejected_call_writes_nothing(r, form, over, status):
    res = M.run(r, M.FORMS[r.entry][form], **over)
    assert res.rc == status, res.rc
    assert res.untouched and res.intact, "a rejected call wrote to an output or to the workspace"


def test_headroom_per_family():
    """the worst error / bound ratio of each output of each entry point over the pairs run so far in
    this process (outputs with a bound of 0 are bit for bit and not part of the figure)"""
    for entry, out in sorted(HEADROOM):
        print("headroom %-8s %-12s %.3g" % (entry, out, HEADROOM[entry, out]))
    assert {e for e, _ in HEADROOM} <= set(M.FORMS)
    assert all(q <= 1.0 for q in HEADROOM.values())
