"""Every weight-gradient GEMM kernel the plan can pick, in every form it can be given, against fp64
(case table, reference, bounds and runner: tests/wgrad_matrix.py; their CPU checks:
test_wgrad_matrix.py).

Per (case, form): the call returns PU_OK on the pinned plan; every dweight and dbias entry lies within
the derived bound c * 2^-24 * A of the fp64 reference; dweight, dbias and the workspace - exactly the
queried bytes - keep the sentinel bands around them; no entry keeps its NaN fill; an accumulate call
equals seed + the plain call's result bit for bit (one fp32 addition per entry).  Per row: a second
run and phase 1 followed by phase 2 are bitwise the single call.  Rejected calls return their status
and write nothing.

Each test prints its error / bound ratio; test_headroom_per_kernel prints the maximum per kernel
(the record in DESIGN.md comes from it).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_matrix as W  # noqa: E402

PAIRS = W.pairs()
assert len(PAIRS) == W.PAIR_COUNT
HEADROOM = {}


def _plain_within_bound(c, bias, view):
    """the plain call of (row, bias_mode, alignment) - run once - against the reference"""
    res = W.plain(c.name, bias, view)
    assert res.rc == 0, res.rc
    assert res.plan == W.PLANS[c.name][bias], "the row is planned off its kernel: %s" % (res.plan,)
    assert res.intact, "sentinels around dweight, dbias or the workspace were overwritten"
    assert not bool(res.dw.isnan().any()), "dweight keeps part of its NaN fill"
    ref = W.reference(c.name, bias)
    rw = W.ratio(res.dw, ref.dw, ref.mag_w, W.bound_c(c, bias)).max().item()
    rb = 0.0
    if bias:
        assert not bool(res.db.isnan().any()), "dbias keeps part of its NaN fill"
        rb = W.ratio(res.db, ref.db, ref.mag_b, W.bias_c(c, bias)).max().item()
    HEADROOM[c.kernel] = max(HEADROOM.get(c.kernel, 0.0), rw, rb)
    print("%s [%s | bias %d%s]: dweight %.3g dbias %.3g of the bound" % (c.kernel, c.name, bias, " view" if view else "", rw, rb))
    assert rw <= 1.0, "dweight off the fp64 reference: %.3g x the bound" % rw
    assert rb <= 1.0, "dbias off the fp64 reference: %.3g x the bound" % rb
    return res


@pytest.mark.parametrize("name,form", PAIRS, ids=["%s | %s" % p for p in PAIRS])
def test_kernel_times_form(name, form):
    c = W.CASE[name]
    f = W.FORMS[c.layout][form]
    base = _plain_within_bound(c, f.bias, f.view)
    if not f.acc:
        return
    v = W.values(name)
    res = W.run(c, f)
    assert res.rc == 0 and res.plan == W.PLANS[name][f.bias] and res.intact
    assert torch.equal(res.dw, torch.add(v["seed_w"], base.dw)), "accumulate is not one fp32 addition onto the seed"
    if f.bias:
        assert torch.equal(res.db, torch.add(v["seed_b"][f.bias], base.db))


def _bits(t):
    return None if t is None else t.view(torch.int32)


@pytest.mark.parametrize("name", [c.name for c in W.CASES])
def test_second_run_and_phase_split_are_bitwise(name):
    c = W.CASE[name]
    f = W.forms(c)[0][1]
    first = W.plain(name, f.bias, f.view)
    for what, res in (("a second run", W.run(c, f)), ("phase 1 then phase 2", W.run(c, f, phases=True))):
        assert res.rc == 0 and res.intact
        assert torch.equal(_bits(res.dw), _bits(first.dw)), "%s differs in dweight" % what
        assert f.bias == 0 or torch.equal(_bits(res.db), _bits(first.db)), "%s differs in dbias" % what


INVALID, WORKSPACE = -1, -4
REJECTED = [
    # (row, form, what the call changes, status)
    ("dma 64x128 fq 32+16", "b1", dict(ws_short=1), WORKSPACE),
    ("dma 64x128 fq 32+16", "b1", dict(ws_null=True), WORKSPACE),
    ("small 8+4->16", "b1", dict(ws_short=1), WORKSPACE),
    ("wino cols gate 128->128", "b1", dict(ws_short=1), WORKSPACE),
    ("bf16 halo<2> 64+64->128", "b1", dict(ws_short=1), WORKSPACE),
    ("bf16 32+24->40", "b1", dict(ws_null=True), WORKSPACE),
    ("dma 64x128 fq 32+16", "b1", dict(rows_off=1), INVALID),           # rows 4 bytes off alignment
    ("reg 64x64 3->16", "b1", dict(rows_off=1), INVALID),
    ("bf16 32+24->40", "b1", dict(rows_off=1), INVALID),
    ("dma 64x128 fq 32+16", "b1", dict(src0_off=1), INVALID),           # a float4 row: src0 4 bytes off
    ("halo<1> 64->64", "b0", dict(src0_off=1), INVALID),
    ("dma 64x64 fq", "b1", dict(math=2), INVALID),                      # math 2 off the stem
    ("small 1->4", "b1", dict(math=2), INVALID),                        # ... a single channel, but n = 4
    ("dma 64x64 fq", "b1", dict(n=30), INVALID),                        # n % 4
    ("bf16 40->72, 2 splits", "b1", dict(n=68), INVALID),               # n % 8 on the bf16 entry
    ("dma 64x64 fq", "b1", dict(dbias_null=True), INVALID),
    ("dma 64x64 ConvT2", "b2", dict(dbias_null=True), INVALID),
    ("bf16 ConvT2 32->64", "b2", dict(dbias_null=True), INVALID),
]


@pytest.mark.parametrize("name,form,change,status", REJECTED,
                         ids=["%s | %s" % (n, ",".join("%s=%s" % kv for kv in ch.items())) for n, _, ch, _ in REJECTED])
def test_rejected_call_writes_nothing(name, form, change, status):
    c = W.CASE[name]
    res = W.run(c, W.FORMS[c.layout][form], **change)
    assert res.rc == status, res.rc
    assert res.untouched and res.intact, "a rejected call wrote to an output or to the workspace"


def test_headroom_per_kernel():
    """the worst error / bound ratio of each kernel over the pairs run so far in this process"""
    for kernel in sorted(HEADROOM):
        print("headroom %-44s %.3g" % (kernel, HEADROOM[kernel]))
    assert set(HEADROOM) <= {c.kernel for c in W.CASES}
    assert all(r <= 1.0 for r in HEADROOM.values())
