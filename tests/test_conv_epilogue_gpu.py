"""Every conv kernel against every epilogue form it can be given (case table, reference and bounds:
tests/conv_epilogue.py; their CPU self-checks: test_conv_epilogue.py).

fp32 entry, two levels per (case, form):
  GEMM level      the call with identity values (same pointers, same flags minus ReLU; bias 0,
                  resid 0, masks 1, scale 1, seed 0) against the fp64 convolution, at the project's
                  fp32 conv tolerance (rtol 1e-4, atol 1e-5 max|ref|).  Dispatch reads presence and
                  alignment, never values, so it runs the real call's kernel instantiation - asserted
                  through the tile query - and returns its raw accumulators z.
  epilogue level  the real call against the fp64 epilogue of that z, |got - exp| <= 4 * 2^-24 * S
                  per element (S bounds the intermediates): free of accumulation-order noise, so a
                  wrong bias channel, a swapped mask element or a misrouted fragment fails at any size.
bf16 entry, one level: the fp64 reference on the bf16-rounded operands, one round-to-nearest bf16
store on top of the fp32 tolerance.
Both entries: masked-off outputs are exactly 0 (the seed bit for bit under ACCUM), outputs under ReLU
are >= 0 (>= the seed); every destination and the workspace sit between 4096 sentinel floats that
must survive bit for bit; without ACCUM the destination starts as NaN and none may remain.

Each test prints its worst error / bound ratio (the record of headroom in DESIGN.md comes from it).
"""
import pytest

pytestmark = pytest.mark.gpu

import conv_epilogue as E  # noqa: E402

PAIRS = E.pairs()


def _id(p):
    return "%s | %s%s" % (p[0], p[1], " | split-K" if p[2] else "")


@pytest.mark.parametrize("name,form,scratch", PAIRS, ids=[_id(p) for p in PAIRS])
def test_kernel_times_epilogue(name, form, scratch):
    c = E.CASE[name]
    ops = E.FORMS[c.layout][form]
    want_plan = c.plan if scratch else c.plan[:3] + (1,)
    ref = E.reference(name)
    o = E.operands(c, ops)
    real = E.run(c, ops, scratch)
    assert real.rc == 0, real.rc
    assert real.plan == want_plan, "the row is planned off its kernel: %s" % (real.plan,)
    assert real.intact, "sentinels around a destination or the workspace were overwritten"
    assert not bool(real.out.isnan().any()), "the destination keeps part of its NaN fill"
    if c.entry == "f32":
        neutral = E.run(c, ops, scratch, neutral=True)
        assert neutral.rc == 0 and neutral.plan == real.plan and neutral.intact
        z = neutral.out
        r_gemm, r_epi = E.gemm_ratio(z, ref), E.epilogue_ratio(real.out, z, o)
        print("%s [%s]: gemm %.3g epilogue %.3g of the bound" % (c.kernel, _id((name, form, scratch)), r_gemm, r_epi))
        assert r_gemm <= 1.0, "accumulators off the fp64 convolution: %.3g x the tolerance" % r_gemm
        assert r_epi <= 1.0, "epilogue off the fp64 epilogue of its own accumulators: %.3g x the bound" % r_epi
    else:
        r = E.bf16_ratio(real.out, E.epilogue64(ref, o))
        print("%s [%s]: bf16 %.3g of the bound" % (c.kernel, _id((name, form, scratch)), r))
        assert r <= 1.0, "off the fp64 reference: %.3g x the bound" % r
    E.check_exact(real.out, o)


# one representative of each pair the API rejects: PU_ERR_INVALID, and nothing written
REJECTED = [
    ("x6 lean 128x64 32->48 n0 16", {"resid"}),              # RESID with a split
    ("x6 ConvT2 64->4x32", {"bias", "resid"}),               # RESID with SHUFFLE2
    ("bf16 lean 64->64", {"cscale", "mask0"}),               # chan_scale on the bf16 entry
    ("bf16 lean 64+64->96 n0 32", {"resid"}),
    ("bf16 ConvT2 64->4x32", {"bias", "resid"}),
]


@pytest.mark.parametrize("name,ops", REJECTED, ids=["%s | %s" % (n, "+".join(sorted(o))) for n, o in REJECTED])
def test_rejected_pair_writes_nothing(name, ops):
    c = E.CASE[name]
    assert E.excluded(c, ops)
    res = E.run(c, frozenset(ops))
    assert res.rc == -1                                      # PU_ERR_INVALID
    assert res.untouched and res.intact
