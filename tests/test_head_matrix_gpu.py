"""Every kernel of csrc/plastic.hip and csrc/adam.hip, in every form it can be given, against fp64 (case
table, references, bounds and runner: tests/head_matrix.py; their CPU checks: test_head_matrix.py).

Per (row, form): the call returns PU_OK; every entry of every output lies within its derived bound of
the reference (bound 0: bit for bit); every destination and the workspace - exactly the queried
bytes, NaN-filled - keep the sentinel bands around them; no entry the call must write keeps its NaN
fill (a partial read unwritten would leave one); deta without dhebb_out keeps its fill; hebb (when not
aliased) and Adam's g are unchanged.  The bit-exact classes: H' from the call's own X[:, 0] and
Y[:, 0] on every row that writes one (the fused head's serial and pipelined kernels and the R = 32
rows included), dw / dalpha as the in-order fp32 slot sum of the slab the call left in the workspace,
dhebb without dhebb_out as alpha times that slab.  The identities: the fused head is pu_outconv_fwd
then pu_plastic_fwd; pu_plastic_fwd's Y does not depend on the form; pu_plastic_bwd_trace without
dhebb_out is pu_plastic_bwd; the pipelined head is the serial one (a PU_HEAD_PIPE=0 child process).
A second run is bitwise the first.  Rejected calls return their status and write nothing.

Each test prints its error / bound ratio; test_headroom_per_output prints the maximum per output (the
record in DESIGN.md comes from it).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_matrix as M  # noqa: E402

PAIRS = M.pairs()
assert len(PAIRS) == M.PAIR_COUNT
HEADROOM = {}
F32 = torch.float32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _checked(r, fname, res):
    """status, bands, fill, inputs and every output against the reference of (row, form)"""
    assert res.rc == M.OK, res.rc
    assert res.intact, "sentinels around a destination or the workspace were overwritten"
    assert not res.kept, "an output keeps part of its NaN fill"
    assert res.extra, "deta was written without dhebb_out"
    assert res.same, "an input was changed"
    ref = M.reference(r.name, fname)
    assert set(ref) == set(res.outs), (sorted(ref), sorted(res.outs))
    for out, (val, bound) in ref.items():
        q = M.ratio(res.outs[out], val, bound).max().item()
        print("%s [%s | %s] %s: %.3g of the bound" % (r.entry, r.name, fname, out, q))
        assert q <= 1.0, "%s off the reference: %.3g x the bound" % (out, q)
        if bool((bound > 0).any()):
            HEADROOM[r.entry, out] = max(HEADROOM.get((r.entry, out), 0.0), q)
    return res


def _two_launch(r, f):
    """pu_outconv_fwd, then pu_plastic_fwd, on the operands of head row r"""
    from punet import kernels as K
    L, p, v, s = M._lib.load(), r.p, M.values(r.name), K._stream()
    feat = v["feat"].to(M._DT[p.dt]).cuda()
    wo, bo, H, w, al, eta = (v[k].cuda() for k in ("wo", "bo", "H", "w", "al", "eta"))
    nn = p.B * p.N * p.N
    X, Y, Hn = (torch.full((nn,), float("nan"), device="cuda") for _ in range(3))
    fn = L.pu_outconv_fwd_bf16 if p.dt == "bf16" else L.pu_outconv_fwd
    assert fn(feat.data_ptr(), wo.data_ptr(), bo.data_ptr() if f.bias else None, X.data_ptr(), nn, p.C, s) == M.OK
    a = M._lib.PlasticArgs(p.B, p.N, X.data_ptr(), H.data_ptr(), w.data_ptr(), al.data_ptr(), eta.data_ptr(), Y.data_ptr(),
                           Hn.data_ptr() if f.train else None, p.rule)
    assert L.pu_plastic_fwd(ctypes.byref(a), s) == M.OK
    torch.cuda.synchronize()
    return {"X": X.cpu(), "Y": Y.cpu(), "Hn": Hn.cpu()}


def _slot_sum(slab):
    """head_dw_reduce_kernel: 0 + slot 0 + slot 1 ... in float32, strictly in order"""
    terms = np.concatenate([np.zeros((1,) + slab.shape[1:], dtype=np.float32), slab])
    return torch.from_numpy(np.add.accumulate(terms, axis=0, dtype=np.float32)[-1].copy())


@pytest.mark.parametrize("name,form", PAIRS, ids=["%s | %s" % p for p in PAIRS])
def test_row_times_form(name, form):
    r = M.CASE[name]
    p = r.p
    f = M.FORMS[r.entry][form]
    res = _checked(r, form, M.run(r, f))
    v = M.values(name)
    o = res.outs
    if "Hn" in o:
        # the trace update from the call's own row 0 of X and Y, bit for bit
        shape = (p.B, p.N, p.N)
        X = o["X"].reshape(shape) if "X" in o else v["X"]
        Y = o["Y"].reshape(shape) if "Y" in o else v["Y"]
        want = M.trace_np(v["H"], X[:, 0], Y[:, 0], v["eta"], p.rule)
        assert torch.equal(_bits(o["Hn"]), _bits(want.reshape(-1))), "H' is not the float32 trace rule of the call's own X[0], Y[0]"
    if r.entry == "head":
        two = _two_launch(r, f)
        for k in o:
            assert torch.equal(_bits(o[k]), _bits(two[k])), "%s differs from pu_outconv_fwd, then pu_plastic_fwd" % k
    if r.entry == "fwd" and f.train:
        plain = M.run(r, M.FORMS["fwd"]["no hebb_out"])
        assert plain.rc == M.OK and torch.equal(_bits(plain.outs["Y"]), _bits(o["Y"])), "Y depends on the form"
    if r.entry in ("bwd", "bwdt") and (f.dw or f.dh):
        nn = p.N * p.N
        slab = res.ws[:2 * p.B * nn].reshape(p.B, 2, nn).numpy()
        assert not np.isnan(slab).any(), "the slab keeps part of its NaN fill"
        if f.dw:
            assert torch.equal(_bits(o["dw"]), _bits(_slot_sum(slab[:, 0]))), "dw is not the in-order slot sum of the slab"
            assert torch.equal(_bits(o["dalpha"]), _bits(_slot_sum(slab[:, 1]))), "dalpha is not the in-order slot sum"
        if p.data == "zero_h" and f.dw:
            assert torch.count_nonzero(o["dalpha"]).item() == 0
    if r.entry == "bwdt" and not f.P:
        # no gradient reached H': pu_plastic_bwd's own kernels, bit for bit; dhebb = alpha T_b
        base = M.run(M.Row(name, "bwd", None, p), M.FORMS["bwd"]["both"])
        assert base.rc == M.OK and base.intact
        for k in ("dx", "dw", "dalpha"):
            assert torch.equal(_bits(o[k]), _bits(base.outs[k])), "%s differs from pu_plastic_bwd" % k
        want = (v["al"].reshape(1, -1).numpy() * slab[:, 0]).astype(np.float32)
        assert torch.equal(_bits(o["dhebb"]), _bits(torch.from_numpy(want).reshape(-1)))


@pytest.mark.parametrize("name", [r.name for r in M.CASES])
def test_a_second_run_is_bitwise_the_first(name):
    r = M.CASE[name]
    f = M.forms(r)[0][1]
    first, second = M.run(r, f), M.run(r, f)
    assert first.rc == M.OK and second.rc == M.OK and first.intact and second.intact
    assert set(first.outs) == set(second.outs)
    for out in first.outs:
        assert torch.equal(_bits(first.outs[out]), _bits(second.outs[out])), "%s differs between two runs" % out


def test_pipelined_head_equals_the_serial_kernel(tmp_path):
    """PU_HEAD_PIPE is read once per process: one fresh child process runs the N = 128, C = 64 / 96 rows
    on the serial kernel and leaves X, Y, H' in tmp_path; they are the pipelined kernel's bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ("import sys; sys.path[:0] = %r; import head_matrix as M; M.serial_child(sys.argv[1])"
            % [here, os.path.join(root, "plastic-unet_amd"), root])
    child = subprocess.run([sys.executable, "-c", code, str(tmp_path)], env=dict(os.environ, PU_HEAD_PIPE="0"),
                           capture_output=True, text=True, timeout=240)
    assert child.returncode == 0, "the child failed (%d):\n%s" % (child.returncode, child.stderr[-2000:])
    for i, name in enumerate(M.PIPE_AB):
        r = M.CASE[name]
        assert "head_pipe_fwd_kernel<%s>" % M._T[r.p.dt] in r.kernels
        serial = torch.load(os.path.join(str(tmp_path), "%d.pt" % i))
        res = M.run(r, M.FORMS["head"]["train"])
        assert res.rc == M.OK and set(res.outs) == set(serial) == {"X", "Y", "Hn"}
        for k in serial:
            assert torch.equal(_bits(res.outs[k]), _bits(serial[k])), (name, k)


# ---- rejected calls: one per PU_REQUIRE / workspace line of the two files
def _rej(base, form, status, **over):
    return M.CASE[base], form, over, status


H32, HBF, HPIPE = "head f32 B 2 N 48 C 8 oja", "head bf16 B 2 N 16 C 8 hebb", "head f32 B 1 N 128 C 64 hebb"
FW, TRC, BW, BT = "fwd B 2 N 17 oja", "trace v4 N 16", "bwd B 2 N 17", "bwdt B 2 N 34 hebb"
BCF, BCB, AD, AD33 = "bce fwd n 257", "bce bwd n 257", "adam sizes, step 1", "adam 33 tensors"
REJECTED = [
    _rej(TRC, "plain", M.INVALID, null=("hebb",)),
    _rej(TRC, "plain", M.INVALID, null=("hebb_out",)),
    _rej(TRC, "plain", M.INVALID, B=0),
    _rej(TRC, "plain", M.INVALID, rule=2),
    _rej(TRC, "plain", M.INVALID, N=46341),                       # nbf^2 >= 2^31
    _rej(FW, "fused", M.INVALID, null=("x",)),
    _rej(FW, "fused", M.INVALID, N=0),
    _rej(FW, "fused", M.INVALID, rule=2),
    _rej(FW, "fused", M.INVALID, null=("eta",)),                  # hebb_out without eta
    _rej(FW, "aliased", M.INVALID, null=("eta",)),
    _rej(H32, "train", M.INVALID, null=("feat",)),
    _rej(H32, "train", M.INVALID, rule=3),
    _rej(H32, "train", M.INVALID, N=24),                          # no multiple of 16
    _rej(H32, "train", M.INVALID, N=528),                         # > 512
    _rej(H32, "train", M.INVALID, N=0),
    _rej(H32, "train", M.INVALID, C=6),
    _rej(H32, "train", M.INVALID, C=0),
    _rej(H32, "train", M.INVALID, mis=("feat",)),
    _rej(H32, "train", M.INVALID, mis=("out_w",)),
    _rej(HBF, "train", M.INVALID, mis=("feat",)),                 # 4 bytes off the 8 its bf16 quads need
    _rej(HBF, "train", M.INVALID, mis=("out_w",)),
    _rej(H32, "train", M.INVALID, mis=("hebb",)),
    _rej(H32, "train", M.INVALID, mis=("w",)),
    _rej(H32, "eval", M.INVALID, mis=("alpha",)),
    _rej(H32, "train", M.INVALID, mis=("Hn",)),
    _rej(HPIPE, "train", M.INVALID, mis=("Hn",)),
    _rej(HPIPE, "train", M.INVALID, mis=("w",)),
    _rej(H32, "train", M.INVALID, null=("eta",)),                 # hebb_out without eta
    _rej(H32, "train", M.INVALID, alias=True),                    # hebb_out == hebb on the fused entry
    _rej(H32, "train", M.INVALID, B=4, N=512, C=1 << 20),         # 2^40 features
    _rej(BW, "both", M.INVALID, null=("dy",)),
    _rej(BW, "both", M.INVALID, null=("dalpha",)),                # dw without dalpha
    _rej(BW, "both", M.INVALID, null=("dw",)),
    _rej(BW, "both", M.WORKSPACE, ws_short=1),
    _rej(BW, "both", M.WORKSPACE, ws_null=True),
    _rej(BT, "all", M.INVALID, null=("x",)),
    _rej(BT, "all", M.INVALID, null=("dy", "dhebb_out")),         # neither gradient
    _rej(BT, "all", M.INVALID, rule=2),
    _rej(BT, "all", M.INVALID, null=("deta",)),                   # dhebb_out without deta
    _rej(BT, "all", M.INVALID, null=("eta",)),
    _rej(BT, "all", M.INVALID, N=46341),
    _rej(BT, "all", M.INVALID, B=65536),
    _rej(BT, "all", M.INVALID, null=("dalpha",)),
    _rej(BT, "all", M.INVALID, null=("dw",)),
    _rej(BT, "all", M.WORKSPACE, ws_short=1),
    _rej(BT, "all", M.WORKSPACE, ws_null=True),
    _rej(BT, "all", M.INVALID, ws_mis=True),                      # four bytes off 16-byte alignment
    _rej(BT, "no dhebb_out", M.WORKSPACE, ws_short=1),
    _rej(BCF, "plain", M.INVALID, null=("y",)),
    _rej(BCF, "plain", M.INVALID, null=("loss",)),
    _rej(BCF, "plain", M.INVALID, n=0),
    _rej(BCF, "plain", M.WORKSPACE, ws_short=1),
    _rej(BCF, "plain", M.WORKSPACE, ws_null=True),
    _rej(BCF, "plain", M.INVALID, ws_mis=True),                   # four bytes off the 8 its fp64 partials need
    _rej(BCB, "grad_loss", M.INVALID, null=("dy",)),
    _rej(BCB, "grad_loss", M.INVALID, null=("t",)),
    _rej(BCB, "grad_loss", M.INVALID, n=0),
    _rej(AD, "plain", M.INVALID, n_tensors=-1),
    _rej(AD, "plain", M.INVALID, adam_null=True),
    _rej(AD, "plain", M.INVALID, adam_bad=(3, "numel")),
    _rej(AD, "plain", M.INVALID, adam_bad=(6, "grad")),
    _rej(AD33, "plain", M.INVALID, adam_bad=(32, "exp_avg")),     # in the second launch: the first 32 stay unstepped
    _rej(AD33, "plain", M.INVALID, adam_bad=(32, "numel")),
]


@pytest.mark.parametrize("r,form,over,status", REJECTED,
                         ids=["%s | %s" % (r.name, ",".join("%s=%s" % kv for kv in o.items())) for r, _, o, _ in REJECTED])
def test_rejected_call_writes_nothing(r, form, over, status):
    res = M.run(r, M.FORMS[r.entry][form], **over)
    assert res.rc == status, res.rc
    assert res.untouched and res.intact and res.same, "a rejected call wrote to an output, to the workspace or to an input"


def test_headroom_per_output():
    """the worst error / bound ratio of each output of each entry point over the pairs run so far in
    this process (outputs with a bound of 0 are bit for bit and not part of the figure)"""
    for entry, out in sorted(HEADROOM):
        print("headroom %-8s %-8s %.3g" % (entry, out, HEADROOM[entry, out]))
    assert {e for e, _ in HEADROOM} <= set(M.FORMS)
    assert all(q <= 1.0 for q in HEADROOM.values())
