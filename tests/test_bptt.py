"""CPU side of backpropagation through the plastic trace: the new C-ABI entry validates its
arguments without touching the GPU, the constructors take trace_grad, --bptt parses, and the
oracle's un-detached trace path is pinned to the reference's own outputs
(tests/golden/bptt_{hebb,oja}.npz, written by tests/golden/gen_golden_bptt.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import golden, PKG

torch.set_num_threads(4)


def test_new_entry_rejects_bad_arguments_without_gpu():
    from punet import _lib
    lib = _lib.load()
    A = 0x10000          # aligned stand-in pointers: validation never dereferences them
    assert lib.pu_plastic_bwd_trace(None, None, 0, None) == -1
    assert lib.pu_plastic_bwd_trace(ctypes.byref(_lib.PlasticBwdTraceArgs()), None, 0, None) == -1
    assert b"pu_plastic_bwd_trace: bad args" in lib.pu_last_error()

    def args(**kw):
        a = _lib.PlasticBwdTraceArgs(2, 16, 0, A, A, A, A, A, A, A, A, A, A, A, A, A)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    need = lib.pu_plastic_bwd_trace_workspace_bytes(2, 16)
    assert need >= 2 * 2 * 16 * 16 * 4 and lib.pu_plastic_bwd_trace_workspace_bytes(0, 16) == 0
    for field in ("x", "hebb", "w", "alpha", "y"):
        assert lib.pu_plastic_bwd_trace(ctypes.byref(args(**{field: None})), A, need, None) == -1, field
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(dy=None, dhebb_out=None)), A, need, None) == -1
    assert b"neither dy nor dhebb_out" in lib.pu_last_error()
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(rule=7)), A, need, None) == -1
    assert b"Must select one learning rule" in lib.pu_last_error()
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(deta=None)), A, need, None) == -1
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(eta=None)), A, need, None) == -1
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(dalpha=None)), A, need, None) == -1
    assert b"dw and dalpha go together" in lib.pu_last_error()
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args(nbf=1 << 16)), A, need, None) == -1
    assert b"nbf too large" in lib.pu_last_error()
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args()), A, need - 1, None) == -4
    assert lib.pu_plastic_bwd_trace(ctypes.byref(args()), None, need, None) == -4
    assert b"workspace" in lib.pu_last_error()
    assert lib.pu_abi_version() == 3


def test_trace_args_struct_matches_header():
    import re
    from punet import _lib
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "plastic_unet.h")).read()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^}]*)\}\s*(\w+);", src))["pu_plastic_bwd_trace_args"]
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = re.sub(r"\bconst\b", "", decl.strip())
        if decl:
            fields += [re.sub(r"[\*\s]", " ", part).split()[-1] for part in decl.split(",")]
    assert fields == [f for f, _ in _lib.PlasticBwdTraceArgs._fields_]


def test_constructors_take_trace_grad():
    from unet import UNetp, UNetpRes
    from unet.coord_conv import CoordConvUNetp
    cpu = torch.device("cpu")
    for ctor in (lambda **k: UNetp(1, 1, cpu, nbf=32, **k), lambda **k: UNetpRes(1, 1, cpu, neurons=4, nbf=32, **k),
                 lambda **k: CoordConvUNetp(1, 1, cpu, nbf=32, **k)):
        assert ctor().trace_grad is False
        net = ctor(trace_grad=True)
        assert net.trace_grad is True
        assert list(net.state_dict()) == list(ctor().state_dict())     # not part of the state_dict
    for cls, kw in ((UNetp, {}), (UNetpRes, {"neurons": 4})):
        with pytest.raises(ValueError, match="trace_grad=True needs hebb_mode='slots'"):
            cls(1, 1, cpu, nbf=32, hebb_mode="sequential", trace_grad=True, **kw)
        assert cls(1, 1, cpu, nbf=32, hebb_mode="sequential", **kw).trace_grad is False


def test_step_episode_needs_trace_grad():
    from unet import UNetp
    from punet.engine import Trainer
    net = UNetp(1, 1, torch.device("cpu"), nbf=32)
    tr = Trainer(net, flat_grads=False)
    with pytest.raises(ValueError, match="trace_grad=True"):
        tr.step_episode([torch.zeros(1, 1, 32, 32)], [torch.zeros(1, 32, 32)], torch.zeros(1, 32, 32))


def test_bptt_option_parses():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train
    assert train.parse_args(["-o", "x"]).bptt == 0
    assert train.parse_args(["-o", "x", "--bptt", "4"]).bptt == 4


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().numpy() if torch.is_tensor(a) else np.asarray(a), np.asarray(b),
                               rtol=rtol, atol=atol)


@pytest.mark.parametrize("rule", ["hebb", "oja"])
@pytest.mark.parametrize("live", [True, False])
def test_oracle_undetached_episode_matches_reference(rule, live):
    """The reference UNetp over a 3-sample episode, hebb carried as returned (live) or detached
    between the samples (cut): RefUNetp reproduces its losses, final trace and gradients - eta's
    among them on the live path - at test_oracle_golden.py's tolerances."""
    g = golden("bptt_%s.npz" % rule)
    torch.manual_seed(0)
    net = oracle.RefUNetp(1, 1, rule=rule, nbf=64)      # test_unetp_c8_init_matches_reference_rng pins this init
    with torch.no_grad():
        net.alpha.copy_(_t(g["alpha"]))
        net.eta.copy_(_t(g["eta"]))
    tag = "live." if live else "cut."
    hebb = _t(g["hebb0"])
    losses = []
    for k in range(3):
        y, hebb = net(_t(g["xs"][k]), hebb if live else hebb.detach())
        losses.append(oracle.bce_loss(y, _t(g["ts"][k].astype(np.float32))))
    (sum(losses) / 3).backward()
    np.testing.assert_allclose([l.item() for l in losses], g[tag + "losses"], rtol=1e-6)
    _close(hebb, g[tag + "hebb"], rtol=1e-4, atol=1e-6)
    assert (net.eta.grad is not None) == live and (tag + "g.eta" in g) == live
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        if tag + "g." + k in g:
            _close(p.grad, g[tag + "g." + k], rtol=1e-4, atol=1e-7)
        else:
            gg = p.grad.double()
            got = np.array([gg.sum().item(), gg.abs().sum().item(), gg.norm().item()])
            want = g[tag + "gsum." + k]
            np.testing.assert_allclose(got[1:], want[1:], rtol=1e-4)
            np.testing.assert_allclose(got[0], want[0], rtol=1e-3, atol=1e-6 * got[1])
    if live:
        # eta's gradient exists only through the trace path: compared above, and not a zero
        assert abs(float(g["live.g.eta"][0])) > 0 and not np.array_equal(g["live.g.w"], g["cut.g.w"])
