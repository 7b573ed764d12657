"""CPU checks of the packed-operand state machine (punet/packs.py): which operands a repack
refreshes, when a stale direct operand is repacked, and what the cache hits on.  No GPU and no
library launch: PackedWeights are built from small CPU tensors, and kernels.pack_weight /
pack_weights / pack_wino are replaced by recorders."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))

from punet import kernels as K  # noqa: E402
from punet import packs  # noqa: E402
from punet.packs import KEPT, WINO_FRESH, WINO_STALE, PackedWeight, Packs  # noqa: E402

BF = torch.bfloat16


def operand(w, mode=0, k_pad=None, cgroup=0, dtype=torch.float32, wino=False):
    """A PackedWeight of CPU parameter w with buffers of the right kinds (their content is never read)."""
    k_pad = k_pad or K.round16(w[0].numel())
    rows = w.shape[0]
    planes = torch.zeros(k_pad // 16, 6, rows, 8, dtype=BF) if dtype == torch.float32 else None
    return PackedWeight(w, mode, k_pad, cgroup, torch.zeros(rows, k_pad, dtype=dtype), planes,
                        torch.zeros(16, dtype=BF) if wino else None)


@pytest.fixture
def calls(monkeypatch):
    """The launches the code under test asks for, in order: ("pack_weights", operands, wino),
    ("pack_wino", jobs) or ("pack_weight", w, mode, k_pad, cgroup, dtype).  The library is out of reach."""
    log = []

    def no_lib():
        raise AssertionError("the library was touched")

    def pack_weights(jobs, wino=True):
        log.append(("pack_weights", list(jobs), wino))
        for p in jobs:             # as the launch wrapper does
            p.direct_repacked()

    def pack_weight(w, mode, k_pad, cgroup=0, dtype=torch.float32):
        log.append(("pack_weight", w, mode, k_pad, cgroup, dtype))
        return operand(w, mode, k_pad, cgroup, dtype, wino=dtype == torch.float32 and w.shape[0] % 64 == 0)

    monkeypatch.setattr(K, "lib", no_lib)
    monkeypatch.setattr(K, "pack_weights", pack_weights)
    monkeypatch.setattr(K, "pack_wino", lambda jobs: log.append(("pack_wino", list(jobs))))
    monkeypatch.setattr(K, "pack_weight", pack_weight)
    return log


def three(pk):
    """A KEPT, a WINO_FRESH and a bf16 KEPT operand in pk, through get()."""
    ws = [torch.ones(8, 4, 3, 3), torch.ones(64, 32, 3, 3), torch.ones(8, 4, 3, 3)]
    ops = [pk.get(ws[0], 0, 48), pk.get(ws[1], 1, 576, 32), pk.get(ws[2], 0, 64, 0, BF)]
    return ws, ops


def test_creation_state():
    w = torch.ones(8, 4, 3, 3)
    w.add_(0)
    p, q = operand(w), operand(w, wino=True)
    assert (p.state, q.state) == (KEPT, WINO_FRESH)
    assert p.version == w._version == 1 and p.src is w
    assert (p.mode, p.k_pad, p.cgroup, p.dtype) == (0, 48, 0, torch.float32)
    assert p.data_ptr() == p.direct.data_ptr()
    assert operand(w, dtype=BF).dtype == BF and operand(w, dtype=BF).planes is None
    with pytest.raises(AttributeError):       # __slots__: no state can be hung on the side
        p.stale = True


def test_refresh_after_version_bump(calls):
    pk = Packs()
    ws, (kept, fresh, bf) = three(pk)
    assert [p.state for p in (kept, fresh, bf)] == [KEPT, WINO_FRESH, KEPT]
    del calls[:]
    for w in ws:
        w.add_(0)
    pk.refresh()
    assert len(calls) == 2
    name, jobs, wino = calls[0]
    assert name == "pack_weights" and wino is False
    assert len(jobs) == 2 and jobs[0] is kept and jobs[1] is bf
    name, ujobs = calls[1]
    assert name == "pack_wino" and len(ujobs) == 1
    assert ujobs[0][0] is ws[1] and ujobs[0][1] is fresh.wino and ujobs[0][2] is True      # mode 1: dgrad
    assert [p.state for p in (kept, fresh, bf)] == [KEPT, WINO_STALE, KEPT]
    assert [p.version for p in (kept, fresh, bf)] == [w._version for w in ws] == [1, 1, 1]
    # a second refresh without a bump makes no calls
    del calls[:]
    pk.refresh()
    assert calls == []


def test_direct_call_on_a_stale_operand(calls):
    pk = Packs()
    ws, (kept, fresh, bf) = three(pk)
    ws[1].add_(0)
    pk.refresh()
    assert fresh.state == WINO_STALE
    del calls[:]
    K.direct_call(fresh)
    assert len(calls) == 1
    name, jobs, wino = calls[0]
    assert name == "pack_weights" and wino is False and len(jobs) == 1 and jobs[0] is fresh
    assert fresh.state == KEPT
    # from now on it is in the direct job list of a refresh, and its U still is refreshed
    del calls[:]
    ws[1].add_(0)
    pk.refresh()
    assert len(calls) == 2
    assert calls[0][0] == "pack_weights" and calls[0][2] is False
    assert len(calls[0][1]) == 1 and calls[0][1][0] is fresh
    assert calls[1][0] == "pack_wino" and len(calls[1][1]) == 1 and calls[1][1][0][1] is fresh.wino
    assert fresh.state == KEPT and fresh.version == ws[1]._version == 2


def test_direct_call_on_a_fresh_operand(calls):
    p = operand(torch.ones(64, 32, 3, 3), wino=True)
    assert p.state == WINO_FRESH
    K.direct_call(p)
    assert calls == [] and p.state == KEPT
    K.direct_call(p)                          # and on a KEPT one
    assert calls == [] and p.state == KEPT


def test_transitions():
    """The three methods over the three states, one row each."""
    def at(state):
        p = operand(torch.ones(64, 32, 3, 3), wino=True)
        p.state = state
        return p
    for state, due, after in ((KEPT, (True, True), KEPT), (WINO_FRESH, (False, True), WINO_STALE),
                              (WINO_STALE, (False, True), WINO_STALE)):
        p = at(state)
        assert p.repack_due() == due and p.state == after, state
    for state, repack in ((KEPT, False), (WINO_FRESH, False), (WINO_STALE, True)):
        p = at(state)
        assert p.take_direct() is repack and p.state == KEPT, state
    for state, after in ((KEPT, KEPT), (WINO_FRESH, WINO_FRESH), (WINO_STALE, WINO_FRESH)):
        p = at(state)
        p.direct_repacked()
        assert p.state == after, state
    p = operand(torch.ones(8, 4, 3, 3))       # no U
    assert p.repack_due() == (True, False) and p.state == KEPT


def test_lazy_direct_off(calls, monkeypatch):
    monkeypatch.setattr(packs, "_LAZY", False)
    pk = Packs()
    ws, (kept, fresh, bf) = three(pk)
    for step in (1, 2):
        del calls[:]
        for w in ws:
            w.add_(0)
        pk.refresh()
        assert len(calls) == 2
        name, jobs, wino = calls[0]
        assert name == "pack_weights" and wino is False
        assert len(jobs) == 3 and jobs[0] is kept and jobs[1] is fresh and jobs[2] is bf
        assert calls[1][0] == "pack_wino" and len(calls[1][1]) == 1 and calls[1][1][0][1] is fresh.wino
        assert fresh.state != WINO_STALE and fresh.version == step
    K.direct_call(fresh)                      # has nothing to repack
    assert len(calls) == 2 and fresh.state == KEPT


def test_refresh_skips_a_moved_parameter(calls):
    pk = Packs()
    ws, (kept, fresh, bf) = three(pk)
    del calls[:]
    for w in ws:
        w.add_(0)
    ws[0].data = torch.ones(8, 4, 3, 3)       # new storage: the entry's key no longer names it
    assert kept.src.data_ptr() != next(k for k, p in pk.cache.items() if p is kept)[0]
    pk.refresh()
    assert len(calls) == 2
    assert len(calls[0][1]) == 1 and calls[0][1][0] is bf
    assert kept.version == 0 and bf.version == 1 and fresh.version == 1


def test_get(calls):
    pk = Packs()
    w = torch.ones(8, 4, 3, 3)
    p = pk.get(w, 0, 48)
    assert len(calls) == 1 and calls[0][0] == "pack_weight" and calls[0][1] is w
    assert calls[0][2:] == (0, 48, 0, torch.float32) and p.src is w
    assert pk.get(w, 0, 48) is p and pk.get(w.detach(), 0, 48) is p and len(calls) == 1
    q = pk.get(w, 0, 64)                      # another k_pad
    assert q is not p and q.k_pad == 64 and len(calls) == 2
    assert pk.get(w, 0, 64) is q and len(calls) == 2
    w.add_(0)                                 # a stale version
    r = pk.get(w, 0, 64)
    assert r is not q and r.version == 1 and len(calls) == 3
    assert pk.get(w, 1, 64) is not r and len(calls) == 4      # another layout: another entry
    assert pk.get(w, 0, 64) is r and len(calls) == 4


def test_igemm_refuses_a_bare_tensor(calls):
    x = torch.zeros(1, 4, 4, 16)
    with pytest.raises(TypeError, match="PackedWeight"):
        K.igemm(batch=1, in_hw=(4, 4), out_hw=(4, 4), k=3, stride=1, pad=1, src0=x, c0=16,
                weight=torch.zeros(16, 144), k_pad=144, n=16, dst0=torch.zeros(1, 4, 4, 16))
    assert calls == []
