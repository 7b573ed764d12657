"""CPU checks of the Lovasz loss (csrc/lovasz.hip, kernels.lovasz_fwd / lovasz_bwd, punet.head, the
Trainer's loss selection, train.py --loss): the numpy restatement of the contract (tests/lovasz_ref.py)
against Berman's cumsum form, the vertex property and a finite difference; the workspace formula and the
argument validation of the C-ABI without a device; the plumbing; the kernel set of the build."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import lovasz_ref as R

A = 0x10000          # 16-byte aligned stand-in pointer: validation never dereferences it


# ---- the restatement
def _grid(g, n):
    """n different probabilities (4 k + 5) / M, M the power of two >= 4 n + 8: 1 - y is exact in fp32, and
    no y equals another's 1 - y (4 (i + j) + 10 = M has no solution), so the errors never tie and lie at
    least 2 / M apart"""
    M = 1 << int(np.ceil(np.log2(4 * n + 8)))
    return ((4 * g.permutation(n) + 5) / M).astype(np.float32)


@pytest.mark.parametrize("n,density", [(1, 1.0), (2, 0.5), (7, 0.0), (7, 1.0), (50, 0.3), (333, 0.6)])
def test_restatement_equals_bermans_cumsum_form(n, density):
    g = np.random.RandomState(n)
    y = _grid(g, n)
    t = (g.rand(n) < density).astype(np.float32)
    e = R.errors(y, t)
    assert len(np.unique(e)) == n                                   # tie-free
    loss, D = R.image(y, t)
    want, order, jac = R.berman(y, t)
    assert abs(loss - want) <= 1e-12                                # e is exact on the grid: the summation order only
    sign = np.where(R.foreground(t), -1.0, 1.0)
    dense = np.empty(n)
    dense[order] = jac
    assert np.array_equal(D, (sign * dense).astype(np.float32))     # the same counts, the same fp64 operations


@pytest.mark.parametrize("n", [1, 5, 64, 301])
def test_vertices_give_the_jaccard_loss(n):
    """y in {0, 1}: loss_b = 1 - |P and T| / |P or T|, 0 when both are empty - the defining property of
    the extension"""
    g = np.random.RandomState(100 + n)
    cases = [(g.rand(n) < 0.5, g.rand(n) < 0.5) for _ in range(4)]
    cases += [(np.zeros(n, bool), np.zeros(n, bool)), (np.ones(n, bool), np.zeros(n, bool)),
              (np.zeros(n, bool), np.ones(n, bool)), (np.ones(n, bool), np.ones(n, bool))]
    for p, t in cases:
        loss, _ = R.image(p.astype(np.float32), t.astype(np.float32))
        union = np.count_nonzero(p | t)
        want = 1.0 - np.count_nonzero(p & t) / union if union else 0.0
        assert abs(loss - want) <= 1e-12, (p, t)


def test_gradient_table_agrees_with_a_central_difference():
    n = 40
    g = np.random.RandomState(5)
    y = _grid(g, n)                                                 # M = 256: the errors lie 2^-7 apart or more
    t = (g.rand(n) < 0.4).astype(np.float32)
    assert np.diff(np.sort(R.errors(y, t))).min() >= 2.0 ** -7
    _, D = R.image(y, t)
    h = np.float32(2.0 ** -10)                                      # far below half a gap: the order holds; exact in fp32
    for i in range(n):
        up, dn = y.copy(), y.copy()
        up[i] += h
        dn[i] -= h
        fd = (R.image(up, t)[0] - R.image(dn, t)[0]) / float(up[i] - dn[i])
        # the loss is linear in y between two ties and e is exact here: the fp32 rounding of D (2^-24
        # relative) and the fp64 rounding of the two losses over 2 h are all that differs
        assert abs(fd - float(D[i])) <= 1e-7 * abs(fd) + 1e-10, i


def test_batch_mean_and_backward():
    g = np.random.RandomState(8)
    y, t = g.rand(3, 20).astype(np.float32), (g.rand(3, 20) < 0.5).astype(np.float32)
    loss, per, D = R.batch(y, t)
    assert abs(loss - np.float32(per).astype(np.float64).sum() / 3) < 1e-15
    assert np.array_equal(R.backward(D, 0.37, 3), D * (np.float32(0.37) / np.float32(3)))
    empty = R.batch(y, np.zeros_like(t))[1]
    assert np.array_equal(np.float32(empty), y.max(axis=1))         # G = 0: the largest probability


def test_negative_zero_is_zero_in_the_restatement():
    g = np.random.RandomState(2)
    y = np.array([-0.0, 0.0, 1.0, 0.5, -0.0], dtype=np.float32)[g.randint(0, 5, 60)]
    t = (g.rand(60) < 0.5).astype(np.float32)
    assert np.signbit(y[t == 0]).any()
    loss, D = R.image(y, t)
    loss_plus, D_plus = R.image(np.where(y == 0, np.float32(0.0), y), t)
    assert loss == loss_plus and np.array_equal(D.view(np.uint32), D_plus.view(np.uint32))


# ---- the C-ABI without a device
def test_workspace_formula():
    from punet import _lib
    ws = _lib.load().pu_lovasz_workspace_bytes
    for n in (1, 2, 1024, 10201, 16384):
        for batch in (1, 3, 32, 65535):
            assert ws(batch, n) == 8 * batch
    for bad in ((0, 8), (-1, 8), (65536, 8), (1, 0), (1, -5), (1, 16385), (4, 1 << 20)):
        assert ws(*bad) == 0, bad


def test_entries_reject_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the first launch."""
    from punet import _lib
    lib = _lib.load()
    B, n = 3, 1000
    nb = lib.pu_lovasz_workspace_bytes(B, n)

    def rejected(rc, entry, word, code=-1):
        assert rc == code, rc
        msg = lib.pu_last_error()
        assert msg.startswith(entry + b":") and word in msg, msg

    fwd, bwd = lib.pu_lovasz_fwd, lib.pu_lovasz_bwd
    F = b"pu_lovasz_fwd"
    rejected(fwd(None, A, B, n, A, A, A, A, nb, None), F, b"y is null")
    rejected(fwd(A, None, B, n, A, A, A, A, nb, None), F, b"t is null")
    rejected(fwd(A, A, B, n, None, A, A, A, nb, None), F, b"loss is null")
    rejected(fwd(A, A, B, n, A, A, A, None, nb, None), F, b"workspace is null")
    for bad in (0, -2, 65536):
        rejected(fwd(A, A, bad, n, A, A, A, A, 1 << 30, None), F, b"batch")
    for bad in (0, -1):
        rejected(fwd(A, A, B, bad, A, A, A, A, nb, None), F, b"pixels per image")
    for big in (16385, 65536, 512 * 512):
        rejected(fwd(A, A, B, big, A, A, A, A, 1 << 30, None), F, b"n %d pixels" % big, code=-2)     # unsupported
    for k in range(5):                                              # y, t, loss, loss_per_image, dtab off by two bytes
        ptrs = [A] * 5
        ptrs[k] = A + 2
        rejected(fwd(ptrs[0], ptrs[1], B, n, ptrs[2], ptrs[3], ptrs[4], A, nb, None), F, b"4-byte aligned")
    rejected(fwd(A, A, B, n, A, A, A, A + 4, nb, None), F, b"8-byte aligned")
    rejected(fwd(A, A, B, n, A, A, A, A, nb - 1, None), F, b"workspace", code=-4)
    rejected(fwd(A, A, B, n, A, A, A, A, 0, None), F, b"workspace", code=-4)
    # the optional outputs may be null: the next check is what fails
    rejected(fwd(A, A, B, n, A, None, None, A + 4, nb, None), F, b"8-byte aligned")
    W = b"pu_lovasz_bwd"
    rejected(bwd(None, A, B, n, A, None), W, b"dtab is null")
    rejected(bwd(A, A, B, n, None, None), W, b"dy is null")
    for bad in (0, -2, 65536):
        rejected(bwd(A, A, bad, n, A, None), W, b"batch")
    for bad in (0, -1):
        rejected(bwd(A, A, B, bad, A, None), W, b"pixels per image")
    rejected(bwd(A, A, B, 16385, A, None), W, b"n 16385 pixels", code=-2)
    for k in range(3):
        ptrs = [A] * 3
        ptrs[k] = A + 1
        rejected(bwd(ptrs[0], ptrs[1], B, n, ptrs[2], None), W, b"4-byte aligned")


# ---- the plumbing
def test_wrappers_are_exported_and_check_their_tensors():
    import punet
    from punet import kernels as K
    assert "lovasz_fwd" in K.__all__ and "lovasz_bwd" in K.__all__
    for name in ("LovaszLoss", "LovaszLossFunction", "lovasz_loss", "BCELoss", "bce_loss"):
        assert hasattr(punet, name)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.lovasz_fwd(torch.rand(2, 8), torch.rand(2, 8))
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        K.lovasz_bwd(torch.rand(2, 8), None)
    with pytest.raises(RuntimeError, match="must be on the ROCm device"):
        punet.lovasz_loss(torch.rand(2, 4, 4), torch.rand(2, 4, 4))
    with pytest.raises(ValueError, match="Target size"):
        punet.lovasz_loss(torch.rand(2, 4, 4), torch.rand(2, 4, 5))
    with pytest.raises(ValueError, match="batch axis"):
        punet.lovasz_loss(torch.rand(4), torch.rand(4))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2, 2))


def test_trainer_selects_its_loss():
    from punet import engine, head
    assert engine.Trainer(_Net()).loss_fn is head.bce_loss                    # the default: bce_loss itself
    assert engine.Trainer(_Net(), loss="bce", lovasz_weight=3.0).loss_fn is head.bce_loss
    assert engine.Trainer(_Net(), loss="lovasz").loss_fn is head.lovasz_loss
    both = engine.Trainer(_Net(), loss="bce+lovasz", lovasz_weight=0.5)
    assert both.loss_name == "bce+lovasz" and callable(both.loss_fn)
    for bad in ("nope", "", None, "BCE", "lovasz+bce"):
        with pytest.raises(ValueError, match="loss must be one of"):
            engine.Trainer(_Net(), loss=bad)


def test_composed_loss_is_bce_plus_w_lovasz(monkeypatch):
    from punet import engine
    monkeypatch.setattr(engine, "bce_loss", lambda y, t: (y * 2.0).sum())
    monkeypatch.setattr(engine, "lovasz_loss", lambda y, t: (y * t).sum())
    y, t = torch.tensor([1.0, 2.0], requires_grad=True), torch.tensor([3.0, 5.0])
    loss = engine.select_loss("bce+lovasz", 0.5)(y, t)
    assert float(loss.detach()) == 6.0 + 0.5 * 13.0
    loss.backward()
    assert y.grad.tolist() == [2.0 + 1.5, 2.0 + 2.5]


def test_train_cli_takes_the_loss_flags():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import inspect
    import train
    a = train.parse_args([])
    assert a.loss == "bce" and a.lovasz_weight == 1.0
    a = train.parse_args(["--loss", "bce+lovasz", "--lovasz-weight", "0.25"])
    assert a.loss == "bce+lovasz" and a.lovasz_weight == 0.25
    assert train.parse_args(["--loss", "lovasz"]).loss == "lovasz"
    with pytest.raises(SystemExit):
        train.parse_args(["--loss", "hinge"])
    sig = inspect.signature(train.start_train).parameters
    assert sig["loss"].default == "bce" and sig["lovasz_weight"].default == 1.0


# ---- the build
def test_kernel_set_of_the_build():
    """lovasz.hip holds the image kernel at its three LDS sizes, the finish and the backward, free of
    scratch and spills; the largest keeps 128 KiB of keys in LDS under the 160 KiB of a CU"""
    import build_native
    from wgrad_matrix import demangle
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    mine = [sym for sym, k in d["kernels"].items() if k["source"] == "lovasz.hip"]
    assert sorted(demangle(s) for s in mine) == ["lovasz_bwd_kernel", "lovasz_finish_kernel", "lovasz_image_kernel<1024>",
                                                 "lovasz_image_kernel<16384>", "lovasz_image_kernel<4096>"]
    for sym in mine:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (sym, k)
        assert k["vgpr"] + k.get("agpr", 0) <= 128, (sym, k)        # 1024 threads: 128 registers per thread
        if demangle(sym).startswith("lovasz_image_kernel<"):
            cap = int(demangle(sym)[len("lovasz_image_kernel<"):-1])
            assert 8 * cap <= k["lds"] <= 8 * cap + 512 and k["lds"] <= 160 * 1024, (sym, k)
    design = open(os.path.join(os.path.dirname(PKG), "DESIGN.md")).read()
    for name in ("lovasz_image_kernel", "lovasz_finish_kernel", "lovasz_bwd_kernel"):
        assert name in design
