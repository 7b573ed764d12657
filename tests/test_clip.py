"""CPU checks of gradient clipping by global norm (csrc/clip.hip, FusedAdam / Trainer max_grad_norm,
train.py --clip-grad): argument validation and the workspace formula of the C-ABI without a device,
the constructors, the default path (clipping off: the calls of before, nothing added), the command
line and the kernel sets of the build."""
import json
import sys

import pytest
import torch

from conftest import PKG

A = 0x10000          # 16-byte aligned stand-in pointer: validation never dereferences it

SIZE_LISTS = [(1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 5), (4096, 0, 5), tuple(range(1, 34)),
              tuple(7 + i % 5 for i in range(65)), (4097, 9), (), (0, 0)]


def _list(numels, grad=A):
    from punet import _lib
    arr = (_lib.AdamTensor * max(len(numels), 1))()
    for i, n in enumerate(numels):
        arr[i] = _lib.AdamTensor(None, grad if n else None, None, None, n)
    return arr


@pytest.mark.parametrize("numels", SIZE_LISTS, ids=[str(i) for i in range(len(SIZE_LISTS))])
def test_workspace_formula(numels):
    from punet import _lib
    lib = _lib.load()
    want = 8 * max(1, sum(-(-n // 4096) for n in numels))
    assert lib.pu_grad_norm_workspace_bytes(_list(numels), len(numels)) == want
    assert lib.pu_grad_norm_workspace_bytes(None, 0) == 8


def test_grad_norm_rejects_bad_arguments_without_a_device():
    """Every call below has exactly one bad argument and returns before the first launch."""
    from punet import _lib
    lib = _lib.load()
    numels = (4097, 9)
    good, nb = _list(numels), 8 * 3

    def rejected(rc, word):
        assert rc == -1
        msg = lib.pu_last_error()
        assert msg.startswith(b"pu_grad_norm") and word in msg, msg

    rejected(lib.pu_grad_norm(None, 2, 1.0, A, A, nb, None), b"list")
    rejected(lib.pu_grad_norm(good, -1, 1.0, A, A, nb, None), b"list")
    null_grad = _list(numels)
    null_grad[1].grad = None
    rejected(lib.pu_grad_norm(null_grad, 2, 1.0, A, A, nb, None), b"tensor 1")
    negative = _list(numels)
    negative[0].numel = -4
    rejected(lib.pu_grad_norm(negative, 2, 1.0, A, A, nb, None), b"tensor 0")
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        rejected(lib.pu_grad_norm(good, 2, bad, A, A, nb, None), b"max_norm")
    rejected(lib.pu_grad_norm(good, 2, 1.0, None, A, nb, None), b"out2")
    rejected(lib.pu_grad_norm(good, 2, 1.0, A, A, nb - 8, None), b"workspace")
    rejected(lib.pu_grad_norm(good, 2, 1.0, A, None, nb, None), b"workspace")
    # the whole list is checked before the first launch: a bad tensor in the second launch
    late = _list(tuple(range(1, 34)))
    late[32].grad = None
    rejected(lib.pu_grad_norm(late, 33, 1.0, A, A, 8 * 33, None), b"tensor 32")


def test_clipped_adam_rejects_bad_arguments_without_a_device():
    from punet import _lib
    lib = _lib.load()
    sc = (0.9, 0.999, 1e-8, 0.0, 1e-3, 1.0)
    full = (_lib.AdamTensor * 2)(_lib.AdamTensor(A, A, A, A, 10), _lib.AdamTensor(A, A, A, A, 3))
    assert lib.pu_adam_multi_clipped(full, 2, *sc, None, None) == -1
    assert b"grad_scale" in lib.pu_last_error()
    assert lib.pu_adam_multi_clipped(None, 2, *sc, A, None) == -1
    assert b"pu_adam_multi_clipped: bad tensor list" in lib.pu_last_error()
    full[1].exp_avg = None
    assert lib.pu_adam_multi_clipped(full, 2, *sc, A, None) == -1
    assert b"pu_adam_multi_clipped: tensor 1" in lib.pu_last_error()
    # the unclipped entry keeps its messages
    assert lib.pu_adam_multi(full, 2, *sc, None) == -1
    assert b"pu_adam_multi: tensor 1" in lib.pu_last_error()


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_constructors_reject_non_positive_max_grad_norm(bad):
    from punet import FusedAdam
    from punet.engine import Trainer
    from unet import UNetp
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([torch.zeros(3, requires_grad=True)], max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer(UNetp(1, 1, torch.device("cpu"), nbf=32, depth=3, base_ch=8), flat_grads=False, max_grad_norm=bad)


class _Recorder:
    def __init__(self, monkeypatch):
        from punet import kernels as K
        self.norm_calls, self.adam_calls = [], []
        monkeypatch.setattr(K, "grad_norm", self.grad_norm)
        monkeypatch.setattr(K, "adam_multi", self.adam_multi)

    def grad_norm(self, grads, max_norm):
        self.norm_calls.append((list(grads), max_norm))
        return torch.tensor([4.0, 0.25])

    def adam_multi(self, *args, **kw):
        self.adam_calls.append((args, kw))


def _two_groups():
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 7, 3, 2)]
    for p in ps[:3]:
        p.grad = torch.randn_like(p)
    return ps, [{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-2}]


def test_default_path_adds_no_call(monkeypatch):
    """max_grad_norm=None: kernels.grad_norm is never called and every adam_multi call has the ten
    positional arguments of before, no keyword."""
    from punet import FusedAdam
    rec = _Recorder(monkeypatch)
    ps, groups = _two_groups()
    opt = FusedAdam(groups, lr=1e-3)
    opt.step()
    opt.step()
    assert rec.norm_calls == []
    assert len(rec.adam_calls) == 4
    for args, kw in rec.adam_calls:
        assert len(args) == 10 and kw == {}
    assert opt.grad_norm is None and opt.clip_coef is None and opt.max_grad_norm is None


def test_clipping_takes_one_norm_over_all_groups_before_any_update(monkeypatch):
    from punet import FusedAdam
    rec = _Recorder(monkeypatch)
    ps, groups = _two_groups()
    order = []
    rec_norm, rec_adam = rec.grad_norm, rec.adam_multi
    from punet import kernels as K
    monkeypatch.setattr(K, "grad_norm", lambda *a: (order.append("norm"), rec_norm(*a))[1])
    monkeypatch.setattr(K, "adam_multi", lambda *a, **k: (order.append("adam"), rec_adam(*a, **k))[1])
    opt = FusedAdam(groups, lr=1e-3, max_grad_norm=2.0)
    opt.step()
    assert order == ["norm", "adam", "adam"]
    (grads, max_norm), = rec.norm_calls
    assert max_norm == 2.0
    # the parameter without a gradient is left out; the tensors are the ones Adam is handed
    assert [g.data_ptr() for g in grads] == [p.grad.data_ptr() for p in ps[:3]]
    handed = [g for args, _ in rec.adam_calls for g in args[1]]
    assert [g.data_ptr() for g in handed] == [g.data_ptr() for g in grads]
    for args, kw in rec.adam_calls:
        assert len(args) == 10 and list(kw) == ["grad_scale"]
        assert kw["grad_scale"].numel() == 1 and kw["grad_scale"].item() == 0.25
    assert opt.grad_norm.dim() == 0 and opt.grad_norm.item() == 4.0 and opt.clip_coef.item() == 0.25
    for p in ps[:3]:
        assert p.grad is not None           # left in place, unscaled


def test_trainer_threads_max_grad_norm_to_the_optimiser():
    from punet.engine import Trainer
    from unet import UNetp
    net = UNetp(1, 1, torch.device("cpu"), nbf=32, depth=3, base_ch=8)
    off = Trainer(net, flat_grads=False)
    assert off.opt.max_grad_norm is None and off.last_grad_norm is None
    on = Trainer(net, flat_grads=False, max_grad_norm=0.5)
    assert on.opt.max_grad_norm == 0.5 and on.last_grad_norm is None     # no step yet


def test_train_cli_clip_grad():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train
    assert train.parse_args(["-o", "x"]).clip_grad == 0.0
    assert train.parse_args(["-o", "x", "--clip-grad", "0.5"]).clip_grad == 0.5
    import inspect
    assert inspect.signature(train.start_train).parameters["clip_grad"].default == 0.0


def test_kernel_sets_of_the_build():
    """clip.hip holds exactly the three new kernels; adam.hip still holds exactly adam_kernel."""
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    by_source = {}
    for sym, k in d["kernels"].items():
        by_source.setdefault(k["source"], []).append(sym)

    def names(source):
        return sorted(n for s in by_source.get(source, []) for n in
                      ("adam_kernel", "adam_clip_kernel", "grad_sumsq_kernel", "grad_norm_finish_kernel")
                      if ("2pu%d%sE" % (len(n), n)) in s)

    assert len(by_source.get("clip.hip", [])) == 3
    assert names("clip.hip") == ["adam_clip_kernel", "grad_norm_finish_kernel", "grad_sumsq_kernel"]
    assert len(by_source.get("adam.hip", [])) == 1 and names("adam.hip") == ["adam_kernel"]
    for sym in by_source["clip.hip"]:
        k = d["kernels"][sym]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (sym, k)
