"""Input validation of UNetp, UNetpRes and CoordConvUNetp: one bad input at a time on CPU models,
exception type and message pinned to tests/golden/model_input_errors.json (recorded before the
three forwards were given one shared set of checks).

Every case runs twice.  "cpu": as a caller on a CPU device sees it - the device check of x / hebb
is then often the one that fires, and that is the pinned result.  "dev": with that device check
switched off, so the shape checks behind it are reached and their order is pinned too.  No case
gets past the checks: nothing is launched.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN

N = 32
MODELS = {
    "unetp": ("UNetp", dict(depth=3, base_ch=8, nbf=N)),
    "res": ("UNetpRes", dict(neurons=4, nbf=N)),
    "coord": ("CoordConvUNetp", dict(depth=3, base_ch=8, nbf=N)),
}
# bad input -> (constructor overrides, x shape, hebb shape, attributes set after construction)
BAD = {
    "batch_with_2d_hebb": ({}, (2, 1, N, N), (N, N), {}),
    "channels": ({}, (1, 3, N, N), (N, N), {}),
    "not_square": ({}, (1, 1, N // 2, 2 * N), (N, N), {}),
    "wrong_nbf": ({}, (1, 1, 2 * N, 2 * N), (N, N), {}),
    "hebb_shape": ({}, (2, 1, N, N), (3, N, N), {}),
    "hebb_side": ({}, (1, 1, N, N), (N, N + 1), {}),
    "rule": ({}, (1, 1, N, N), (N, N), {"rule": "bcm"}),
    "alfa_type": ({}, (1, 1, N, N), (N, N), {"alfa_type": "tied"}),
    "n_classes": ({}, (1, 1, N, N), (N, N), {"n_classes": 2}),
    # a side the model cannot pool: not divisible by 2^(depth-1) (UNetp, Coord), below 16 (Res)
    "side": ({"unetp": dict(depth=3, nbf=6), "coord": dict(depth=3, nbf=6), "res": dict(nbf=8)}, None, None, {}),
    "sequential_3d_hebb": ({"unetp": dict(hebb_mode="sequential"), "res": dict(hebb_mode="sequential")},
                           (2, 1, N, N), (2, N, N), {}),
    # two at once: the order of the checks
    "rule_and_channels": ({}, (1, 3, N, N), (N, N), {"rule": "bcm"}),
    "n_classes_and_side": ({"unetp": dict(depth=3, nbf=6), "coord": dict(depth=3, nbf=6), "res": dict(nbf=8)},
                           None, None, {"n_classes": 2}),
    "channels_and_hebb_shape": ({}, (2, 3, N, N), (3, N, N), {}),
}


def case_ids():
    ids = []
    for bad, (over, _, _, _) in BAD.items():
        for model in MODELS:
            if over and model not in over:
                continue                      # CoordConvUNetp has no sequential mode
            ids += ["%s-%s-%s" % (model, bad, mode) for mode in ("cpu", "dev")]
    return ids


def raised(case_id):
    """[exception type name, message] of model(x, hebb) for the case."""
    import unet
    model, bad, mode = case_id.split("-")
    cls, kw = MODELS[model]
    over, xs, hs, attrs = BAD[bad]
    kw = dict(kw, **over.get(model, {}))
    n = kw["nbf"]
    net = getattr(unet, cls)(1, 1, torch.device("cpu"), **kw)
    for k, v in attrs.items():
        setattr(net, k, v)
    x = torch.zeros(xs or (1, 1, n, n))
    hebb = torch.zeros(hs or (n, n))
    mp = pytest.MonkeyPatch()
    if mode == "dev":
        import importlib
        for mod in ("unet._plastic", "unet.unet_p", "unet.coord_conv"):
            try:
                m = importlib.import_module(mod)
            except ImportError:
                continue
            mp.setattr(m, "_check_gpu_tensor", lambda t, what: None, raising=False)
    try:
        net(x, hebb)
    except Exception as e:          # noqa: BLE001 - the type is what is pinned
        return [type(e).__name__, str(e)]
    finally:
        mp.undo()
    return ["no exception", ""]


@pytest.mark.parametrize("case_id", case_ids())
def test_bad_input_raises_the_pinned_exception(case_id):
    with open(os.path.join(GOLDEN, "model_input_errors.json")) as f:
        want = json.load(f)[case_id]
    assert want[0] != "no exception"
    assert raised(case_id) == want
