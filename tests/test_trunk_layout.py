"""Order of trunk.params and trunk.backward_order() as state_dict names (CPU, no launches).

The flat gradient buffer, the data-parallel buckets and Adam's tensor list are laid out by these
two orders; tests/golden/trunk_layout.json holds them as recorded before the trunks were moved
onto their shared base.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN

CASES = {
    "unetp": ("UNetp", dict(depth=3, base_ch=8, nbf=32)),
    "unetp_bn": ("UNetp", dict(depth=3, base_ch=8, nbf=32, batch_norm=True)),
    "unetp_bilinear": ("UNetp", dict(depth=3, base_ch=8, nbf=32, bilinear_upsample=True)),
    "coord": ("CoordConvUNetp", dict(depth=2, base_ch=8, nbf=16)),       # smallest: one pooling level
    "res": ("UNetpRes", dict(neurons=4, nbf=16)),
    "res_bn": ("UNetpRes", dict(neurons=4, nbf=16, batch_norm=True)),
}


def layout(case):
    import unet
    cls, kw = CASES[case]
    torch.manual_seed(0)
    model = getattr(unet, cls)(1, 1, torch.device("cpu"), **kw)
    trunk = model._trunk_plan()
    name = {id(p): n for n, p in model.named_parameters()}
    return {"params": [name[id(p)] for p in trunk.params],
            "backward_order": [name[id(p)] for p in trunk.backward_order()]}


@pytest.mark.parametrize("case", sorted(CASES))
def test_trunk_parameter_and_backward_order(case):
    with open(os.path.join(GOLDEN, "trunk_layout.json")) as f:
        want = json.load(f)[case]
    got = layout(case)
    assert got["params"] == want["params"]
    assert got["backward_order"] == want["backward_order"]
    assert sorted(got["params"]) == sorted(got["backward_order"])       # the same set, each once
    assert len(set(got["params"])) == len(got["params"])


def test_trunks_share_the_layer_definitions():
    from punet import layers as L, trunk as T, res_trunk as R
    for name in ("conv3x3", "conv3x3_dgrad", "conv3x3_wgrad"):
        assert getattr(T, name) is getattr(L, name) and getattr(R, name) is getattr(L, name)
    for name in ("convT2x2", "convT2x2_dgrad", "convT2x2_wgrad", "as_nhwc_input"):
        assert getattr(T, name) is getattr(L, name)
    for name in ("convT3x3", "convT3x3_dgrad", "convT3x3_wgrad"):
        assert getattr(R, name) is getattr(L, name)
    assert not hasattr(R, "ResTrunkFunction")
    from punet.trunk_base import TrunkFunction
    assert T.TrunkFunction is TrunkFunction
