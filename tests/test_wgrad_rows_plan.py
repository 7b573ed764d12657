"""CPU checks of the weight-gradient plan around the column form of the Winograd-domain kernel
(csrc/wgrad.hip plan_wino): planning queries only, with stand-in pointers that nothing dereferences.

1. C2: the plan of every 3x3 weight-gradient call of UNetp(depth 5, base 64) on 128 x 128 images at
   batch 32.  The eleven layers whose channel counts are multiples of 128 take the plan of one
   position column per block (kind 5, reported tile 128 x 384, splits = 4 pages per tile split, each
   tile split the same tile range as in the 64 x 64 plan); the others keep theirs.
2. The 128-multiple shapes under the gate that other tests pin keep the 64 x 64 plan.
3. The column kernel keeps its register budget: no scratch, no spills, vgpr + agpr <= 256 (one
   512-thread block per CU).
"""
import ctypes
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))

from punet import _lib  # noqa: E402

A = 0x10000          # 16-byte aligned stand-in device pointer


def query(B, H, W, c0, c1, n, bias_mode=1):
    """(bn, bk, kind, splits, workspace bytes) of the fp32 (6-product) 3x3 same-size weight gradient."""
    L = _lib.load()
    a = _lib.WgradArgs(B, H, W, H, W, 3, 3, 1, 1, A, n, A, c0, A if c1 else None, c1, bias_mode, A,
                       A if bias_mode else None, 0, 1)
    v = [ctypes.c_int() for _ in range(4)]
    assert L.pu_wgrad_tile(ctypes.byref(a), *(ctypes.byref(x) for x in v)) == 0
    return tuple(x.value for x in v) + (L.pu_wgrad_workspace_bytes(ctypes.byref(a)),)


def col_plan(B, H, W, c0, c1, n, bias_mode=1):
    """The column plan's values from its rule: gx x gy channel blocks of 128, 256 / (4 gx gy) tile
    splits of whole 16-tile stages (the 64 x 64 plan's splits), 4 pages of [n][3 C (+ 1)] per tile split."""
    C = c0 + c1
    tiles = B * (H // 2) * (W // 2)
    stages = -(-tiles // 16)
    zs = max(1, min(stages, 256 // (4 * (C // 128) * (n // 128))))
    tps = -(-stages // zs) * 16
    splits = 4 * -(-tiles // tps)
    kcp = (3 * C + (bias_mode == 1) + 3) // 4 * 4
    total = n * kcp
    ws = (4 * splits * total + 255) // 256 * 256      # the slab alone: the finisher keeps no partials
    return 128, 384, 5, splits, ws


# ((B, H, W, c0, c1, n), (bn, bk, kind, splits, workspace bytes)) in the order of the backward pass
C2 = [
    ((32, 128, 128, 64, 0, 64), (64, 576, 5, 256, 40386560)),        # outermost up stage, second conv
    ((32, 128, 128, 64, 64, 64), (64, 576, 5, 128, 40247296)),
    ((32, 64, 64, 64, 0, 64), (64, 576, 5, 256, 40386560)),
    ((32, 64, 64, 128, 128, 64), (64, 576, 5, 64, 40177664)),
    ((32, 32, 32, 128, 0, 128), (128, 384, 5, 256, 50855936)),
    ((32, 32, 32, 256, 256, 128), (128, 384, 5, 64, 50462720)),
    ((32, 16, 16, 256, 0, 256), (128, 384, 5, 64, 50593792)),
    ((32, 16, 16, 512, 512, 256), (128, 384, 5, 16, 50397184)),
    ((32, 8, 8, 512, 0, 512), (128, 384, 5, 16, 50462720)),          # bottom, both convs
    ((32, 8, 8, 512, 0, 512), (128, 384, 5, 16, 50462720)),
    ((32, 16, 16, 512, 0, 512), (128, 384, 5, 16, 50462720)),
    ((32, 16, 16, 256, 0, 512), (128, 384, 5, 32, 50593792)),
    ((32, 32, 32, 256, 0, 256), (128, 384, 5, 64, 50593792)),
    ((32, 32, 32, 128, 0, 256), (128, 384, 5, 128, 50855936)),
    ((32, 64, 64, 128, 0, 128), (128, 384, 5, 256, 50855936)),
    ((32, 64, 64, 64, 0, 128), (64, 576, 5, 128, 40386560)),
    ((32, 128, 128, 64, 0, 64), (64, 576, 5, 256, 40386560)),
]


@pytest.mark.parametrize("shape,want", C2)
def test_c2_plans(shape, want):
    assert query(*shape) == want
    if want[0] == 128:
        assert want == col_plan(*shape)


def test_c2_stem_is_not_a_winograd_plan():
    assert query(32, 128, 128, 1, 0, 64)[2] == 4


def test_c2_has_eleven_column_layers():
    assert sum(1 for _, w in C2 if w[:2] == (128, 384)) == 11


# 128-multiple shapes of 64 - 224 tiles whose plan tests/test_wgrad_reduce_gpu.py (t_slab_6,
# q_view_slab_14) and tests/test_wino_gpu.py (WGRAD_CASES) pin or rely on
@pytest.mark.parametrize("shape,want", [
    ((3, 8, 16, 128, 0, 256), (64, 576, 5, 6, 7102464)),
    ((7, 8, 16, 128, 0, 256), (64, 576, 5, 14, 16572416)),
    ((3, 10, 14, 128, 0, 128), (64, 576, 5, 7, 4143104)),
    ((4, 8, 8, 512, 0, 512), (64, 576, 5, 4, 37781504)),
    ((2, 16, 16, 256, 256, 256), (64, 576, 5, 8, 37781504)),
])
def test_small_128_multiple_shapes_keep_the_64x64_plan(shape, want):
    assert query(*shape) == want


def test_gate_is_512_tiles_and_whole_128_channel_blocks():
    assert query(2, 32, 32, 128, 0, 128)[:3] == (128, 384, 5)        # 512 tiles
    assert query(2, 32, 30, 128, 0, 128)[:3] == (64, 576, 5)         # 480 tiles
    assert query(2, 32, 32, 128, 0, 192)[:3] == (64, 576, 5)
    assert query(2, 32, 32, 128, 64, 128)[:3] == (64, 576, 5)
    assert query(2, 32, 32, 64, 64, 128)[:3] == (64, 576, 5)
    for bias_mode in (0, 1):
        assert query(2, 32, 32, 128, 128, 128, bias_mode) == col_plan(2, 32, 32, 128, 128, 128, bias_mode)
        assert query(2, 32, 32, 512, 0, 256, bias_mode) == col_plan(2, 32, 32, 512, 0, 256, bias_mode)


def test_pmc_tag_of_the_column_kernel_is_the_bench_tag():
    """tools/pmc_traffic.py keys the column kernel by the tag kernels.py builds from pu_wgrad_tile."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(ROOT, "tools", "pmc_traffic.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    bn, bk, kind = query(32, 32, 32, 256, 0, 256)[:3]
    tag = "wgrad<%dx%d,%s,x6>" % (bn, bk, ("scalar", "vec4", "direct", "halo", "stem", "wino", "pointwise")[kind])
    assert m.tag_of("pu::wgrad_wino_cols_x6_kernel(pu::WinoWgradParams)") == tag == "wgrad<128x384,wino,x6>"
    assert m.tag_of("pu::wgrad_wino_x6_kernel(pu::WinoWgradParams)") == "wgrad<64x576,wino,x6>"


def test_column_kernel_register_budget():
    import build_native
    build_native.build(verbose=False)       # no-op when the objects are current
    d = json.load(open(build_native.RESOURCES))
    assert d["build_id"] == build_native.source_hash()
    rows = {n: v for n, v in d["kernels"].items() if "wgrad_wino_cols_x6_kernel" in n}
    assert rows, "wgrad_wino_cols_x6_kernel is not in the resource report"
    for n, v in rows.items():
        assert not v.get("scratch", 0) and not v.get("vgpr_spill", 0) and not v.get("sgpr_spill", 0), (n, v)
        assert v["vgpr"] + v["agpr"] <= 256, (n, v)
        assert v["occupancy"] >= 2, (n, v)
