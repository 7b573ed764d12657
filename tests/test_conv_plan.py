"""CPU checks of the convolution dispatch plans (csrc/igemm.hip plan_conv, csrc/igemm_bf16.hip
plan_conv_b): planning queries only, with stand-in pointers that nothing dereferences.

1. PINNED: the plan of every kind of both ladders, recorded from the library before the three entry
   points of each file were rebuilt on one plan struct - the dispatch must reproduce it exactly.
2. The tile query and the workspace query agree with each other over the trunks' layer shapes.
3. PU_CONV_HALO_DMA / PU_CONV_HALO_V1 select nothing; the Python switch is on / off.
"""
import ctypes

import pytest

from punet import _lib

A = 0x10000          # 16-byte aligned stand-in device pointer
WS = 0x20000         # stand-in scratch
RELU, SHUF, NO_HALO, HALO_V1, NO_SMALLX6, HALO_DMA = 1, 4, 16, 32, 64, 128


def conv(B, H, c0, c1, n, k=3, stride=1, pad=1, cg=0, flags=RELU, w6=False, wino=False, W=None, out=None, n0=None,
         kp=None, kpm=16):
    """ConvArgs of a kxk convolution of B x H x W x (c0 + c1) into n channels; out: the output grid
    when it differs from the input's; kp: weight row stride (default: K rounded up to kpm)."""
    W = H if W is None else W
    oh, ow = (H, W) if out is None else out
    K = k * k * (c0 + c1)
    a = _lib.ConvArgs(B, H, W, oh, ow, k, k, stride, pad, A, c0, A if c1 else None, c1, A,
                      (K + kpm - 1) // kpm * kpm if kp is None else kp, cg, n, A, A, n if n0 is None else n0,
                      A if (n0 is not None and n0 != n) else None, None, None, flags, None, 0)
    a.weight6 = A if w6 else None
    a.wino = A if wino else None
    return a


def query(entry, a, scratch):
    """(rc, bm, bn, mode | kind, ksplit, workspace_bytes) of ConvArgs a; scratch: None, or the
    difference between the scratch passed to the tile query and what the workspace query asks for."""
    L = _lib.load()
    ws_fn, tile_fn = ((L.pu_conv_igemm_workspace_bytes, L.pu_conv_igemm_tile) if entry == "f32" else
                      (L.pu_conv_igemm_bf16_workspace_bytes, L.pu_conv_igemm_bf16_tile))
    a.workspace, a.ws_bytes = None, 0
    need = ws_fn(ctypes.byref(a))
    if scratch is not None:
        a.workspace, a.ws_bytes = WS, max(0, need + scratch)
    bm, bn, x, y = (ctypes.c_int(0) for _ in range(4))
    rc = tile_fn(ctypes.byref(a), *(ctypes.byref(v) for v in (bm, bn, x, y)))
    mode, ks = (x.value, y.value) if entry == "f32" else (y.value, x.value)   # f32: (mode, ksplit); bf16: (ksplit, kind)
    return rc, bm.value, bn.value, mode, ks, need


X6 = dict(w6=True)
WINO = dict(w6=True, wino=True)
CONVT = dict(k=2, pad=1, flags=RELU | SHUF)      # the ConvT 2x2/s2 forward as a 2x2 sub-pixel conv

# (entry, what, conv() positional arguments, conv() keyword arguments, scratch given to the tile query)
CASES = [
    # ---- fp32 ladder
    ("f32", "stem n8", (2, 64, 1, 0, 8), {}, False),
    ("f32", "stem n16", (2, 64, 1, 0, 16), {}, False),
    ("f32", "stem n32", (2, 64, 1, 0, 32), {}, False),
    ("f32", "stem n64", (2, 100, 1, 0, 64), dict(W=72), False),
    ("f32", "1x1 small 4->8", (2, 64, 4, 0, 8), dict(k=1, pad=0), False),
    ("f32", "1x1 small 4+4->16", (2, 24, 4, 4, 16), dict(k=1, pad=0, W=40), False),
    ("f32", "smallx6 8->8", (4, 64, 8, 0, 8), X6, False),
    ("f32", "smallx6 8+8->16", (4, 64, 8, 8, 16), X6, False),
    ("f32", "smallx6 stride 2", (4, 64, 8, 0, 16), dict(w6=True, stride=2, out=(32, 32)), False),
    ("f32", "smallx6 ConvT 16->4x8", (4, 32, 16, 0, 32), dict(w6=True, out=(33, 33), kp=64, **CONVT), False),
    ("f32", "direct 8->8 (no weight6)", (4, 64, 8, 0, 8), {}, False),
    ("f32", "direct 16->16 (NO_SMALLX6)", (4, 64, 16, 0, 16), dict(w6=True, flags=RELU | NO_SMALLX6), False),
    ("f32", "direct 12->8", (4, 64, 12, 0, 8), {}, False),
    ("f32", "direct 4->4", (1, 24, 4, 0, 4), dict(W=40), False),
    ("f32", "wino narrow", (32, 128, 64, 0, 64), dict(cg=32, **WINO), False),
    ("f32", "wino narrow two sources", (8, 64, 64, 64, 64), dict(cg=16, **WINO), True),
    ("f32", "wino wide 64->128", (32, 64, 64, 0, 128), dict(cg=32, **WINO), False),
    ("f32", "wino wide split column", (4, 64, 32, 32, 256), dict(cg=32, n0=96, **WINO), True),
    ("f32", "wino 8x8 split, no scratch", (32, 8, 512, 0, 512), dict(cg=32, **WINO), False),
    ("f32", "wino 8x8 split", (32, 8, 512, 0, 512), dict(cg=32, **WINO), True),
    ("f32", "wino 8x8 split two sources", (32, 8, 512, 512, 512), dict(cg=32, **WINO), True),
    ("f32", "wino 16x16 split", (8, 16, 256, 0, 256), dict(cg=16, **WINO), True),
    ("f32", "x6 lean 256x128", (32, 32, 256, 0, 256), dict(cg=32, **X6), True),
    ("f32", "x6 lean 256x128 split, no scratch", (32, 8, 512, 0, 512), dict(cg=32, **X6), False),
    ("f32", "x6 lean 256x128 split", (32, 8, 512, 0, 512), dict(cg=32, **X6), True),
    ("f32", "x6 lean 256x128 split cgroup 16", (32, 16, 256, 256, 256), dict(cg=16, **X6), True),
    ("f32", "x6 lean 256x64", (32, 128, 64, 0, 64), dict(cg=32, **X6), False),
    ("f32", "x6 lean 256x64 cgroup 16", (32, 128, 64, 64, 64), dict(cg=16, **X6), True),
    ("f32", "x6 lean 128x128", (32, 64, 64, 0, 128), dict(cg=32, **X6), False),
    ("f32", "x6 lean 128x128 split, no scratch", (4, 16, 128, 0, 192), dict(cg=16, **X6), False),
    ("f32", "x6 lean 128x128 split", (4, 16, 128, 0, 192), dict(cg=16, **X6), True),
    ("f32", "x6 lean 128x64", (4, 128, 64, 0, 64), dict(cg=32, **X6), True),
    ("f32", "x6 lean 128x64 split in two", (2, 64, 64, 0, 64), dict(cg=32, **X6), True),
    ("f32", "x6 lean 128x64 split", (2, 16, 128, 128, 64), dict(cg=32, **X6), True),
    ("f32", "x6 lean 128x64 split, no scratch", (2, 16, 128, 128, 64), dict(cg=32, **X6), False),
    ("f32", "x6 lean 256x32", (32, 256, 32, 0, 32), dict(cg=32, **X6), False),
    ("f32", "x6 lean 256x32 cgroup 16", (32, 256, 16, 16, 32), dict(cg=16, **X6), True),
    ("f32", "x6 lean 128x32", (4, 128, 32, 0, 32), dict(cg=32, **X6), False),
    ("f32", "x6 lean 128x32 split in two", (2, 64, 32, 0, 32), dict(cg=16, **X6), True),
    ("f32", "x6 lean 128x32 split", (1, 16, 64, 0, 32), dict(cg=32, **X6), True),
    ("f32", "x6 lean 128x32 split, no scratch", (1, 16, 64, 0, 32), dict(cg=32, **X6), False),
    ("f32", "x6 lean stride 2", (8, 64, 64, 0, 128), dict(cg=32, stride=2, out=(32, 32), **X6), True),
    ("f32", "x6 cgroup 0", (32, 128, 64, 0, 64), X6, False),
    ("f32", "x6 cgroup 0 256x128 split", (32, 8, 512, 0, 512), X6, True),
    ("f32", "x6 cgroup 0 256x128 split, no scratch", (32, 8, 512, 0, 512), X6, False),
    ("f32", "x6 c1 != c0", (8, 32, 128, 64, 128), dict(cg=32, **X6), True),
    ("f32", "x6 32 channels into 64 (tile 128x64)", (2, 32, 32, 0, 64), X6, True),
    ("f32", "x6 1x1", (32, 64, 64, 0, 64), dict(k=1, pad=0, **X6), False),
    ("f32", "x6 1x1 split", (32, 8, 512, 0, 256), dict(k=1, pad=0, **X6), True),
    ("f32", "x6 ConvT 128->4x64", (32, 32, 128, 0, 256), dict(w6=True, out=(33, 33), **CONVT), False),
    ("f32", "x6 ConvT 512->4x256 split", (8, 8, 512, 0, 1024), dict(w6=True, out=(9, 9), **CONVT), True),
    ("f32", "dma 256x64", (32, 128, 64, 0, 64), {}, False),
    ("f32", "dma 128x64 split in two, no scratch", (4, 128, 64, 0, 64), dict(cg=32), False),
    ("f32", "dma 128x128", (32, 64, 64, 64, 128), dict(cg=16), False),
    ("f32", "dma 128x64 for n 128, split in two", (32, 32, 128, 0, 128), {}, True),
    ("f32", "dma 64x64 split, no scratch", (32, 8, 512, 0, 512), {}, False),
    ("f32", "dma 64x64 split", (32, 8, 512, 0, 512), {}, True),
    ("f32", "dma 64x64 split two sources", (2, 24, 64, 64, 64), dict(cg=32, W=40), True),
    ("f32", "dma ConvT", (4, 16, 128, 0, 256), dict(out=(17, 17), **CONVT), True),
    ("f32", "vec4 loader", (8, 64, 20, 0, 32), {}, True),
    ("f32", "vec4 loader 128x128", (32, 64, 36, 0, 128), {}, False),
    ("f32", "scalar loader", (8, 64, 3, 0, 32), {}, True),
    ("f32", "scalar loader 64x64", (1, 24, 5, 2, 64), dict(W=40), False),
    # ---- bf16 ladder
    ("bf16", "rows", (4, 128, 64, 0, 64), dict(cg=32, kpm=32), False),
    ("bf16", "rows dgrad form", (32, 128, 64, 0, 64), dict(cg=32, kpm=32, flags=0), True),
    ("bf16", "halo W 128 two sources", (2, 128, 32, 32, 64), dict(cg=32, kpm=32), False),
    ("bf16", "halo W 128 n 128", (2, 128, 128, 0, 128), dict(cg=32, kpm=32), True),
    ("bf16", "halo W 128, 8 rows (not a rows strip)", (3, 8, 64, 0, 64), dict(cg=32, kpm=32, W=128), True),
    ("bf16", "halo W 64", (8, 64, 128, 0, 64), dict(cg=32, kpm=32), False),
    ("bf16", "halo W 64 two sources", (4, 64, 64, 64, 192), dict(cg=32, kpm=32, n0=64), True),
    ("bf16", "halo W 32", (16, 32, 64, 0, 64), dict(cg=32, kpm=32), False),
    ("bf16", "halo W 32 two sources", (4, 32, 64, 64, 128), dict(cg=32, kpm=32), True),
    ("bf16", "halo W 32 unequal sources", (32, 32, 128, 64, 128), dict(cg=32, kpm=32), True),
    ("bf16", "NO_HALO: rows shape", (4, 128, 64, 0, 64), dict(cg=32, kpm=32, flags=RELU | NO_HALO), True),
    ("bf16", "NO_HALO: W 64", (8, 64, 128, 0, 64), dict(cg=32, kpm=32, flags=RELU | NO_HALO), True),
    ("bf16", "NO_HALO: W 32 two sources", (4, 32, 64, 64, 128), dict(cg=32, kpm=32, flags=RELU | NO_HALO), True),
    ("bf16", "NO_HALO: W 32 two sources, no scratch", (4, 32, 64, 64, 128), dict(cg=32, kpm=32, flags=RELU | NO_HALO),
     False),
    ("bf16", "lean 256x128", (32, 64, 128, 0, 128), dict(cg=32, kpm=32, flags=RELU | NO_HALO), False),
    ("bf16", "lean 256x128 stride 2", (32, 128, 64, 0, 128), dict(cg=32, kpm=32, stride=2, out=(64, 64)), True),
    ("bf16", "lean 256x64", (32, 64, 64, 0, 64), dict(cg=32, kpm=32, flags=RELU | NO_HALO), False),
    ("bf16", "lean 256x64 odd grid", (32, 101, 64, 64, 64), dict(cg=32, kpm=32), True),
    ("bf16", "lean 256x64 split", (2, 16, 64, 0, 64), dict(cg=32, kpm=32), True),
    ("bf16", "lean 256x64 split, no scratch", (2, 16, 64, 0, 64), dict(cg=32, kpm=32), False),
    ("bf16", "lean 128x128 unsplit (t128 256)", (32, 16, 512, 0, 512), dict(cg=32, kpm=32), True),
    ("bf16", "lean 128x128 unsplit (t128 240)", (30, 16, 256, 256, 512), dict(cg=32, kpm=32), False),
    ("bf16", "lean 128x128 split 8x8", (32, 8, 512, 0, 512), dict(cg=32, kpm=32), True),
    ("bf16", "lean 128x128 split 8x8, no scratch", (32, 8, 512, 0, 512), dict(cg=32, kpm=32), False),
    ("bf16", "lean 128x128 split 8x8 two sources", (32, 8, 512, 512, 512), dict(cg=32, kpm=32), True),
    ("bf16", "lean 128x128 split 16x16", (32, 16, 256, 0, 256), dict(cg=32, kpm=32), True),
    ("bf16", "lean 128x128 split 16x16, no scratch", (32, 16, 256, 0, 256), dict(cg=32, kpm=32), False),
    ("bf16", "lean 128x128 short K (k2 < 2)", (8, 16, 32, 0, 128), dict(cg=32, kpm=32), True),
    ("bf16", "generic 256x64", (32, 128, 64, 0, 64), dict(kpm=32), False),
    ("bf16", "generic 128x128", (32, 64, 128, 0, 128), dict(kpm=32), True),
    ("bf16", "generic 128x64 split in two, no scratch", (4, 128, 64, 0, 64), dict(kpm=32), False),
    ("bf16", "generic 128x64 for n 128, split in two", (32, 32, 128, 0, 128), dict(kpm=32), True),
    ("bf16", "generic unequal sources (not lean)", (32, 16, 128, 64, 128), dict(cg=32, kpm=32), True),
    ("bf16", "generic 64x64 split", (32, 8, 512, 0, 512), dict(kpm=32), True),
    ("bf16", "generic 64x64 split, no scratch", (32, 8, 512, 0, 512), dict(kpm=32), False),
    ("bf16", "generic 1x1", (32, 64, 64, 0, 64), dict(k=1, pad=0, kpm=32), False),
    ("bf16", "generic 1x1 split", (4, 16, 512, 0, 64), dict(k=1, pad=0, cg=32, kpm=32), True),
    ("bf16", "SHUFFLE2 ConvT 128->4x64", (32, 32, 128, 0, 256), dict(out=(33, 33), kpm=32, **CONVT), False),
    ("bf16", "SHUFFLE2 ConvT 3x3-shaped (cgroup 32: not lean)", (8, 16, 64, 0, 256),
     dict(cg=32, kpm=32, flags=RELU | SHUF), True),
    ("bf16", "SHUFFLE2 ConvT 512->4x256 split", (8, 8, 512, 0, 1024), dict(out=(9, 9), kpm=32, **CONVT), True),
    ("bf16", "refused: 48 channels", (4, 64, 48, 0, 64), dict(kpm=32), False),
]

# (rc, bm, bn, mode | kind, ksplit, workspace_bytes) of each case, in order
PINNED = [
    (0, 1024, 8, 5, 1, 0),                     # f32: stem n8
    (0, 1024, 16, 5, 1, 0),                    # f32: stem n16
    (0, 1024, 32, 5, 1, 0),                    # f32: stem n32
    (0, 1024, 64, 5, 1, 0),                    # f32: stem n64
    (0, 256, 8, 3, 1, 0),                      # f32: 1x1 small 4->8
    (0, 256, 16, 3, 1, 0),                     # f32: 1x1 small 4+4->16
    (0, 512, 8, 7, 1, 0),                      # f32: smallx6 8->8
    (0, 512, 16, 7, 1, 0),                     # f32: smallx6 8+8->16
    (0, 128, 16, 7, 1, 0),                     # f32: smallx6 stride 2
    (0, 256, 32, 7, 1, 0),                     # f32: smallx6 ConvT 16->4x8
    (0, 512, 8, 3, 1, 0),                      # f32: direct 8->8 (no weight6)
    (0, 512, 16, 3, 1, 0),                     # f32: direct 16->16 (NO_SMALLX6)
    (0, 512, 8, 3, 1, 0),                      # f32: direct 12->8
    (0, 512, 4, 3, 1, 0),                      # f32: direct 4->4
    (0, 256, 64, 6, 1, 0),                     # f32: wino narrow
    (0, 256, 64, 6, 1, 0),                     # f32: wino narrow two sources
    (0, 128, 128, 6, 1, 0),                    # f32: wino wide 64->128
    (0, 128, 128, 6, 1, 0),                    # f32: wino wide split column
    (0, 256, 64, 6, 1, 16777216),              # f32: wino 8x8 split, no scratch
    (0, 256, 64, 6, 4, 16777216),              # f32: wino 8x8 split
    (0, 256, 64, 6, 4, 16777216),              # f32: wino 8x8 split two sources
    (0, 256, 64, 6, 2, 4194304),               # f32: wino 16x16 split
    (0, 256, 128, 4, 1, 0),                    # f32: x6 lean 256x128
    (0, 256, 128, 4, 1, 33554432),             # f32: x6 lean 256x128 split, no scratch
    (0, 256, 128, 4, 8, 33554432),             # f32: x6 lean 256x128 split
    (0, 256, 128, 4, 4, 33554432),             # f32: x6 lean 256x128 split cgroup 16
    (0, 256, 64, 4, 1, 0),                     # f32: x6 lean 256x64
    (0, 256, 64, 4, 1, 0),                     # f32: x6 lean 256x64 cgroup 16
    (0, 128, 128, 4, 1, 0),                    # f32: x6 lean 128x128
    (0, 128, 128, 4, 1, 6291456),              # f32: x6 lean 128x128 split, no scratch
    (0, 128, 128, 4, 8, 6291456),              # f32: x6 lean 128x128 split
    (0, 128, 64, 4, 1, 0),                     # f32: x6 lean 128x64
    (0, 128, 64, 4, 2, 4194304),               # f32: x6 lean 128x64 split in two
    (0, 128, 64, 4, 8, 1048576),               # f32: x6 lean 128x64 split
    (0, 128, 64, 4, 1, 1048576),               # f32: x6 lean 128x64 split, no scratch
    (0, 256, 32, 4, 1, 0),                     # f32: x6 lean 256x32
    (0, 256, 32, 4, 1, 0),                     # f32: x6 lean 256x32 cgroup 16
    (0, 128, 32, 4, 1, 0),                     # f32: x6 lean 128x32
    (0, 128, 32, 4, 2, 2097152),               # f32: x6 lean 128x32 split in two
    (0, 128, 32, 4, 2, 65536),                 # f32: x6 lean 128x32 split
    (0, 128, 32, 4, 1, 65536),                 # f32: x6 lean 128x32 split, no scratch
    (0, 128, 128, 4, 2, 8388608),              # f32: x6 lean stride 2
    (0, 256, 64, 4, 1, 0),                     # f32: x6 cgroup 0
    (0, 256, 128, 4, 8, 33554432),             # f32: x6 cgroup 0 256x128 split
    (0, 256, 128, 4, 1, 33554432),             # f32: x6 cgroup 0 256x128 split, no scratch
    (0, 128, 128, 4, 8, 33554432),             # f32: x6 c1 != c0
    (0, 128, 64, 4, 2, 1048576),               # f32: x6 32 channels into 64 (tile 128x64)
    (0, 256, 64, 4, 1, 0),                     # f32: x6 1x1
    (0, 128, 128, 4, 4, 8388608),              # f32: x6 1x1 split
    (0, 128, 128, 4, 1, 0),                    # f32: x6 ConvT 128->4x64
    (0, 256, 128, 4, 11, 29196288),            # f32: x6 ConvT 512->4x256 split
    (0, 256, 64, 0, 1, 0),                     # f32: dma 256x64
    (0, 128, 64, 0, 1, 33554432),              # f32: dma 128x64 split in two, no scratch
    (0, 128, 128, 0, 1, 0),                    # f32: dma 128x128
    (0, 128, 64, 0, 2, 33554432),              # f32: dma 128x64 for n 128, split in two
    (0, 64, 64, 0, 1, 16777216),               # f32: dma 64x64 split, no scratch
    (0, 64, 64, 0, 4, 16777216),               # f32: dma 64x64 split
    (0, 64, 64, 0, 9, 4423680),                # f32: dma 64x64 split two sources
    (0, 64, 64, 0, 4, 4734976),                # f32: dma ConvT
    (0, 64, 64, 1, 1, 0),                      # f32: vec4 loader
    (0, 128, 128, 1, 1, 0),                    # f32: vec4 loader 128x128
    (0, 64, 64, 2, 1, 0),                      # f32: scalar loader
    (0, 64, 64, 2, 1, 0),                      # f32: scalar loader 64x64
    (0, 128, 64, 3, 1, 0),                     # bf16: rows
    (0, 128, 64, 3, 1, 0),                     # bf16: rows dgrad form
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 128 two sources
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 128 n 128
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 128, 8 rows (not a rows strip)
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 64
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 64 two sources
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 32
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 32 two sources
    (0, 256, 64, 2, 1, 0),                     # bf16: halo W 32 unequal sources
    (0, 256, 64, 1, 2, 33554432),              # bf16: NO_HALO: rows shape
    (0, 256, 64, 1, 4, 33554432),              # bf16: NO_HALO: W 64
    (0, 128, 128, 1, 4, 8388608),              # bf16: NO_HALO: W 32 two sources
    (0, 128, 128, 1, 1, 8388608),              # bf16: NO_HALO: W 32 two sources, no scratch
    (0, 256, 128, 1, 1, 0),                    # bf16: lean 256x128
    (0, 256, 128, 1, 1, 0),                    # bf16: lean 256x128 stride 2
    (0, 256, 64, 1, 1, 0),                     # bf16: lean 256x64
    (0, 256, 64, 1, 1, 0),                     # bf16: lean 256x64 odd grid
    (0, 256, 64, 1, 2, 262144),                # bf16: lean 256x64 split
    (0, 256, 64, 1, 1, 262144),                # bf16: lean 256x64 split, no scratch
    (0, 128, 128, 1, 1, 0),                    # bf16: lean 128x128 unsplit (t128 256)
    (0, 128, 128, 1, 1, 0),                    # bf16: lean 128x128 unsplit (t128 240)
    (0, 128, 128, 1, 8, 33554432),             # bf16: lean 128x128 split 8x8
    (0, 128, 128, 1, 1, 33554432),             # bf16: lean 128x128 split 8x8, no scratch
    (0, 128, 128, 1, 8, 33554432),             # bf16: lean 128x128 split 8x8 two sources
    (0, 128, 128, 1, 4, 33554432),             # bf16: lean 128x128 split 16x16
    (0, 128, 128, 1, 1, 33554432),             # bf16: lean 128x128 split 16x16, no scratch
    (0, 128, 128, 1, 1, 0),                    # bf16: lean 128x128 short K (k2 < 2)
    (0, 256, 64, 0, 1, 0),                     # bf16: generic 256x64
    (0, 128, 128, 0, 1, 0),                    # bf16: generic 128x128
    (0, 128, 64, 0, 1, 33554432),              # bf16: generic 128x64 split in two, no scratch
    (0, 128, 64, 0, 2, 33554432),              # bf16: generic 128x64 for n 128, split in two
    (0, 64, 64, 0, 4, 16777216),               # bf16: generic unequal sources (not lean)
    (0, 64, 64, 0, 4, 16777216),               # bf16: generic 64x64 split
    (0, 64, 64, 0, 1, 16777216),               # bf16: generic 64x64 split, no scratch
    (0, 256, 64, 0, 1, 0),                     # bf16: generic 1x1
    (0, 64, 64, 0, 4, 1048576),                # bf16: generic 1x1 split
    (0, 128, 128, 0, 1, 0),                    # bf16: SHUFFLE2 ConvT 128->4x64
    (0, 64, 64, 0, 4, 8388608),                # bf16: SHUFFLE2 ConvT 3x3-shaped (cgroup 32: not lean)
    (0, 64, 64, 0, 5, 13271040),               # bf16: SHUFFLE2 ConvT 512->4x256 split
    (-1, 0, 0, 0, 0, 0),                       # bf16: refused: 48 channels
]


def test_pinned_table_covers_every_kind():
    assert len(PINNED) == len(CASES)
    f32 = {(p[3], p[4] > 1, p[5] > 0) for c, p in zip(CASES, PINNED) if c[0] == "f32"}
    assert {m for m, _, _ in f32} == set(range(8))                 # every reported fp32 mode
    for mode in (0, 4, 6):                                         # the split-K kinds, with and without scratch
        assert (mode, True, True) in f32 and (mode, False, True) in f32, mode
    b16 = {(p[3], p[4] > 1, p[5] > 0) for c, p in zip(CASES, PINNED) if c[0] == "bf16" and p[0] == 0}
    assert {k for k, _, _ in b16} == {0, 1, 2, 3}
    for kind in (0, 1):
        assert (kind, True, True) in b16 and (kind, False, True) in b16, kind


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] + ": " + c[1] for c in CASES])
def test_pinned_plan(i):
    entry, _, pos, kw, scratch = CASES[i]
    assert query(entry, conv(*pos, **kw), 0 if scratch else None) == PINNED[i]


def trunk_shapes():
    """the layer shapes tests/asan_abi_driver.py plans (C2/C3 base 64, C4 base 8 at 256, C5 n8 at 512)"""
    shapes = []
    for S, chans in ((128, [64, 128, 256, 512, 512]), (256, [8, 16, 32, 64, 128]), (512, [8, 16, 32, 64, 128])):
        for lvl, c in enumerate(chans):
            for B in (1, 2, 16, 32):
                h = S >> lvl
                shapes += [(B, h, c, 0, c), (B, h, c, c, c), (B, h, c, 0, 2 * c), (B, h, 2 * c, 0, c)]
    return shapes


def test_tile_and_workspace_queries_agree():
    checked = split = 0
    for entry, variants in (("f32", ({}, X6, WINO)), ("bf16", (dict(kpm=32),))):
        for B, H, c0, c1, n in trunk_shapes():
            for cg in ((0, 16, 32) if entry == "f32" else (0, 32)):
                if cg and (c0 % cg or c1 % cg):
                    continue
                for kw in variants:
                    def q(scratch):
                        return query(entry, conv(B, H, c0, c1, n, cg=cg, **kw), scratch)
                    rc, bm, bn, mode, ks, need = q(None)
                    if entry == "bf16" and c0 % 32:
                        assert rc == -1 and need == 0       # the bf16 queries validate (setup_bf16)
                        continue
                    assert rc == 0 and bm > 0 and bn > 0
                    assert ks == 1, "no scratch: unsplit"
                    rc, bm2, bn2, mode2, ks, need2 = q(0)
                    assert (rc, bm2, bn2, mode2, need2) == (0, bm, bn, mode, need)
                    assert ks * (B * H * H) * n * 4 == need if need else ks == 1
                    assert q(-1)[4] == 1, "scratch one byte short: unsplit"
                    checked += 1
                    split += ks > 1
    assert checked > 500 and split > 50


BF16_OK = [i for i, c in enumerate(CASES) if c[0] == "bf16"]


@pytest.mark.parametrize("flag", [HALO_DMA, HALO_V1, HALO_DMA | HALO_V1])
def test_retired_halo_flags_select_nothing(flag):
    for i in BF16_OK:
        _, _, pos, kw, scratch = CASES[i]
        kw = dict(kw, flags=kw.get("flags", RELU) | flag)
        assert query("bf16", conv(*pos, **kw), 0 if scratch else None) == PINNED[i], CASES[i][1]


def test_python_halo_switch_is_on_off():
    from punet import kernels as K
    prev = K.set_conv_halo(True)
    try:
        assert K._halo_flags() == 0
        assert K.set_conv_halo(0) == 1 and K._halo_flags() == NO_HALO
        assert K.set_conv_halo(1) == 0 and K._halo_flags() == 0
        assert K.set_conv_halo(False) == 1 and K._halo_flags() == NO_HALO
        for bad in (2, -1, "1", None):
            with pytest.raises(ValueError):
                K.set_conv_halo(bad)
        assert K._halo_flags() == NO_HALO            # a refused setting changes nothing
    finally:
        K.set_conv_halo(prev)
