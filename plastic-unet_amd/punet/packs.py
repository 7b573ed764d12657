"""Packed conv operands: the object a conv call reads its weight from, and the cache that keeps
every such object in step with its parameter.

A PackedWeight owns the operands packed from one OIHW parameter - the direct [rows][k_pad] GEMM
operand, its six exact bf16 planes, the Winograd operand U - and the one piece of state that says
which of them the next repack refreshes.  Nothing else decides that: kernels.pack_weight creates
the object, Packs.refresh asks it what is due after the optimizer step, kernels.igemm tells it when
a call takes a direct kernel, kernels.pack_weights tells it when the direct operand was repacked.
"""
import os

import torch

from . import kernels as K

# PU_LAZY_DIRECT=0: refresh every packed direct operand after each optimizer step (A/B runs)
_LAZY = os.environ.get("PU_LAZY_DIRECT", "1") != "0"

# PackedWeight.state.  A layer that has only ever run on the Winograd kernel gets only its U
# refreshed after the optimizer step; its direct operand is repacked by the first call that takes
# a direct kernel, and with every repack from then on.
KEPT = "KEPT"                  # direct (+ planes) is refreshed with every repack
WINO_FRESH = "WINO_FRESH"      # only U is refreshed; direct currently matches src
WINO_STALE = "WINO_STALE"      # only U is refreshed; direct is behind src


class PackedWeight:
    """The GEMM operands of one parameter in one layout (mode, k_pad, cgroup, dtype)."""
    __slots__ = ("src", "mode", "k_pad", "cgroup", "dtype", "direct", "planes", "wino", "state", "version")

    def __init__(self, src, mode, k_pad, cgroup, direct, planes=None, wino=None):
        self.src = src                  # the fp32 OIHW parameter
        self.mode, self.k_pad, self.cgroup, self.dtype = mode, k_pad, cgroup, direct.dtype
        self.direct = direct            # packed [rows][k_pad], fp32 or bf16
        self.planes = planes            # its six-plane bf16 split (kernels.split_weight6), or None
        self.wino = wino                # U (kernels.pack_wino), or None
        self.state = KEPT if wino is None else WINO_FRESH
        self.version = src._version     # the src._version the operands were packed from

    def data_ptr(self):
        """The address a conv call passes as its weight (pu_conv_args.weight): the direct operand's."""
        return self.direct.data_ptr()

    def repack_due(self):
        """src moved: (refresh direct + planes, refresh U) for the repack about to be issued."""
        lazy = _LAZY and self.state != KEPT
        if lazy:
            self.state = WINO_STALE
        return not lazy, self.wino is not None

    def take_direct(self):
        """A call is about to take a direct kernel: direct is refreshed with every repack from
        now on.  True if it has to be repacked before this call."""
        stale, self.state = self.state == WINO_STALE, KEPT
        return stale

    def direct_repacked(self):
        """direct (+ planes) was just repacked from src."""
        if self.state == WINO_STALE:
            self.state = WINO_FRESH


class Packs:
    """Packed GEMM operands of the OIHW parameters, rebuilt only when a parameter changes.

    The cache keys on the parameter's storage and checks its version counter (the optimizer and
    the DP broadcast bump it).  ``refresh()`` - called once at the start of every trunk forward -
    re-packs every stale entry in place with ONE multi-tensor launch (pu_pack_weights: pack + exact
    bf16 split fused) instead of two launches per operand at first use, and one more for the
    Winograd operands (pu_pack_wino)."""

    def __init__(self):
        self.cache = {}

    def get(self, w, mode, k_pad, cgroup=0, dtype=torch.float32):
        # keyed by storage (detached views share the parameter's version counter)
        key = (w.data_ptr(), tuple(w.shape), mode, cgroup, dtype)
        hit = self.cache.get(key)
        if hit is not None and hit.version == w._version and hit.k_pad == k_pad:
            return hit
        # src is w itself, not a detached view: refresh() sees it when the parameter's storage moves
        packed = self.cache[key] = K.pack_weight(w, mode, k_pad, cgroup=cgroup, dtype=dtype)
        return packed

    def refresh(self):
        stale = [p for key, p in self.cache.items() if p.src._version != p.version and p.src.data_ptr() == key[0]]
        if stale:
            due = [p.repack_due() for p in stale]
            K.pack_weights([p for p, (direct, _) in zip(stale, due) if direct], wino=False)
            K.pack_wino([(p.src, p.wino, p.mode == 1) for p, (_, u) in zip(stale, due) if u])
            for p in stale:
                p.version = p.src._version
