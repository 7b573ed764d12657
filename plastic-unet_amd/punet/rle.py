"""Host side of the device run-length encoding (kernels.rle_encode / pu_rle_encode).

The entry compares (double)y > th.  NumPy compares an fp32 array with a threshold in one of two ways:
against a Python float (or an fp32 scalar) in fp32, with the threshold rounded to fp32 first; against
an np.float64 scalar in fp64.  compare_value turns a threshold into the double that makes the device
compare NumPy's own: (double)y > (double)(float)thr is the fp32 comparison exactly.

What the host needs of a chunk is its table of runs: the offsets (B + 1 integers) and the pairs in
use.  RunTable brings those back in two small copies; rle_strings prints them as utils.encode does.
"""
import numpy as np
import torch


def compare_value(thr):
    """The double th for which (double)y > th is what NumPy's ``y > thr`` gives on an fp32 array y:
    thr itself for an np.float64 (a strong fp64 scalar), thr rounded to fp32 for a Python float or
    int and for an np.float32."""
    if isinstance(thr, np.float64) or (isinstance(thr, np.ndarray) and thr.dtype == np.float64):
        return float(thr)                    # np.float64 is a Python float too: asked first
    return float(np.float32(thr))


def rle_strings(offsets, runs):
    """Host offsets [B + 1] and runs [>= total, 2] -> the B strings utils.encode gives ("" for an empty mask)."""
    offsets = np.asarray(offsets)
    runs = np.asarray(runs)
    return [" ".join(map(str, runs[offsets[b]:offsets[b + 1]].ravel().tolist())) for b in range(len(offsets) - 1)]


_COPY_STREAMS = {}       # device index -> the stream the tables come back on


class RunTable:
    """The run table of one chunk, on the device until fetch().  Made right after the chunk's
    rle_encode; fetch() waits for that call alone, not for work enqueued after it, so the device goes
    on with the next chunk while the host reads and prints this one."""

    def __init__(self, offsets, runs):
        if offsets.dim() != 1 or runs.dim() != 2 or runs.shape[1] != 2:
            raise ValueError("RunTable: offsets [B + 1] and runs [cap, 2], not %s and %s" % (tuple(offsets.shape),
                                                                                            tuple(runs.shape)))
        self.offsets, self.runs = offsets, runs
        self.done = None
        if offsets.is_cuda:
            self.done = torch.cuda.Event()
            self.done.record()

    def fetch(self):
        """(offsets [B + 1], runs [total, 2]) as numpy arrays: the offsets, then the pairs in use."""
        if self.done is None:
            offsets = self.offsets.numpy()
            return offsets, self.runs[:int(offsets[-1])].numpy()
        index = self.offsets.device.index
        if index not in _COPY_STREAMS:
            _COPY_STREAMS[index] = torch.cuda.Stream(self.offsets.device)
        side = _COPY_STREAMS[index]
        side.wait_event(self.done)
        with torch.cuda.stream(side):
            offsets = self.offsets.cpu().numpy()
            runs = self.runs[:int(offsets[-1])].cpu().numpy()
        return offsets, runs

    def strings(self):
        return rle_strings(*self.fetch())
