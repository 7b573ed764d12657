"""Host side of the device validation metrics (kernels.seg_metrics / pu_seg_metrics).

A validation pass runs the forward chunk by chunk and makes one seg_metrics call per chunk.  What the
host needs of it is a table of N rows (one per sample) of int64: the bits of the sample's fp32 loss
and its pixel counts.  MetricTable collects the per-chunk device tensors without synchronising and
brings the table to the host in ONE copy at the end.

Under data parallelism the chunks are dealt to the ranks (chunks_for_rank) and the table is merged by
one SUM all-reduce (merge_table): a row a rank did not compute is zero on it, so the sum of the
integers is exact and every rank holds the bits the single process holds.  Whole chunks are dealt,
not samples: the split-K plans of the forward depend on the batch size, and a chunk computed with the
same batch on any rank gives the single process's bits.
"""
import numpy as np
import torch
import torch.distributed as dist

LOSS_COL, COUNT_COL = 0, 1       # columns of the table: the loss bits, then the counts row


def world_and_rank():
    """(world size, rank) of the default process group; (1, 0) without one."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def chunks_for_rank(n, batch, world=1, rank=0):
    """The (start, stop) sample ranges of the chunks of ``batch`` samples (the last one ragged) that
    ``rank`` of ``world`` evaluates: chunk i goes to rank i % world."""
    if n < 0 or batch <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError("chunks_for_rank: n %r, batch %r, world %r, rank %r" % (n, batch, world, rank))
    return [(s, min(n, s + batch)) for i, s in enumerate(range(0, n, batch)) if i % world == rank]


def merge_table(table):
    """Sum an int64 [N, cols] device table over the ranks of the default group and return it on the
    host (numpy).  One all-reduce - on the device tensor for nccl, on the host copy for gloo - and one
    device-to-host copy; without a group, or in a world of one, the copy alone."""
    if table.dtype != torch.int64 or table.dim() != 2:
        raise ValueError("merge_table: an int64 [N, cols] tensor, not %s %s" % (table.dtype, tuple(table.shape)))
    world, _ = world_and_rank()
    if world > 1 and dist.get_backend() != "gloo":
        dist.all_reduce(table, op=dist.ReduceOp.SUM)
    host = table.cpu()
    if world > 1 and dist.get_backend() == "gloo":
        dist.all_reduce(host, op=dist.ReduceOp.SUM)
    return host.numpy()


class MetricTable:
    """The [N, 1 + 2 + 2 T] int64 table of a validation pass over N samples with T thresholds."""

    def __init__(self, n, n_thr, device):
        self.n, self.n_thr, self.device = n, n_thr, device
        self.parts = []            # (start, loss [B] float32, counts [B, 2 + 2 T] int64), on the device
        self.host = None

    def add(self, start, loss, counts):
        """The seg_metrics result of the chunk whose first sample is ``start``; no synchronisation."""
        if counts.shape != (loss.shape[0], 2 + 2 * self.n_thr) or start < 0 or start + loss.shape[0] > self.n:
            raise ValueError("MetricTable.add: chunk at %d of %d samples, counts %s" % (start, self.n, tuple(counts.shape)))
        self.parts.append((start, loss, counts))

    def finish(self, across_ranks=True):
        """Build the table on the device, merge it across ranks (unless told that this process holds
        every chunk) and copy it to the host, once."""
        table = torch.zeros((self.n, COUNT_COL + 2 + 2 * self.n_thr), dtype=torch.int64, device=self.device)
        for start, loss, counts in self.parts:
            rows = table[start:start + loss.shape[0]]
            rows[:, LOSS_COL] = loss.view(torch.int32)        # the bits, sign-extended: exact under the sum
            rows[:, COUNT_COL:] = counts
        self.host = merge_table(table) if across_ranks else table.cpu().numpy()
        self.parts = []
        return self

    # ---- the columns, on the host after finish()
    def losses(self):
        """float32 [N]: the per-sample mean BCE"""
        return self.host[:, LOSS_COL].astype(np.int32).view(np.float32)

    def agree(self):
        return self.host[:, COUNT_COL]

    def tcount(self):
        return self.host[:, COUNT_COL + 1]

    def pcount(self, k):
        return self.host[:, COUNT_COL + 2 + k]

    def icount(self, k):
        return self.host[:, COUNT_COL + 2 + self.n_thr + k]
