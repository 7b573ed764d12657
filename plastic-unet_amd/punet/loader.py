"""Host -> HBM input pipeline of the training loop: double-buffered, pinned-memory, asynchronous.

The reference copies every sample to the device inside the hot loop (src/train.py:94-95,
``torch.from_numpy(...).to(device)`` per sample, synchronous).  Keeping the whole training set in
HBM instead does not scale past device memory, so batches stream:

  host numpy (any dtype, may be a memmap)  --np.copyto-->  pinned staging slot k
  pinned slot k  --async H2D on a copy stream-->  device slot k   (overlaps the previous step)
  compute stream waits on slot k's copy event, trains on it, then marks slot k consumed

``depth`` slots rotate (2 = double buffering).  A device slot is overwritten only after the
compute stream has recorded that it finished the step reading it; a pinned slot is refilled only
after the copy that read it has completed (host waits on that event).  On a CPU device the same
iterator degenerates to plain copies (test harness for the ordering logic; the product trains on
the GPU).

With an augmentation plan (punet/augment.py) slot k also carries the batch's rows of the epoch's table
(pinned, and a device copy) and a second pair of device buffers:

  pinned slot k  --async H2D-->  raw device slot k  --kernels.augment on the copy stream-->  augmented slot k

and it is the augmented pair that the compute stream reads, so the wait on ``consumed[k]`` comes before
that launch; the raw pair is touched by the copy stream alone.  The kernel runs under the previous step
like the copies do.

With a fit (punet/fit.py: the net's side is not the data's) slot k has one more pair of device buffers at the
net's size, filled by ``fit.to_net`` on the copy stream from the augmented pair, or from the raw pair when
there is no plan - again after the wait on ``consumed[k]``, since the fitted pair is then the one the compute
stream reads.  Host arrays, pinned slots and the augmentation stay at the data size.
"""
import numpy as np
import torch

from . import kernels as K


class BatchPrefetcher:
    """Iterate device batches ``(x, y)`` for the index ranges ``ranges`` of host arrays X, Y.

    X: [N, ...] inputs, Y: [N, ...] targets (numpy or torch CPU).  Yielded tensors are float32
    views of the device slot; they stay valid until the iterator advances ``depth - 1`` more
    times (the trainer consumes them within its step).

    augment: None, or an AugmentPlan over the samples of X: sample i of epoch e (set_epoch) is yielded
    transformed by row i of plan.table(e), image and mask alike, whatever batch it is in.
    fit: None, or a FitSpec for the H x W of X: the yielded batches are fit.to_net of the above, image and
    mask alike, at the net's side."""

    def __init__(self, X, Y, ranges, device, depth=2, augment=None, fit=None):
        self.X, self.Y = X, Y
        self.ranges = list(ranges)
        self.device = torch.device(device)
        self.depth = max(2, int(depth))
        self.gpu = self.device.type == "cuda"
        bmax = max((hi - lo for lo, hi in self.ranges), default=0)
        xs, ys = tuple(np.shape(X)[1:]), tuple(np.shape(Y)[1:])
        self.host, self.dev = [], []
        for _ in range(self.depth if bmax else 0):
            hx = torch.empty((bmax,) + xs, dtype=torch.float32, pin_memory=self.gpu)
            hy = torch.empty((bmax,) + ys, dtype=torch.float32, pin_memory=self.gpu)
            self.host.append((hx, hy))
            self.dev.append((torch.empty((bmax,) + xs, dtype=torch.float32, device=self.device),
                             torch.empty((bmax,) + ys, dtype=torch.float32, device=self.device)))
        if self.gpu:
            self.stream = torch.cuda.Stream(self.device)
            self.copied = [torch.cuda.Event() for _ in range(self.depth)]
            self.consumed = [None] * self.depth
            self.pinned_busy = [None] * self.depth
        self.plan = augment if augment is not None and augment.spec else None
        if self.plan is not None and bmax:
            if len(xs) != 3 or len(ys) not in (2, 3) or tuple(ys[-2:]) != tuple(xs[-2:]):
                raise ValueError("augment: X must be [N, C, H, W] and Y [N, C, H, W] or [N, H, W] of the same H x W "
                                 "(got %s and %s)" % ((len(X),) + xs, (len(Y),) + ys))
            if self.plan.n_samples < max(hi for _, hi in self.ranges):
                raise ValueError("augment: a plan for %d samples, batches up to sample %d" % (
                    self.plan.n_samples, max(hi for _, hi in self.ranges)))
            self.plan.spec.check_fits(*xs[-2:])
            self.rows_host = [torch.empty((bmax, 4), dtype=torch.int32, pin_memory=self.gpu) for _ in range(self.depth)]
            self.rows_dev = [torch.empty((bmax, 4), dtype=torch.int32, device=self.device) for _ in range(self.depth)]
            self.aug = [(torch.empty_like(dx), torch.empty_like(dy)) for dx, dy in self.dev]
            self.set_epoch(0)
        self.fit = fit if fit else None
        if self.fit is not None and bmax:
            if len(xs) < 2 or len(ys) < 2 or tuple(xs[-2:]) != (self.fit.h, self.fit.w) or tuple(ys[-2:]) != tuple(xs[-2:]):
                raise ValueError("fit: X and Y must end in the spec's %d x %d (got %s and %s)" % (
                    self.fit.h, self.fit.w, (len(X),) + xs, (len(Y),) + ys))
            side = (self.fit.side, self.fit.side)
            self.fitted = [(torch.empty((bmax,) + xs[:-2] + side, dtype=torch.float32, device=self.device),
                            torch.empty((bmax,) + ys[:-2] + side, dtype=torch.float32, device=self.device))
                           for _ in range(self.depth)]

    def __len__(self):
        return len(self.ranges)

    def set_epoch(self, epoch):
        """The epoch whose table the next iteration applies (nothing to do without a plan)."""
        self.epoch = int(epoch)
        if self.plan is not None:
            self.table = self.plan.table(self.epoch)

    def _augment(self, k, lo, n):
        """raw slot k -> augmented slot k by the rows of the samples lo .. lo + n, on the current stream"""
        (dx, dy), (ax, ay) = self.dev[k], self.aug[k]
        rows = self.rows_dev[k][:n] if self.gpu else self.table[lo:lo + n]
        planes = (lambda v: v[:n].unsqueeze(1)) if dy.dim() == 3 else (lambda v: v[:n])
        K.augment(dx[:n], planes(dy), rows, self.plan.max_shift, out=(ax[:n], planes(ay)))

    def _ready(self, k):
        """the pair of slot k that the compute stream reads: fitted, else augmented, else as copied"""
        if self.fit is not None:
            return self.fitted[k]
        return self.dev[k] if self.plan is None else self.aug[k]

    def _fit(self, k, n):
        """augmented (or raw) slot k -> fitted slot k, on the current stream"""
        sx, sy = self.dev[k] if self.plan is None else self.aug[k]
        fx, fy = self.fitted[k]
        self.fit.to_net(sx[:n], out=fx[:n])
        self.fit.to_net(sy[:n], out=fy[:n])

    def _fill(self, i):
        """stage batch i into its pinned slot and issue its H2D copy"""
        k = i % self.depth
        lo, hi = self.ranges[i]
        n = hi - lo
        hx, hy = self.host[k]
        dx, dy = self.dev[k]
        if self.gpu and self.pinned_busy[k] is not None:
            self.pinned_busy[k].synchronize()      # the copy that last read this pinned slot is done
        np.copyto(hx[:n].numpy(), np.asarray(self.X[lo:hi]), casting="same_kind")
        np.copyto(hy[:n].numpy(), np.asarray(self.Y[lo:hi]), casting="same_kind")
        if self.plan is not None:
            np.copyto(self.rows_host[k][:n].numpy(), self.table[lo:hi])
        if not self.gpu:
            dx[:n].copy_(hx[:n])
            dy[:n].copy_(hy[:n])
            if self.plan is not None:
                self._augment(k, lo, n)
            if self.fit is not None:
                self._fit(k, n)
            return
        with torch.cuda.stream(self.stream):
            if self.consumed[k] is not None:
                self.stream.wait_event(self.consumed[k])   # compute finished the step that read slot k
            dx[:n].copy_(hx[:n], non_blocking=True)
            dy[:n].copy_(hy[:n], non_blocking=True)
            if self.plan is not None:
                self.rows_dev[k][:n].copy_(self.rows_host[k][:n], non_blocking=True)
                self._augment(k, lo, n)             # after the wait on consumed[k]: compute reads the augmented pair
            if self.fit is not None:
                self._fit(k, n)                     # likewise: compute reads the fitted pair
            self.copied[k].record(self.stream)
        self.pinned_busy[k] = self.copied[k]

    def __iter__(self):
        if not self.ranges:
            return
        if self.gpu:
            # a caller that stops iterating early (zip over the ranges ends before the generator
            # resumes past its last yield) never recorded the last slot's consumed event: order
            # every slot's next copy after all the compute work enqueued so far
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self.consumed = [ev] * self.depth
        for j in range(min(self.depth - 1, len(self.ranges))):
            self._fill(j)
        for i, (lo, hi) in enumerate(self.ranges):
            nxt = i + self.depth - 1
            if nxt < len(self.ranges):
                self._fill(nxt)
            k = i % self.depth
            n = hi - lo
            if self.gpu:
                torch.cuda.current_stream(self.device).wait_event(self.copied[k])
            dx, dy = self._ready(k)
            yield dx[:n], dy[:n]
            if self.gpu:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                self.consumed[k] = ev
