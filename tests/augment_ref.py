"""What tests/test_augment.py and tests/test_augment_gpu.py share: pu_augment and pu_flip_mean restated in
numpy - the shift as numpy.pad(mode='reflect') and a slice, the flip as a reversed view, never through the
index formula of the kernel -, the tables the tests apply, and a stand-in for kernels.augment on CPU
tensors."""
import numpy as np
import torch


def augment_planes(a, flip, dy, dx):
    """a [..., h, w] of any dtype -> the planes translated by (dy, dx) with reflected borders, then mirrored
    left-right when flip is set.  A copy of elements only: the bits of a survive."""
    a = np.asarray(a)
    h, w = a.shape[-2:]
    S = max(abs(int(dy)), abs(int(dx)))
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(S, S), (S, S)], mode="reflect")
    out = p[..., S - dy:S - dy + h, S - dx:S - dx + w]
    return np.ascontiguousarray(out[..., ::-1] if flip else out)


def augment_batch(x, rows):
    """x [B, ...planes..., h, w], rows [B, 4] of {flip, dy, dx, 0}: slot b transformed by row b"""
    x, rows = np.asarray(x), np.asarray(rows)
    assert rows.shape == (x.shape[0], 4)
    return np.stack([augment_planes(x[b], int(rows[b, 0]), int(rows[b, 1]), int(rows[b, 2])) for b in range(x.shape[0])])


def flip_mean(y, y_mirror):
    """0.5f * (y + mirror(y_mirror)) in float32: one addition, one multiplication"""
    y, m = np.asarray(y, dtype=np.float32), np.asarray(y_mirror, dtype=np.float32)
    return (np.float32(0.5) * (y + m[..., ::-1])).astype(np.float32)


def grid_rows(S, extra=4, seed=0):
    """Both flips x dy, dx in {-S, 0, S} (each row once), then `extra` random rows within +-S."""
    rows = sorted({(f, dy, dx, 0) for f in (0, 1) for dy in (-S, 0, S) for dx in (-S, 0, S)})
    g = np.random.RandomState(seed + S)
    for _ in range(extra):
        rows.append((int(g.randint(0, 2)), int(g.randint(-S, S + 1)), int(g.randint(-S, S + 1)), 0))
    return np.array(rows, dtype=np.int32)


def random_words(shape, seed):
    """float32 of every kind: uniformly random 32-bit patterns (NaNs, infinities, denormals among them)"""
    return np.random.RandomState(seed).randint(0, 1 << 32, size=shape, dtype=np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def numpy_augment(calls):
    """kernels.augment on CPU tensors, for the host-side plumbing; calls receives (batch, rows, max_shift)"""
    def augment(x, t, table, max_shift, out=None):
        rows = np.array(table.numpy() if isinstance(table, torch.Tensor) else table)
        calls.append((x.shape[0], rows, max_shift))
        assert np.abs(rows[:, 1:3]).max(initial=0) <= max_shift
        xo = torch.from_numpy(augment_batch(bits(x.numpy()), rows).view(np.float32))
        to = torch.from_numpy(augment_batch(bits(t.numpy()), rows).view(np.float32)) if t is not None else None
        if out is not None:
            out[0].copy_(xo)
            if t is not None:
                out[1].copy_(to)
            return out
        return xo, to
    return augment
