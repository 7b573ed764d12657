"""Fused plastic head forward (pu_plastic_head_fwd) at bs 32 x 128^2, C = 64: us per launch and
algorithmic GB/s (the bench line's oja_update.fused_head_bs32), for the library PLASTIC_UNET_LIB
points at (ablation variants).   python tools/head_bench.py [label] [B N C]  (default 32 128 64 = C2;
32 256 8 = C4)
python tools/head_bench.py bwd-trace [B N]: the head backward with the trace gradient
(pu_plastic_bwd_trace) against pu_plastic_bwd at the same shape (default 32 128, the C2 head)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from punet import kernels as K  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)


def bwd_trace_mode(B, N, rounds=5):
    """python tools/head_bench.py bwd-trace [B N]: the head backward with the trace gradient
    (pu_plastic_bwd_trace: dX, dw, dalpha, dH, deta) next to today's pu_plastic_bwd at the same
    shape, alternated in one process; us (best of `rounds`), the extra time over pu_plastic_bwd and
    what the extra bytes (trace backward 8 B N^2 + dH finish 16 B N^2) come to in GB/s."""
    torch.manual_seed(0)
    X, P, dY = (torch.randn(B, N, N, device=dev) for _ in range(3))
    H = 0.2 * torch.randn(B, N, N, device=dev)
    w = 0.01 * torch.randn(N, N, device=dev)
    a = 0.5 * torch.rand(N, N, device=dev)
    eta = torch.full((1,), 0.1, device=dev)
    for rule, name in ((0, "hebb"), (1, "oja")):
        Y, _ = K.plastic_fwd(X, H, w, a, eta, rule, True)
        cases = (("plastic_bwd", lambda: K.plastic_bwd(X, H, w, a, Y, dY)),
                 ("bwd_trace", lambda: K.plastic_bwd_trace(X, H, w, a, eta, Y, dY, P, rule)),
                 ("bwd_trace no dH", lambda: K.plastic_bwd_trace(X, H, w, a, eta, Y, dY, P, rule, need_dh=False)))
        best = {}
        for _ in range(rounds):
            for label, fn in cases:
                us, how = bench._launch_time_us(fn, 50)
                best[label] = min(us, best.get(label, 1e30))
        base = best["plastic_bwd"]
        for label, _ in cases:
            extra = best[label] - base
            nb = K.plastic_bwd_trace_bytes(B, N, True, label == "bwd_trace") if label != "plastic_bwd" else 0.0
            tail = "" if not nb else "  +%.2f us over plastic_bwd for %.1f MB: %.0f GB/s, %.3f of 8 TB/s" % (
                extra, nb / 1e6, nb / max(extra, 1e-9) / 1e3, nb / max(extra, 1e-9) / 8e6)
            print("%-4s bs %d x %d^2  %-16s %8.2f us%s  (%s)" % (name, B, N, label, best[label], tail, how))


if len(sys.argv) > 1 and sys.argv[1] == "bwd-trace":
    bwd_trace_mode(*((int(v) for v in sys.argv[2:4]) if len(sys.argv) >= 4 else (32, 128)))
    sys.exit(0)

B, N, C = (int(v) for v in sys.argv[2:5]) if len(sys.argv) >= 5 else (32, 128, 64)
torch.manual_seed(0)
H = 0.1 * torch.randn(B, N, N, device=dev)
w = 0.01 * torch.randn(N, N, device=dev)
a = 0.01 * torch.rand(N, N, device=dev)
eta = torch.full((1,), 0.01, device=dev)
feat = torch.rand(B, N, N, C, device=dev)
wo = 0.1 * torch.randn(C, device=dev)
bo = torch.zeros(1, device=dev)
us, how = bench._launch_time_us(lambda: K.plastic_head_fwd(feat, wo, bo, H, w, a, eta, 1, True), 50)
nbytes = 4.0 * B * N * N * C + 16.0 * B * N * N + 8.0 * N * N
print("%-24s %8.2f us  %7.1f GB/s  %.3f of 8 TB/s  (%s)" % (sys.argv[1] if len(sys.argv) > 1 else
      os.path.basename(os.environ.get("PLASTIC_UNET_LIB", "default")), us, nbytes / us / 1e3, nbytes / us / 8e6, how))
