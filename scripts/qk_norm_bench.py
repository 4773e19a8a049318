"""Times ops.qk_norm_rope against the composite it replaces (ops.rmsnorm on
the [T*H, D] views + ops.rope_rotate, for q and for k) at the 8B shape, q/k
as slices of the packed QKV projection, forward and backward, in one
process: device events, 200 calls per sample, 7 alternating rounds, medians.
Needs an MI355X. profiles/qk_norm_rope.txt holds a run."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dlrover_amd import ops  # noqa: E402
from dlrover_amd.ops.api import build_rope_cache  # noqa: E402

T, NH, NKV, D = 8192, 32, 8, 128
ITERS, ROUNDS = 200, 7
dev = "cuda"
torch.manual_seed(0)
qkv = torch.randn(1, T, (NH + 2 * NKV) * D, device=dev).bfloat16()
wq = (1 + 0.3 * torch.randn(D, device=dev)).bfloat16().requires_grad_(True)
wk = (1 + 0.3 * torch.randn(D, device=dev)).bfloat16().requires_grad_(True)
cos, sin = (t.to(dev) for t in build_rope_cache(T, D, 1e6))
pos = torch.arange(T, dtype=torch.int32, device=dev)
q = qkv[..., : NH * D].view(1, T, NH, D).requires_grad_(True)
k = qkv[..., NH * D: (NH + NKV) * D].view(1, T, NKV, D).requires_grad_(True)
dq = torch.randn(1, T, NH, D, device=dev).bfloat16()
dk = torch.randn(1, T, NKV, D, device=dev).bfloat16()
leaves = (q, k, wq, wk)


def fused():
    return ops.qk_norm_rope(q, k, wq, wk, pos, cos, sin, 1e-6)


def composite():
    qn = ops.rmsnorm(q.reshape(T * NH, D), wq, 1e-6).view(1, T, NH, D)
    kn = ops.rmsnorm(k.reshape(T * NKV, D), wk, 1e-6).view(1, T, NKV, D)
    return (ops.rope_rotate(qn, pos, cos, sin),
            ops.rope_rotate(kn, pos, cos, sin))


def timed(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS  # us per call


res = {}
outs = {"fused": fused(), "composite": composite()}
grads = {n: torch.autograd.grad(o, leaves, (dq, dk), retain_graph=True)
         for n, o in outs.items()}
for a, b, name in zip(outs["fused"] + grads["fused"],
                      outs["composite"] + grads["composite"],
                      ["q_out", "k_out", "dx_q", "dx_k", "dwq", "dwk"]):
    err = (a.float() - b.float()).abs().max().item()
    print(f"fused vs composite {name}: max abs diff {err:.4g} "
          f"(max |composite| {b.float().abs().max().item():.4g})")
for r in range(ROUNDS):
    for name, fn in (("fused", fused), ("composite", composite)):
        res.setdefault(name + "_fwd", []).append(timed(fn))
        o = outs[name]
        res.setdefault(name + "_bwd", []).append(timed(
            lambda: torch.autograd.grad(o, leaves, (dq, dk), retain_graph=True)))
rows = T * (NH + NKV)
fwd_bytes = rows * D * 2 * 2 + rows * 4
bwd_bytes = rows * D * 2 * 3 + rows * 4
lines = [f"shape: T={T} nh={NH} nkv={NKV} D={D}, q/k slices of packed qkv; "
         f"{ITERS} calls per sample, {ROUNDS} alternating rounds, device events"]
med = {}
for key, v in res.items():
    med[key] = statistics.median(v)
    lines.append(f"{key:15s} median {med[key]:8.1f} us/call  "
                 f"(min {min(v):.1f}, max {max(v):.1f})")
lines.append(f"fused fwd: {fwd_bytes / 1e6:.1f} MB -> "
             f"{fwd_bytes / med['fused_fwd'] / 1e3:.0f} GB/s (call time)")
lines.append(f"fused bwd: {bwd_bytes / 1e6:.1f} MB -> "
             f"{bwd_bytes / med['fused_bwd'] / 1e3:.0f} GB/s (call time, "
             "includes the dw reduction launch)")
lines.append(f"speedup fwd {med['composite_fwd'] / med['fused_fwd']:.2f}x, "
             f"bwd {med['composite_bwd'] / med['fused_bwd']:.2f}x")
print("\n".join(lines))
