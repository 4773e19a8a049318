"""The grouped GEMMs of the experts (ops/csrc/moe_gemm.hip) through
``moe_grouped_mm(impl="hip")`` against fp64 per-expert matmuls on the same
bf16-rounded inputs, and a bf16 MoE model running them against the CPU fp32
path.

The only roundings are the fp32 accumulation of n exact bf16 products and one
final rounding to bf16, so element-wise

    |got - ref| <= 2^-8 |ref| + 2 n 2^-24 (|A| @ |B|)

with n the reduction length (K for y, N for da, the expert's row count for
dw) and the factor 2 for the accumulation order inside and between MFMAs."""

import copy

import pytest
import torch

from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
from dlrover_amd.ops import (
    moe_dispatch,
    moe_grouped_mm,
    moe_router_ref,
    moe_sort,
)

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIXED = [0, 1, 127, 128, 129, 0, 300, 3]


def run_hip(x, w, dy, offs, gather=None):
    """Forward and backward on fresh leaves -> (y, dx, dw)."""
    x = x.to(DEV).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    y = moe_grouped_mm(x, w, offs, impl="hip", gather=gather)
    dx, dw = torch.autograd.grad(y, (x, w), dy.to(DEV))
    return y.detach(), dx, dw


def reference(a, w, dy, counts):
    """fp64 (ref, |A| @ |B|, n) of y, da and dw, per-expert matmuls."""
    a, w, dy = a.double(), w.double(), dy.double()
    y, da, dw = (torch.zeros_like(t) for t in (dy, a, w))
    ya, daa, dwa = (torch.zeros_like(t) for t in (dy, a, w))
    start = 0
    for e, c in enumerate(counts):
        rows = slice(start, start + c)
        y[rows], ya[rows] = a[rows] @ w[e], a[rows].abs() @ w[e].abs()
        da[rows] = dy[rows] @ w[e].t()
        daa[rows] = dy[rows].abs() @ w[e].abs().t()
        dw[e], dwa[e] = a[rows].t() @ dy[rows], a[rows].abs().t() @ dy[rows].abs()
        start += c
    n_dw = torch.tensor(counts, dtype=torch.float64).view(-1, 1, 1)
    return dict(y=(y, ya, a.shape[1]), da=(da, daa, dy.shape[1]),
                dw=(dw, dwa, n_dw))


def bound_of(ref, absprod, n):
    return 2.0 ** -8 * ref.abs() + 2 * n * 2.0 ** -24 * absprod


def check(name, got, ref, absprod, n):
    err = (got.double().cpu() - ref).abs()
    bound = bound_of(ref, absprod, n)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: worst err / bound = {ratio:.3f}")
    assert (err <= bound).all(), f"{name}: worst err / bound = {ratio}"


@pytest.mark.parametrize("counts,K,N", [
    (MIXED, 64, 96),
    (MIXED, 288, 160),
    ([0, 0, 0, 200], 64, 96),
    ([200, 0, 0, 0], 64, 96),
    ([1] * 256, 32, 32),
], ids=["mixed", "mixed-tails", "last", "first", "e256"])
def test_grouped_gemm_matches_fp64(counts, K, N):
    """Worst err / bound measured on an MI355X over these cases: y 0.990,
    da 0.991, dw 0.995. That is the final rounding alone: half a bf16 ulp
    reaches 2^-8 |ref| just above a power of two."""
    torch.manual_seed(0)
    bf, R, E = torch.bfloat16, sum(counts), len(counts)
    x, w, dy = (torch.randn(s).to(bf) for s in ((R, K), (E, K, N), (R, N)))
    offs = torch.tensor(counts).cumsum(0).int().to(DEV)
    y, da, dw = run_hip(x, w, dy, offs)
    for a, b in zip((y, da, dw), run_hip(x, w, dy, offs)):
        assert torch.equal(a, b)  # the same bits every call
    ref = reference(x, w, dy, counts)
    for name, got in (("y", y), ("da", da), ("dw", dw)):
        check(name, got, *ref[name])
    for e, c in enumerate(counts):
        if c == 0:
            assert not dw[e].any(), f"dw of empty expert {e}"


def test_forward_with_several_blocks_per_cu():
    """1056 blocks of 8 steps, several per CU: the transposed LDS reads once
    lost words only when blocks competed for a SIMD, which none of the small
    cases make them do. fp64 reference on the GPU, the same bound."""
    torch.manual_seed(0)
    bf, counts, K, N = torch.bfloat16, [3000, 1096], 256, 4096
    x = torch.randn(sum(counts), K, device=DEV).to(bf)
    w = torch.randn(2, K, N, device=DEV).to(bf)
    offs = torch.tensor(counts, device=DEV).cumsum(0).int()
    y = moe_grouped_mm(x, w, offs, impl="hip")
    assert torch.equal(y, moe_grouped_mm(x, w, offs, impl="hip"))
    parts = x.double().split(counts)
    ref = torch.cat([p @ w[e].double() for e, p in enumerate(parts)])
    absprod = torch.cat(
        [p.abs() @ w[e].double().abs() for e, p in enumerate(parts)])
    assert ((y.double() - ref).abs() <= bound_of(ref, absprod, K)).all()


def test_fused_dispatch_matches_dispatch_then_gemm():
    """gather mode against moe_dispatch followed by the ungathered call: y
    and dw bit for bit. dx is that call's bf16 da rows summed per token, so it
    is held (a) to the fp64 sum of those rows with the one-rounding rule of
    test_moe_gpu.py, rtol 2^-7 and atol 1e-4 max|ref|, and (b) to the fp64
    gradient itself within the k da bounds of a token plus the final
    rounding. Measured on an MI355X, worst err / bound: y 0.985, da 0.982,
    dw 0.993, dx by (b) 0.568."""
    torch.manual_seed(0)
    bf, T, k, E, K, N = torch.bfloat16, 67, 8, 16, 64, 96
    idx = moe_router_ref(torch.randn(T, E), k)[0]
    offs, row_of_slot, slot_of_row = moe_sort(idx.to(DEV), E)
    x, w, dy = (torch.randn(s).to(bf) for s in ((T, K), (E, K, N), (T * k, N)))
    gather = (slot_of_row, row_of_slot, k)
    y, dx, dw = run_hip(x, w, dy, offs, gather)
    for a, b in zip((y, dx, dw), run_hip(x, w, dy, offs, gather)):
        assert torch.equal(a, b)
    xp = moe_dispatch(x.to(DEV), slot_of_row, row_of_slot, k)
    y2, da2, dw2 = run_hip(xp, w, dy, offs)
    assert torch.equal(y, y2) and torch.equal(dw, dw2)

    counts = torch.diff(offs.cpu(), prepend=torch.zeros(1, dtype=torch.int32))
    ref = reference(xp.cpu(), w, dy, counts.tolist())
    for name, got in (("y", y), ("da", da2), ("dw", dw)):
        check(name, got, *ref[name])
    assert not dw.cpu()[counts == 0].any()
    rows = row_of_slot.cpu().long()
    want = da2.double().cpu()[rows].view(T, k, K).sum(1)
    torch.testing.assert_close(dx.double().cpu(), want, rtol=2.0 ** -7,
                               atol=1e-4 * want.abs().max().item())
    da64, _, _ = ref["da"]
    dx64 = da64[rows].view(T, k, K).sum(1)
    slack = bound_of(*ref["da"])[rows].view(T, k, K).sum(1)
    fp32_sum = k * 2.0 ** -23 * da64.abs()[rows].view(T, k, K).sum(1)
    bound = 2.0 ** -8 * (dx64.abs() + slack) + slack + fp32_sum
    err = (dx.double().cpu() - dx64).abs()
    print(f"dx: worst err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def test_grouped_gemm_rejections():
    bf = torch.bfloat16
    offs = torch.tensor([2, 4], dtype=torch.int32, device=DEV)
    x = torch.randn(4, 64, device=DEV).to(bf)
    w = torch.randn(2, 64, 32, device=DEV).to(bf)
    gather = (torch.arange(4, dtype=torch.int32, device=DEV),) * 2 + (1,)
    with pytest.raises(ValueError):  # K % 32 != 0
        moe_grouped_mm(x[:, :48].contiguous(), w[:, :48].contiguous(), offs,
                       impl="hip")
    with pytest.raises(ValueError):  # fp32 input
        moe_grouped_mm(x.float(), w.float(), offs, impl="hip")
    with pytest.raises(ValueError):
        moe_grouped_mm(x, w, offs, impl="library", gather=gather)
    with pytest.raises(ValueError):
        moe_grouped_mm(x, w, offs, impl="rocblas")


def test_llama_moe_hip_gemm_gpu_matches_cpu_fp32():
    """test_llama_moe_gpu_matches_cpu_fp32 with moe_expert_gemm="hip": the
    same config, seed, 2% cap on flipped selections and bounds, and the
    gradient of experts_down compared as well."""
    torch.manual_seed(55)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512, n_layers=2,
        n_heads=2, n_kv_heads=2, max_seq_len=64, rope_base=10000.0,
        n_experts=8, n_experts_per_tok=2, moe_aux_coef=0.01,
        moe_expert_gemm="hip")
    cpu = LlamaForCausalLM(cfg)
    with torch.no_grad():
        for p in cpu.parameters():  # both models hold bf16-exact weights
            p.copy_(p.bfloat16().float())
    gpu = copy.deepcopy(cpu).to(DEV).bfloat16()
    ids = torch.randint(0, cfg.vocab_size, (2, 64))
    losses, picks = [], []
    for model, dev in ((cpu, "cpu"), (gpu, DEV)):
        seen = []
        hooks = [blk.mlp.router.register_forward_hook(
            lambda m, i, o: seen.append(o.detach().float().cpu()))
            for blk in model.blocks]
        loss = model(ids.to(dev), ids.to(dev))
        loss.backward()
        for h in hooks:
            h.remove()
        losses.append(loss.float().cpu())
        picks.append(torch.stack(
            [moe_router_ref(l, 2)[0].sort(-1).values for l in seen]))
    flipped = (picks[0] != picks[1]).any(-1).any(0)  # per token, any layer
    assert flipped.float().mean().item() <= 0.02, flipped.sum()
    torch.testing.assert_close(losses[1], losses[0], rtol=2e-2, atol=2e-2)
    for b_cpu, b_gpu in zip(cpu.blocks, gpu.blocks):
        for name in ("router.weight", "experts_gate_up", "experts_down"):
            want = b_cpu.mlp.get_parameter(name).grad
            torch.testing.assert_close(
                b_gpu.mlp.get_parameter(name).grad.float().cpu(), want,
                rtol=5e-2, atol=5e-2 * want.abs().max().item())
