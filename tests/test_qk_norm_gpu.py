"""ops.qk_norm_rope HIP kernels (ops/csrc/qk_norm_rope.hip) against the same
math in fp64 with autograd on the bf16-rounded inputs.

Tolerance for y, dx and dw: rtol 2^-7 (one bf16 ulp: the only rounding is the
final store, and another fp32 operation order may flip it) plus
atol 1e-4 * max|ref| (fp32 noise where the two rotation terms cancel)."""

import copy

import pytest
import torch

from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
from dlrover_amd.ops import qk_norm_rope
from dlrover_amd.ops.api import build_rope_cache

pytestmark = pytest.mark.gpu
EPS = 1e-6


def ref64(q, k, wq, wk, pos, cos, sin):
    def one(x, w):
        d = x.shape[-1]
        n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w
        c = cos.double()[pos.long()].view(*x.shape[:-2], 1, d // 2)
        s = sin.double()[pos.long()].view(*x.shape[:-2], 1, d // 2)
        n1, n2 = n[..., : d // 2], n[..., d // 2:]
        return torch.cat([n1 * c - n2 * s, n2 * c + n1 * s], -1)

    return one(q, wq), one(k, wk)


def close(got, want, name):
    torch.testing.assert_close(
        got.double().cpu(), want, rtol=2.0 ** -7,
        atol=1e-4 * want.abs().max().item(), msg=lambda m: f"{name}: {m}")


# (B, S, nh, nkv, D, variant). q/k are slices of one packed
# [B, S, (nh+2nkv)*D] tensor except in "contiguous". (2,5,5,1,128): 6 head
# rows per token, 60 in all, the last wave partly filled. (1,67,3,3,64): the
# 4-lanes-per-head mapping, odd token count, nh == nkv. (2,1040,32,8,128):
# 83,200 head rows = 2600 row groups of 32 against the 2048-block grid cap,
# so the grid-stride loop and the cross-iteration dw accumulation run twice
# in 552 blocks.
@pytest.mark.parametrize("B,S,nh,nkv,D,variant", [
    (2, 5, 5, 1, 128, "shared_pos"),
    (2, 5, 5, 1, 128, "per_token_pos"),
    (2, 5, 5, 1, 128, "contiguous"),
    (1, 67, 3, 3, 64, "shared_pos"),
    (2, 1040, 32, 8, 128, "shared_pos"),
])
def test_qk_norm_rope_matches_fp64(B, S, nh, nkv, D, variant):
    torch.manual_seed(0)
    dev, bf = "cuda", torch.bfloat16
    cos, sin = build_rope_cache(S, D, 10000.0)
    pos = torch.arange(S, dtype=torch.int32)
    if variant == "per_token_pos":  # [B, S], restarting mid-sequence
        pos = pos.repeat(B, 1)
        pos[0, 2:] -= 2
        pos[1, 3:] -= 3
    qkv = torch.randn(B, S, (nh + 2 * nkv) * D).to(bf)
    dq = torch.randn(B, S, nh, D).to(bf)
    dk = torch.randn(B, S, nkv, D).to(bf)
    wq, wk = ((1 + 0.3 * torch.randn(D)).to(bf) for _ in range(2))

    def split(t):
        q, k, _ = t.split([nh * D, nkv * D, nkv * D], dim=-1)
        return q.view(B, S, nh, D), k.view(B, S, nkv, D)

    leaves = [t.to(dev).requires_grad_(True) for t in (qkv, wq, wk)]
    q, k = split(leaves[0])
    dq_g, dk_g = dq.to(dev), dk.to(dev)
    if variant == "contiguous":  # and a non-contiguous upstream gradient
        q, k = q.contiguous(), k.contiguous()
        dq_g = dq_g.transpose(1, 2).contiguous().transpose(1, 2)
        dk_g = dk_g.transpose(1, 2).contiguous().transpose(1, 2)
    oq, ok = qk_norm_rope(q, k, leaves[1], leaves[2], pos.to(dev),
                          cos.to(dev), sin.to(dev), EPS)
    assert oq.is_contiguous() and ok.is_contiguous()
    grads = [torch.autograd.grad((oq, ok), leaves, (dq_g, dk_g),
                                 retain_graph=True) for _ in range(2)]
    # no floating-point atomics: two backward calls give the same bits
    assert torch.equal(grads[0][1], grads[1][1])
    assert torch.equal(grads[0][2], grads[1][2])

    leaves64 = [t.double().requires_grad_(True) for t in (qkv, wq, wk)]
    rq, rk = ref64(*split(leaves64[0]), leaves64[1], leaves64[2],
                   pos.expand(B, S), cos, sin)
    want = torch.autograd.grad((rq, rk), leaves64, (dq.double(), dk.double()))
    close(oq, rq.detach(), "q_out")
    close(ok, rk.detach(), "k_out")
    dx, dx64 = split(grads[0][0]), split(want[0])
    close(dx[0], dx64[0], "dx_q")
    close(dx[1], dx64[1], "dx_k")
    close(grads[0][1], want[1], "dwq")
    close(grads[0][2], want[2], "dwk")


def test_llama_qk_norm_gpu_matches_cpu_fp32():
    """bf16 model on the GPU against the same weights through the CPU fp32
    path. test_ops_gpu.test_llama_tiny_gpu_step compares no two values, so
    the bounds are the ones this suite uses for a bf16 model against fp32
    (test_doc_mask_gpu): 2e-2 on the loss, 5e-2 on gradients, the gradient's
    absolute part scaled by max|ref| since a norm-weight gradient is small."""
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512, n_layers=2,
        n_heads=2, n_kv_heads=1, max_seq_len=64, rope_base=10000.0,
        norm_eps=1e-6, qk_norm=True)
    cpu = LlamaForCausalLM(cfg)
    with torch.no_grad():
        for blk in cpu.blocks:
            for norm in (blk.attn.q_norm, blk.attn.k_norm):
                norm.weight.add_(0.3 * torch.randn_like(norm.weight))
        for p in cpu.parameters():  # both models hold bf16-exact weights
            p.copy_(p.bfloat16().float())
    gpu = copy.deepcopy(cpu).to("cuda").bfloat16()
    ids = torch.randint(0, cfg.vocab_size, (2, 64))
    losses = []
    for model, dev in ((cpu, "cpu"), (gpu, "cuda")):
        loss = model(ids.to(dev), ids.to(dev))
        loss.backward()
        losses.append(loss.float().cpu())
    torch.testing.assert_close(losses[1], losses[0], rtol=2e-2, atol=2e-2)
    for b_cpu, b_gpu in zip(cpu.blocks, gpu.blocks):
        want = b_cpu.attn.q_norm.weight.grad
        torch.testing.assert_close(
            b_gpu.attn.q_norm.weight.grad.float().cpu(), want, rtol=5e-2,
            atol=5e-2 * want.abs().max().item())
