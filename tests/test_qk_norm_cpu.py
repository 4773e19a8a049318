"""ops.qk_norm_rope on the CPU path and LlamaConfig.qk_norm.

Reference: the same math in fp64 with autograd on the bf16-rounded inputs.
Tolerance for y, dx and dw: rtol 2^-7 (one bf16 ulp: the only rounding is the
final store, and another fp32 operation order may flip it) plus
atol 1e-4 * max|ref| (fp32 noise where the two rotation terms cancel)."""

from types import SimpleNamespace

import pytest
import torch

from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
from dlrover_amd.ops import qk_norm_rope
from dlrover_amd.ops.api import build_rope_cache


def ref64(q, k, wq, wk, pos, cos, sin, eps):
    def one(x, w):
        d = x.shape[-1]
        n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
        c = cos.double()[pos.long()].view(*x.shape[:-2], 1, d // 2)
        s = sin.double()[pos.long()].view(*x.shape[:-2], 1, d // 2)
        n1, n2 = n[..., : d // 2], n[..., d // 2:]
        return torch.cat([n1 * c - n2 * s, n2 * c + n1 * s], -1)

    return one(q, wq), one(k, wk)


def close(got, want):
    torch.testing.assert_close(
        got.double(), want, rtol=2.0 ** -7,
        atol=1e-4 * want.abs().max().item())


@pytest.mark.parametrize("B,S,nh,nkv,D", [(2, 5, 5, 1, 128), (1, 67, 3, 3, 64)])
def test_qk_norm_rope_cpu_matches_fp64(B, S, nh, nkv, D):
    torch.manual_seed(0)
    eps = 1e-6
    cos, sin = build_rope_cache(128, D, 10000.0)
    pos = torch.randint(0, 128, (B, S), dtype=torch.int32)
    bf = torch.bfloat16
    q, k, dq, dk = (torch.randn(B, S, h, D).to(bf)
                    for h in (nh, nkv, nh, nkv))
    wq, wk = ((1 + 0.3 * torch.randn(D)).to(bf) for _ in range(2))
    ins = [t.clone().requires_grad_(True) for t in (q, k, wq, wk)]
    oq, ok = qk_norm_rope(*ins, pos, cos, sin, eps)
    torch.autograd.backward((oq, ok), (dq, dk))
    ins64 = [t.double().requires_grad_(True) for t in (q, k, wq, wk)]
    rq, rk = ref64(*ins64, pos.expand(B, S), cos, sin, eps)
    torch.autograd.backward((rq, rk), (dq.double(), dk.double()))
    close(oq, rq.detach())
    close(ok, rk.detach())
    for got, want in zip(ins, ins64):
        assert got.grad.dtype == bf
        close(got.grad, want.grad)


@pytest.mark.parametrize("packed", [False, True])
def test_llama_qk_norm_cpu(packed):
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    cfg.qk_norm = True
    model = LlamaForCausalLM(cfg)
    ids = torch.randint(0, cfg.vocab_size, (2, 32))
    doc_start = None
    if packed:
        doc_start = torch.zeros(2, 32, dtype=torch.int32)
        doc_start[:, 11:] = 11
    loss = model(ids, ids.clone(), doc_start=doc_start)
    loss.backward()
    assert torch.isfinite(loss)
    keys = model.state_dict().keys()
    for blk_i, blk in enumerate(model.blocks):
        for name in ("q_norm", "k_norm"):
            w = getattr(blk.attn, name).weight
            assert w.shape == (cfg.head_dim,)
            assert w.grad is not None and w.grad.abs().sum() > 0
            assert f"blocks.{blk_i}.attn.{name}.weight" in keys
    plain = LlamaForCausalLM(LlamaConfig.tiny()).state_dict().keys()
    assert not [key for key in plain if "q_norm" in key or "k_norm" in key]


def test_qwen3_preset_and_tp_refusal():
    cfg = LlamaConfig.qwen3_8b()
    assert (cfg.qk_norm, cfg.head_dim, cfg.n_layers) == (True, 128, 36)
    from dlrover_amd.models.llama_parallel import ParallelAttention

    tiny = LlamaConfig.tiny()
    tiny.qk_norm = True
    with pytest.raises(ValueError, match="tensor parallelism"):
        ParallelAttention(tiny, SimpleNamespace(dims=SimpleNamespace(tp=1)))
