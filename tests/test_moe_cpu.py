"""Mixture-of-experts layers on the CPU reference path: the routing rule of
``moe_router_ref`` and a tiny MoE ``LlamaForCausalLM`` against a dense,
loop-over-experts fp64 evaluation of the same weights."""

import copy
import types

import pytest
import torch
import torch.nn.functional as F

from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
from dlrover_amd.ops import moe_router_ref


@pytest.mark.parametrize("norm_topk", [True, False])
def test_router_ref_tie_rule(norm_topk):
    """Equal logits go to the lower expert; slots descend by logit."""
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0],
                           [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                           [-1.0, 5.0, 2.0, 2.0, 7.0, 2.0]])
    idx, w, pm = moe_router_ref(logits, 3, norm_topk)
    assert idx.tolist() == [[1, 2, 4], [0, 1, 2], [4, 1, 2]]
    p = torch.softmax(logits, -1)
    want = p.gather(1, idx.long())
    if norm_topk:
        want = want / want.sum(-1, keepdim=True)
        torch.testing.assert_close(w.sum(-1), torch.ones(3))
    torch.testing.assert_close(w, want)
    torch.testing.assert_close(pm, p.mean(0))


def dense_moe_fp64(self, x):
    """MoEMLP.forward without routing machinery: every expert runs on every
    token in fp64 and a [T, E] gate matrix weights the results."""
    cfg = self.cfg
    E, k = cfg.n_experts, cfg.n_experts_per_tok
    xf = x.reshape(-1, x.shape[-1]).double()
    p = torch.softmax(xf @ self.router.weight.double().t(), -1)
    top = torch.topk(p, k, dim=-1)  # no ties among random logits
    gate = torch.zeros_like(p).scatter(
        1, top.indices, top.values / top.values.sum(-1, keepdim=True))
    y = torch.zeros_like(xf)
    for e in range(E):
        g, u = (xf @ self.experts_gate_up[e].double()).chunk(2, -1)
        y = y + gate[:, e:e + 1] * ((F.silu(g) * u) @ self.experts_down[e].double())
    f = (gate > 0).sum(0).double() / (xf.shape[0] * k)
    aux = E * (f * p.mean(0)).sum()
    return y.to(x.dtype).view(x.shape), aux.to(x.dtype)


def test_tiny_moe_model_matches_dense_fp64():
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=128, intermediate_size=256, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=128, rope_base=10000.0,
        n_experts=4, n_experts_per_tok=2, moe_aux_coef=0.01)
    model = LlamaForCausalLM(cfg)
    dense = copy.deepcopy(model)
    for blk in dense.blocks:
        blk.mlp.forward = types.MethodType(dense_moe_fp64, blk.mlp)
    ids = torch.randint(0, cfg.vocab_size, (2, 32))
    losses = []
    for m in (model, dense):
        loss = m(ids, ids.clone())
        loss.backward()
        losses.append(loss)
    # fp32 against fp64 through two layers: a few hundred roundings of 2^-24
    torch.testing.assert_close(losses[0], losses[1], rtol=1e-5, atol=1e-5)
    grads = dict(dense.named_parameters())
    for name, p in model.named_parameters():
        if not any(s in name for s in ("router", "experts", "embed")):
            continue
        want = grads[name].grad
        assert want.abs().max() > 0, name
        torch.testing.assert_close(
            p.grad, want, rtol=1e-4, atol=1e-5 * want.abs().max().item(),
            msg=lambda m, name=name: f"{name}: {m}")


def test_dense_config_is_unchanged_and_moe_rejects_fp8():
    cfg = LlamaConfig.tiny()
    assert cfg.n_experts == 0
    per_block = ["attn_norm.weight", "attn.qkv_proj.weight",
                 "attn.o_proj.weight", "mlp_norm.weight",
                 "mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
    want = ["embed.weight"] + [
        f"blocks.{i}.{n}" for i in range(cfg.n_layers) for n in per_block
    ] + ["final_norm.weight", "lm_head.weight"]
    assert list(LlamaForCausalLM(cfg).state_dict()) == want
    moe = LlamaForCausalLM(LlamaConfig(
        vocab_size=64, hidden_size=32, intermediate_size=64, n_layers=1,
        n_heads=2, n_kv_heads=1, max_seq_len=16, n_experts=4,
        moe_intermediate_size=16))
    shapes = {k: tuple(v.shape) for k, v in moe.state_dict().items()}
    assert shapes["blocks.0.mlp.router.weight"] == (4, 32)
    assert shapes["blocks.0.mlp.experts_gate_up"] == (4, 32, 32)
    assert shapes["blocks.0.mlp.experts_down"] == (4, 16, 32)
    with pytest.raises(ValueError):
        LlamaConfig(n_experts=8, linear_precision="fp8")
    with pytest.raises(ValueError):
        LlamaConfig(n_experts=4, n_experts_per_tok=5)
