"""``moe_grouped_mm(impl="hip")`` and ``LlamaConfig(moe_expert_gemm="hip")``
on the CPU, where the option is a plain loop over the experts."""

import copy
import dataclasses

import pytest
import torch

from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
from dlrover_amd.ops import moe_grouped_mm, moe_router_ref, moe_sort


@pytest.mark.parametrize("gathered", [False, True])
def test_hip_impl_on_cpu_matches_fp64(gathered):
    torch.manual_seed(0)
    T, k, E, K, N = 19, 2, 4, 32, 64
    idx = moe_router_ref(torch.randn(T, E), k)[0]
    offs, row_of_slot, slot_of_row = moe_sort(idx, E)
    x = torch.randn(T, K, requires_grad=True)
    w = torch.randn(E, K, N, requires_grad=True)
    dy = torch.randn(T * k, N)
    src = (slot_of_row // k).long()
    if gathered:
        y = moe_grouped_mm(x, w, offs, impl="hip",
                           gather=(slot_of_row, row_of_slot, k))
    else:
        y = moe_grouped_mm(x[src], w, offs, impl="hip")
    dx, dw = torch.autograd.grad(y, (x, w), dy)

    x64 = x.detach().double().requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    expert = torch.bucketize(torch.arange(T * k), offs.long(), right=True)
    y64 = torch.einsum("rk,rkn->rn", x64[src], w64[expert])
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), dy.double())
    # fp32 sums of at most T*k = 38 terms against fp64
    for got, want in ((y, y64.detach()), (dx, dx64), (dw, dw64)):
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5)


def test_hip_config_trains_like_library_on_cpu():
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=128, intermediate_size=256, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=128, rope_base=10000.0,
        n_experts=4, n_experts_per_tok=2, moe_aux_coef=0.01)
    lib = LlamaForCausalLM(cfg)
    hip = LlamaForCausalLM(dataclasses.replace(cfg, moe_expert_gemm="hip"))
    hip.load_state_dict(copy.deepcopy(lib.state_dict()))
    ids = torch.randint(0, cfg.vocab_size, (2, 32))
    losses = []
    for model in (lib, hip):
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        model(ids, ids.clone()).backward()
        opt.step()
        losses.append(model(ids, ids.clone()).detach())
    # the bounds of test_tiny_moe_model_matches_dense_fp64
    torch.testing.assert_close(losses[1], losses[0], rtol=1e-5, atol=1e-5)


def test_unknown_expert_gemm_raises():
    with pytest.raises(ValueError):
        LlamaConfig(moe_expert_gemm="x")
