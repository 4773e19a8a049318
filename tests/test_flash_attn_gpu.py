"""Flash attention kernels vs the fp32 composite reference (fwd + bwd)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(q, k, v, scale):
    B, H, S, D = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, 1)
    vf = v.float().repeat_interleave(rep, 1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * scale
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1)
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    return torch.matmul(p, vf)


@pytest.mark.parametrize("B,H,HKV,S", [(2, 8, 2, 256), (1, 4, 4, 512), (1, 8, 1, 128)])
def test_flash_fwd_matches_ref(B, H, HKV, S):
    from dlrover_amd.ops.api import hip_ops

    torch.manual_seed(0)
    D = 128
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16)
    out, lse = hip_ops().flash_attn_fwd(q, k, v, 1 / math.sqrt(D))
    ref = _ref(q, k, v, 1 / math.sqrt(D))
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)


def test_flash_bwd_matches_autograd():
    from dlrover_amd.ops import flash_attention

    torch.manual_seed(1)
    B, H, HKV, S, D = 2, 8, 2, 256, 128
    scale = 1 / math.sqrt(D)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    dout = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)

    out = flash_attention(q, k, v, scale)
    out.backward(dout)

    q2 = q.detach().float().requires_grad_(True)
    k2 = k.detach().float().requires_grad_(True)
    v2 = v.detach().float().requires_grad_(True)
    ref = _ref(q2, k2, v2, scale)
    ref.backward(dout.float())

    torch.testing.assert_close(out.float(), ref.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(q.grad.float(), q2.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(k.grad.float(), k2.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(v.grad.float(), v2.grad, rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("S", [64, 192])
def test_flash_16x16_fwd_bwd_matches_ref(S):
    """S % 256 != 0 runs the 16x16 kernels in both directions. S=64 is one
    tile (diagonal only); S=192 is three, so the off-diagonal tiles and the
    running rescale run too. HKV < H: two heads add into one dK/dV."""
    from dlrover_amd.ops import flash_attention

    torch.manual_seed(2)
    B, H, HKV, D = 1, 4, 2, 128
    scale = 1 / math.sqrt(D)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    dout = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)

    out = flash_attention(q, k, v, scale)
    out.backward(dout)

    q2 = q.detach().float().requires_grad_(True)
    k2 = k.detach().float().requires_grad_(True)
    v2 = v.detach().float().requires_grad_(True)
    ref = _ref(q2, k2, v2, scale)
    ref.backward(dout.float())

    torch.testing.assert_close(out.float(), ref.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(q.grad.float(), q2.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(k.grad.float(), k2.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(v.grad.float(), v2.grad, rtol=5e-2, atol=5e-2)


def test_flash_bwd_argument_checks():
    """Every bad argument is refused by a check made before anything is
    allocated or launched."""
    from dlrover_amd.ops.api import hip_ops

    torch.manual_seed(3)
    scale = 1 / math.sqrt(128)

    def mk(B, H, HKV, S, D):
        return (
            torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16),
            torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16),
            torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16),
        )

    q, k, v = mk(1, 4, 2, 64, 128)
    out, lse = hip_ops().flash_attn_fwd(q, k, v, scale)
    dout = torch.randn_like(out)
    assert lse.shape == (1, 4, 64)

    def bwd(q=q, k=k, v=v, out=out, dout=dout, lse=lse):
        return hip_ops().flash_attn_bwd(q, k, v, out, dout, lse, scale)

    # the binding's message for each bad argument: the error must come from
    # its check, not from a kernel that ran on the bad input
    bad = [
        (dict(lse=lse.double()), "lse must be fp32"),
        (dict(lse=lse.transpose(1, 2).contiguous()), r"lse must be contiguous \[B, H, S\]"),
        (dict(dout=torch.randn(1, 4, 128, 128, device="cuda", dtype=torch.bfloat16)),
         "dout must have q's shape"),
        (dict(zip("qkv", mk(1, 4, 2, 64, 64))), "head_dim must be 128"),
        (dict(zip("qkv", mk(1, 4, 2, 96, 128))), "multiple of 64"),
        (dict(zip("qkv", mk(1, 3, 2, 64, 128))), "H % HKV"),
    ]
    for kw, message in bad:
        with pytest.raises(RuntimeError, match=message):
            bwd(**kw)
    torch.cuda.synchronize()
    # the valid arguments still pass
    dq, dk, dv = bwd()
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape


def test_flash_attn_in_model_trains():
    """Tiny-8B-shaped config (D=128) trains with the flash path."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
        attn_impl="flash",
    )
    model = LlamaForCausalLM(cfg).cuda().bfloat16()
    opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.0)
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device="cuda")
    first = last = None
    for _ in range(10):
        loss = model(ids, ids.clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        first = first or loss.item()
        last = loss.item()
    assert last < first * 0.9, (first, last)


def test_model_grads_flash_vs_composite():
    """Full tiny-model (D=128) step: flash and composite attention must give
    the same loss and parameter gradients."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    base = dict(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
    )
    m1 = LlamaForCausalLM(LlamaConfig(**base, attn_impl="flash")).cuda().bfloat16()
    m2 = LlamaForCausalLM(LlamaConfig(**base, attn_impl="composite")).cuda().bfloat16()
    m2.load_state_dict(m1.state_dict())
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    l1 = m1(ids, ids.clone())
    l1.backward()
    l2 = m2(ids, ids.clone())
    l2.backward()
    torch.testing.assert_close(l1, l2, rtol=2e-2, atol=2e-2)
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        g1, g2 = p1.grad.float(), p2.grad.float()
        denom = g2.norm().clamp_min(1e-6)
        rel = (g1 - g2).norm() / denom
        assert rel < 0.05, (n1, rel.item())


def test_fused_residual_stream_matches_plain_forward():
    """GPU fused residual-stream model form == plain per-block form."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=3,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
    )
    model = LlamaForCausalLM(cfg).cuda().bfloat16()
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    loss_fused = model(ids, ids.clone())
    # plain path: run the CPU-structured loop manually on GPU
    pos = torch.arange(128, device="cuda", dtype=torch.int32)
    x = model.embed(ids)
    for blk in model.blocks:
        x = blk(x, pos, model.rope_cos, model.rope_sin)
    x = model.final_norm(x)
    logits = x @ model.lm_head.weight.t()
    ref = torch.nn.functional.cross_entropy(
        logits.float().view(-1, 512), ids.clone().view(-1)
    )
    torch.testing.assert_close(loss_fused.float(), ref, rtol=2e-2, atol=2e-2)


def test_rmsnorm_add_gpu_matches_ref():
    from dlrover_amd.ops import rmsnorm_add

    torch.manual_seed(1)
    x = torch.randn(64, 4096, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    r = torch.randn(64, 4096, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(4096, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    y, h = rmsnorm_add(x, r, w, 1e-5)
    (y.float().pow(2).sum() + h.float().sum() * 0.5).backward()
    x2 = x.detach().float().requires_grad_(True)
    r2 = r.detach().float().requires_grad_(True)
    w2 = w.detach().float().requires_grad_(True)
    h2 = x2 + r2
    inv = torch.rsqrt(h2.pow(2).mean(-1, keepdim=True) + 1e-5)
    y2 = h2 * inv * w2
    (y2.pow(2).sum() + h2.sum() * 0.5).backward()
    torch.testing.assert_close(y.float(), y2, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(x.grad.float(), x2.grad, rtol=5e-2, atol=5e-1)
    torch.testing.assert_close(w.grad.float(), w2.grad, rtol=5e-2, atol=5e-1)


def test_chunked_staging_roundtrip(monkeypatch, tmp_path):
    """The chunked _DeviceStager fallback (payload too big for a device
    staging buffer) must produce a byte-identical snapshot — it drains the
    LIVE tensors synchronously, so mutating them right after save_state_dict
    returns must NOT affect the stored snapshot."""
    import os
    import torch

    monkeypatch.setenv("DLROVER_CKPT_FORCE_CHUNKED", "1")
    from dlrover_amd.trainer.flash_checkpoint.shm_handler import (
        SharedMemoryHandler,
    )

    h = SharedMemoryHandler(f"test_chunked_{os.getpid()}")
    try:
        t1 = torch.randn(3 << 20, device="cuda")
        t2 = torch.randn(1000, device="cuda", dtype=torch.bfloat16)
        sd = {"a": t1, "b": {"c": t2}, "step": 5}
        want1, want2 = t1.clone(), t2.clone()
        blocking = h.save_state_dict(5, sd, block=False)
        # chunked mode is synchronous: mutations after return are not seen
        t1.add_(100.0)
        t2.add_(7.0)
        h.wait_drained()
        out = h.load_state_dict(device=torch.device("cuda:0"))
        assert out["step"] == 5
        torch.testing.assert_close(out["a"], want1)
        torch.testing.assert_close(out["b"]["c"], want2)
        assert blocking > 0
    finally:
        h.unlink()


def test_fsdp_dtensor_ckpt_roundtrip_gpu(tmp_path, monkeypatch):
    """The sharded (DTensor) checkpoint path on REAL hardware: fully_shard
    over a 1-rank device mesh still produces DTensor params, so this covers
    exactly what the driver's multi-GPU scale run does per rank — gather
    local shards to shm, restore into live DTensor storage."""
    import os

    import torch
    import torch.distributed as dist

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29581")
    monkeypatch.setenv("ELASTIC_JOB_NAME", f"fsdpgpu{os.getpid()}")
    dist.init_process_group(
        "nccl", rank=0, world_size=1, device_id=torch.device("cuda:0")
    )
    try:
        from torch.distributed.fsdp import fully_shard
        from torch.distributed.tensor import DTensor

        from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
        from dlrover_amd.ops import FusedAdamW
        from dlrover_amd.trainer.flash_checkpoint import FsdpShardCheckpointer

        torch.manual_seed(0)
        cfg = LlamaConfig.tiny()
        model = LlamaForCausalLM(cfg).cuda().bfloat16()
        model.rope_cos = model.rope_cos.float()
        model.rope_sin = model.rope_sin.float()
        for blk in model.blocks:
            fully_shard(blk)
        fully_shard(model)
        assert isinstance(next(model.parameters()), DTensor)
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
        ids = torch.randint(0, cfg.vocab_size, (2, 32), device="cuda")
        model(ids, ids.clone()).backward()
        opt.step()
        opt.zero_grad()

        cp = FsdpShardCheckpointer(str(tmp_path / "ckpt"), model, opt)
        from dlrover_amd.trainer.flash_checkpoint import StorageType

        cp.save_checkpoint(3, storage_type=StorageType.MEMORY)
        cp.engine.wait_saving()
        name, p = next(iter(model.named_parameters()))
        want = p.to_local().clone()
        with torch.no_grad():
            p.to_local().add_(1.0)
        out = cp.engine.restore_into(model, opt)
        assert out is not None and out.get("step") == 3
        # the bf16 params were OMITTED from the snapshot (derived-ckpt,
        # default on) — this equality only holds if the device rederive
        # from the restored fp32 master actually ran
        assert out.get("_derived"), "snapshot did not use derived-ckpt"
        assert name in out["_derived"]
        torch.testing.assert_close(p.to_local(), want)
        # training continues after restore
        model(ids, ids.clone()).backward()
        opt.step()
        torch.cuda.synchronize()
        cp.close()
        cp.engine.shm_handler.unlink()
    finally:
        dist.destroy_process_group()
