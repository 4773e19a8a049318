"""Document-masked flash attention (DOC variant of the v3 kernels) vs the fp32
masked reference. Tolerances are those of tests/test_flash_attn_gpu.py:
outputs rtol=atol=2e-2, gradients rtol=atol=5e-2."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1 / math.sqrt(D)


def _starts(layouts, device="cuda"):
    """int32 doc_start [B, S] from one list of document lengths per row."""
    rows = []
    for lengths in layouts:
        row, at = [], 0
        for n in lengths:
            row += [at] * n
            at += n
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int32, device=device)


def _ref(q, k, v, doc_start):
    """fp32 dense masked softmax, written out here on purpose."""
    B, H, S, _ = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, 1)
    vf = v.float().repeat_interleave(rep, 1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * SCALE
    i = torch.arange(S, device=q.device)[:, None]
    j = torch.arange(S, device=q.device)[None, :]
    visible = (j <= i)[None] & (j[None] >= doc_start.long()[:, :, None])
    s = s.masked_fill(~visible[:, None], float("-inf"))
    return torch.matmul(torch.softmax(s, -1), vf)


def _inputs(B, H, HKV, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def mk(h, shift):
        # asymmetric: non-zero mean, so a wrongly included key shows
        t = torch.randn(B, h, S, D, device="cuda", generator=g) + shift
        return t.to(torch.bfloat16)

    return mk(H, 0.1), mk(HKV, -0.2), mk(HKV, 0.3), mk(H, 0.05)


def _run_both(q, k, v, dout, doc_start):
    """(out, dq, dk, dv) of the kernels and of the fp32 reference."""
    from dlrover_amd.ops import flash_attention

    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    out = flash_attention(*leaves, SCALE, doc_start)
    out.backward(dout)
    ref_leaves = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
    ref = _ref(*ref_leaves, doc_start)
    ref.backward(dout.float())
    got = [out.detach()] + [t.grad for t in leaves]
    want = [ref.detach()] + [t.grad for t in ref_leaves]
    return got, want


def _check(got, want, names=("out", "dq", "dk", "dv")):
    for name, g, w in zip(("out", "dq", "dk", "dv"), got, want):
        if name not in names:
            continue
        tol = 2e-2 if name == "out" else 5e-2
        err = (g.float() - w).abs().max().item()
        print(f"{name}: max abs err {err:.4g}")
        torch.testing.assert_close(g.float(), w, rtol=tol, atol=tol, msg=lambda m, n=name: f"{n}: {m}")


def test_doc_fwd_bwd_mixed_layouts():
    # row 0 (starts 0, 1, 64, 128, 257): a length-1 document, a boundary
    #   inside a 32-row subtile (1), boundaries on 64-tile edges (64, 128), a
    #   document (128..256) straddling the 256-row block edge, so block 1
    #   starts at tile 2 and its rows 257.. meet fully masked leading tiles
    # row 1: block 1 starts at tile 4; kv block 0 stops at q tile 4
    # row 2: a boundary inside a tile and inside block 1
    doc_start = _starts([[1, 63, 64, 129, 255], [256, 256], [300, 212]])
    q, k, v, dout = _inputs(3, 4, 2, 512, seed=0)
    got, want = _run_both(q, k, v, dout, doc_start)
    _check(got, want)


def test_doc_single_document_equals_causal_path():
    from dlrover_amd.ops.api import doc_end_from_start, hip_ops

    q, k, v, dout = _inputs(3, 4, 2, 512, seed=1)
    doc_start = torch.zeros(3, 512, dtype=torch.int32, device="cuda")
    doc_end = doc_end_from_start(doc_start)
    assert bool((doc_end == 512).all())
    out_c, lse_c = hip_ops().flash_attn_fwd(q, k, v, SCALE)
    out_d, lse_d = hip_ops().flash_attn_doc_fwd(q, k, v, SCALE, doc_start)
    assert torch.equal(out_c, out_d)
    assert torch.equal(lse_c, lse_d)
    dq_c, dk_c, dv_c = hip_ops().flash_attn_bwd(q, k, v, out_c, dout, lse_c, SCALE)
    dq_d, dk_d, dv_d = hip_ops().flash_attn_doc_bwd(
        q, k, v, out_d, dout, lse_d, SCALE, doc_start, doc_end)
    assert torch.equal(dq_c, dq_d)
    # the chunked dV/dK path adds with fp32 atomics: order is not fixed
    torch.testing.assert_close(dk_d.float(), dk_c.float(), rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dv_d.float(), dv_c.float(), rtol=5e-2, atol=5e-2)


def test_doc_unchunked_dkv_path():
    # kv_blocks * B * HKV = 4 * 16 * 8 = 512 -> gridDim.y (CH) == 1
    B, H, HKV, S = 16, 8, 8, 1024
    doc_start = _starts([[384, 640]] * B)
    q, k, v, dout = _inputs(B, H, HKV, S, seed=2)
    got, want = _run_both(q, k, v, dout, doc_start)
    _check(got, want, names=("dk", "dv"))


def test_doc_start_out_of_range_is_clamped():
    """Entries outside [0, i] never reach an address: the kernel clamps the
    per-row value into [0, i] and the first tile into the block's range (see
    the DOC prologue of flash_attn_fwd_v3_kernel), so every row keeps its
    diagonal element and stays finite. A batch row that is well-formed
    throughout still comes out right."""
    from dlrover_amd.ops.api import hip_ops

    B, H, HKV, S = 2, 4, 2, 512
    q, k, v, _ = _inputs(B, H, HKV, S, seed=3)
    good = _starts([[200, 312], [512]])
    bad = good.clone()
    bad[1, 0] = -3
    bad[1, 5] = -7
    bad[1, 256] = S + 5  # a block's first row: feeds the first-tile bound
    bad[1, 64:80] = -(2 ** 31)
    bad[1, 300] = S + 5
    bad[1, 400:420] = 2 ** 31 - 1
    out, lse = hip_ops().flash_attn_doc_fwd(q, k, v, SCALE, bad)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    assert bool(torch.isfinite(lse).all())
    ref = _ref(q[:1], k[:1], v[:1], good[:1])
    torch.testing.assert_close(out[:1].float(), ref, rtol=2e-2, atol=2e-2)


def test_doc_model_flash_vs_composite():
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    base = dict(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
    )
    m1 = LlamaForCausalLM(LlamaConfig(**base, attn_impl="flash")).cuda().bfloat16()
    m2 = LlamaForCausalLM(LlamaConfig(**base, attn_impl="composite")).cuda().bfloat16()
    m2.load_state_dict(m1.state_dict())
    ids = torch.randint(0, 512, (2, 256), device="cuda")
    doc_start = _starts([[100, 156]] * 2)
    l1 = m1(ids, ids.clone(), doc_start=doc_start)
    l1.backward()
    l2 = m2(ids, ids.clone(), doc_start=doc_start)
    l2.backward()
    torch.testing.assert_close(l1, l2, rtol=2e-2, atol=2e-2)
    for (n1, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        g1, g2 = p1.grad.float(), p2.grad.float()
        rel = (g1 - g2).norm() / g2.norm().clamp_min(1e-6)
        assert rel < 0.05, (n1, rel.item())


def test_doc_model_activation_checkpointing_sees_doc_start():
    """Recompute in backward must run the same masked attention: loss and
    gradients with block checkpointing equal the ones without (up to the
    order of the fp32 atomics in dK/dV)."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
        attn_impl="flash",
    )
    model = LlamaForCausalLM(cfg).cuda().bfloat16().train()
    ids = torch.randint(0, 512, (2, 256), device="cuda")
    doc_start = _starts([[100, 156], [256]])
    grads = []
    losses = []
    for ckpt in (False, True):
        cfg.activation_checkpointing = ckpt
        model.zero_grad()
        loss = model(ids, ids.clone(), doc_start=doc_start)
        loss.backward()
        losses.append(loss.detach().clone())
        grads.append([p.grad.float().clone() for p in model.parameters()])
    # the forward does not depend on the flag and has no atomics
    torch.testing.assert_close(losses[0], losses[1], rtol=0, atol=1e-5)
    for (name, _), g0, g1 in zip(model.named_parameters(), *grads):
        rel = (g0 - g1).norm() / g0.norm().clamp_min(1e-6)
        # a reordered fp32 sum moves some bf16 results by one ulp (2^-8)
        assert rel < 1e-2, (name, rel.item())


def test_doc_packing_invariance_of_the_kernels():
    from dlrover_amd.ops import flash_attention

    q, k, v, _ = _inputs(2, 4, 2, 512, seed=4)
    doc_start = _starts([[256, 256]] * 2)
    packed = flash_attention(q, k, v, SCALE, doc_start)
    for lo in (0, 256):
        alone = flash_attention(
            q[:, :, lo:lo + 256], k[:, :, lo:lo + 256], v[:, :, lo:lo + 256], SCALE)
        torch.testing.assert_close(
            packed[:, :, lo:lo + 256].float(), alone.float(), rtol=2e-2, atol=2e-2)
    # without the mask the second document sees the first
    causal = flash_attention(q, k, v, SCALE)
    assert (causal[:, :, 256:].float() - packed[:, :, 256:].float()).abs().max() > 5e-2


def test_doc_argument_checks_and_fallback():
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import flash_attention, flash_attention_supports_doc_mask

    base = dict(
        vocab_size=512, hidden_size=512, intermediate_size=1024, n_layers=2,
        n_heads=4, n_kv_heads=2, max_seq_len=256, rope_base=10000.0,
    )
    torch.manual_seed(0)
    flash = LlamaForCausalLM(LlamaConfig(**base, attn_impl="flash")).cuda().bfloat16()
    auto = LlamaForCausalLM(LlamaConfig(**base, attn_impl="auto")).cuda().bfloat16()
    auto.load_state_dict(flash.state_dict())
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    doc_start = _starts([[48, 80], [128]])
    with pytest.raises(ValueError):
        flash(ids, doc_start=doc_start)
    q, k, v, _ = _inputs(2, 4, 2, 128, seed=5)
    assert not flash_attention_supports_doc_mask(q)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, SCALE, doc_start)
    with pytest.raises(RuntimeError):  # the binding's own checks
        from dlrover_amd.ops.api import hip_ops

        hip_ops().flash_attn_doc_fwd(q, k, v, SCALE, doc_start)

    # "auto" falls back to the composite masked softmax: packed documents
    # give the logits of the documents run alone
    with torch.no_grad():
        packed = auto(ids, doc_start=doc_start).float()
        a = auto(ids[:1, :48]).float()
        b = auto(ids[:1, 48:]).float()
        whole = auto(ids[1:]).float()
    torch.testing.assert_close(packed[:1, :48], a, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(packed[:1, 48:], b, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(packed[1:], whole, rtol=2e-2, atol=2e-2)
