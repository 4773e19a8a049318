"""Document masking for packed sequences: helpers, CPU references, model."""

import math

import pytest
import torch

from dlrover_amd.ops import (
    doc_end_from_start,
    doc_positions,
    doc_start_from_eos,
    doc_start_from_ids,
    flash_attention,
    flash_attention_ref,
    rope_ref,
    validate_doc_start,
)
from dlrover_amd.ops.api import build_rope_cache


def _layout(lengths):
    """(doc_ids, tokens with EOS = 0 closing every document, doc_start)."""
    ids, toks, start = [], [], []
    at = 0
    for d, n in enumerate(lengths):
        ids += [7 + 3 * d] * n
        toks += [5] * (n - 1) + [0]
        start += [at] * n
        at += n
    return (torch.tensor([ids]), torch.tensor([toks]),
            torch.tensor([start], dtype=torch.int32))


def test_helpers_agree_on_a_layout():
    ids, toks, want = _layout([1, 5, 2, 8])
    a = doc_start_from_ids(ids, validate=True)
    b = doc_start_from_eos(toks, eos_id=0, validate=True)
    assert a.dtype == torch.int32 and a.shape == want.shape
    assert torch.equal(a, want) and torch.equal(b, want)
    pos = doc_positions(want)
    assert pos.dtype == torch.int32
    assert pos[0].tolist() == [0, 0, 1, 2, 3, 4, 0, 1, 0, 1, 2, 3, 4, 5, 6, 7]
    end = doc_end_from_start(want)
    assert end[0].tolist() == [1] + [6] * 5 + [8] * 2 + [16] * 8


def test_helpers_batched_rows_differ():
    ids = torch.tensor([[1, 1, 2, 2, 2, 3], [4, 4, 4, 4, 4, 4]])
    got = doc_start_from_ids(ids)
    assert got.tolist() == [[0, 0, 2, 2, 2, 5], [0] * 6]
    assert doc_end_from_start(got).tolist() == [[2, 2, 5, 5, 5, 6], [6] * 6]


def test_eos_in_last_position_and_single_document():
    toks = torch.tensor([[5, 5, 0, 5, 5, 0]])
    assert doc_start_from_eos(toks, 0).tolist() == [[0, 0, 0, 3, 3, 3]]
    one = torch.full((2, 9), 5)
    assert torch.equal(doc_start_from_eos(one, 0),
                       torch.zeros(2, 9, dtype=torch.int32))
    assert torch.equal(doc_start_from_ids(one, validate=True),
                       torch.zeros(2, 9, dtype=torch.int32))


def test_validate_rejects_malformed():
    validate_doc_start(torch.tensor([[0, 0, 2, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):  # decreasing
        validate_doc_start(torch.tensor([[0, 1, 0, 3]], dtype=torch.int32))
    with pytest.raises(ValueError):  # doc_start[i] > i
        validate_doc_start(torch.tensor([[0, 2, 2, 3]], dtype=torch.int32))
    with pytest.raises(ValueError):  # negative
        validate_doc_start(torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32))
    with pytest.raises(ValueError):  # start that is not a document's first token
        validate_doc_start(torch.tensor([[0, 0, 1, 1]], dtype=torch.int32))


def _dense_doc_attention(q, k, v, scale, doc_start):
    """Independent reference: explicit boolean visibility, row by row rules."""
    B, H, S, D = q.shape
    rep = H // k.shape[1]
    out = torch.zeros(B, H, S, D, dtype=q.dtype)
    for b in range(B):
        i = torch.arange(S)[:, None]
        j = torch.arange(S)[None, :]
        visible = (j <= i) & (j >= doc_start[b].long()[:, None])
        for h in range(H):
            s = (q[b, h] @ k[b, h // rep].T) * scale
            s = torch.where(visible, s, torch.full_like(s, -float("inf")))
            out[b, h] = torch.softmax(s, -1) @ v[b, h // rep]
    return out


def test_attention_ref_and_autograd_match_dense_masked_softmax():
    torch.manual_seed(0)
    B, H, HKV, S, D = 2, 4, 2, 24, 16
    scale = 1 / math.sqrt(D)
    doc_start = torch.stack([
        _layout([1, 7, 16])[2][0], _layout([10, 14])[2][0]])
    q = torch.randn(B, H, S, D)
    k = torch.randn(B, HKV, S, D)
    v = torch.randn(B, HKV, S, D)
    want = _dense_doc_attention(q, k, v, scale, doc_start)
    got = flash_attention_ref(q, k, v, scale, doc_start)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-5)
    # the mask matters: the causal reference differs
    assert (flash_attention_ref(q, k, v, scale) - want).abs().max() > 1e-2

    dout = torch.randn(B, H, S, D)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    flash_attention(*leaves, scale, doc_start).backward(dout)
    ref_leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    _dense_doc_attention(*ref_leaves, scale, doc_start).backward(dout)
    for a, b in zip(leaves, ref_leaves):
        torch.testing.assert_close(a.grad, b.grad, rtol=0, atol=1e-5)


def test_rope_ref_2d_positions_match_per_batch_calls():
    torch.manual_seed(1)
    B, S, NH, D = 3, 10, 2, 8
    cos, sin = build_rope_cache(32, D, 10000.0)
    x = torch.randn(B, S, NH, D)
    pos = torch.stack([torch.randperm(32)[:S] for _ in range(B)]).int()
    want = torch.stack([rope_ref(x[b], pos[b], cos, sin) for b in range(B)])
    torch.testing.assert_close(rope_ref(x, pos, cos, sin), want, rtol=0, atol=0)
    torch.testing.assert_close(rope_ref(x, pos.reshape(-1), cos, sin), want,
                               rtol=0, atol=0)
    # 1-D shared positions: unchanged
    shared = torch.arange(S, dtype=torch.int32)
    want1 = torch.stack([rope_ref(x[b], shared, cos, sin) for b in range(B)])
    torch.testing.assert_close(rope_ref(x, shared, cos, sin), want1, rtol=0, atol=0)


@pytest.mark.parametrize("ckpt", [False, True])
def test_packing_invariance_of_the_model(ckpt):
    """[docA | docB] with doc_start == docA and docB run alone."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    cfg.activation_checkpointing = ckpt
    model = LlamaForCausalLM(cfg).float()
    model.train(ckpt)  # checkpointing is a training-mode path
    la, lb = 40, 24
    a = torch.randint(0, cfg.vocab_size, (1, la))
    b = torch.randint(0, cfg.vocab_size, (1, lb))
    packed = torch.cat([a, b], dim=1)
    doc_start = torch.tensor([[0] * la + [la] * lb], dtype=torch.int32)

    alone_a, alone_b = model(a), model(b)
    with_mask = model(packed, doc_start=doc_start)
    torch.testing.assert_close(with_mask[:, :la], alone_a, rtol=0, atol=1e-4)
    torch.testing.assert_close(with_mask[:, la:], alone_b, rtol=0, atol=1e-4)

    without = model(packed)
    torch.testing.assert_close(without[:, :la], alone_a, rtol=0, atol=1e-4)
    assert (without[:, la:] - alone_b).abs().max() > 1e-2

    if ckpt:  # recompute sees doc_start: gradients flow and match no-ckpt
        labels = packed.clone()
        model.zero_grad()
        model(packed, labels, doc_start=doc_start).backward()
        g1 = [p.grad.clone() for p in model.parameters()]
        model.cfg.activation_checkpointing = False
        model.zero_grad()
        model(packed, labels, doc_start=doc_start).backward()
        for x, p in zip(g1, model.parameters()):
            torch.testing.assert_close(x, p.grad, rtol=0, atol=1e-6)
