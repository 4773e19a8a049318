"""Autograd-wrapped ops: HIP kernels on GPU, torch fp32 references on CPU."""

from typing import Optional, Tuple

import torch

_EXT = None
_EXT_ERR: Optional[str] = None


class ExtensionMissingError(RuntimeError):
    pass


def hip_ops():
    """Return the compiled extension, importing it lazily. Raises loudly on a
    GPU box if the .so is missing (the driver checks native code is loaded)."""
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from dlrover_amd.ops import _hip_ops as ext  # built in-tree

            _EXT = ext
        except ImportError as e:  # pragma: no cover - build problem
            _EXT_ERR = str(e)
    if _EXT is None:
        raise ExtensionMissingError(
            "dlrover_amd._hip_ops is not built — run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            f"(import error: {_EXT_ERR})"
        )
    return _EXT


def hip_ops_available() -> bool:
    try:
        hip_ops()
        return True
    except ExtensionMissingError:
        return False


def _use_hip(*tensors: torch.Tensor) -> bool:
    on_gpu = any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))
    if on_gpu:
        hip_ops()  # raises if missing: no silent eager fallback on GPU
        return True
    return False


# ---------------------------------------------------------------------------
# reference implementations (CPU path + GPU numerics oracle)
# ---------------------------------------------------------------------------


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def swiglu_ref(gate_up: torch.Tensor) -> torch.Tensor:
    gate, up = gate_up.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(gate) * up).to(gate_up.dtype)


def rope_ref(
    x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor
) -> torch.Tensor:
    """x [..., n_tokens, n_heads, D]; cos/sin [max_pos, D/2] fp32. pos is
    [n_tokens] (one vector shared by every leading index), or one position
    per token of x: [B, S] for x [B, S, n_heads, D], or the same flattened to
    [B*S] (the form the HIP kernel takes)."""
    d = x.shape[-1]
    xf = x.float()
    x1, x2 = xf[..., : d // 2], xf[..., d // 2 :]
    if pos.dim() == 1 and (x.dim() < 3 or pos.numel() == x.shape[-3]):
        shape = [1] * (x.dim() - 3) + [-1, 1, d // 2]
    else:
        shape = list(x.shape[:-2]) + [1, d // 2]
        pos = pos.reshape(-1)
    c = cos[pos].view(*shape)
    s = sin[pos].view(*shape)
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


def causal_softmax_ref(
    scores: torch.Tensor, scale: float, q_offset: int = 0, q_len: int = 0
) -> torch.Tensor:
    s = scores.float() * scale
    n_rows, k_len = s.shape[-2], s.shape[-1]
    q_len = q_len or n_rows
    # row r is query position (r % q_len) — supports the GQA grouped layout
    # where rep query-head blocks are folded into the row dimension
    qpos = (torch.arange(n_rows, device=s.device) % q_len).unsqueeze(-1) + q_offset
    kpos = torch.arange(k_len, device=s.device).unsqueeze(0)
    s = s.masked_fill(kpos > qpos, float("-inf"))
    return torch.softmax(s, dim=-1).to(scores.dtype)


# ---------------------------------------------------------------------------
# autograd functions
# ---------------------------------------------------------------------------


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        if _use_hip(x):
            y, invrms = hip_ops().rmsnorm_fwd(x.contiguous(), w.contiguous(), eps)
            ctx.save_for_backward(x, w, invrms)
            ctx.use_hip = True
        else:
            xf = x.float()
            invrms = torch.rsqrt(xf.pow(2).mean(-1) + eps).reshape(-1)
            y = rmsnorm_ref(x, w, eps)
            ctx.save_for_backward(x, w, invrms)
            ctx.use_hip = False
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, invrms = ctx.saved_tensors
        if ctx.use_hip:
            dx, dw = hip_ops().rmsnorm_bwd(dy.contiguous(), x, w, invrms, None)
            return dx, dw, None
        h = x.shape[-1]
        xf, dyf, wf = x.float(), dy.float(), w.float()
        inv = invrms.view(*x.shape[:-1], 1)
        dot = (dyf * wf * xf).sum(-1, keepdim=True)
        dx = dyf * wf * inv - xf * (dot * inv.pow(3) / h)
        dw = (dyf * xf * inv).reshape(-1, h).sum(0)
        return dx.to(x.dtype), dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNorm.apply(x, w, eps)


class _RMSNormAdd(torch.autograd.Function):
    """Fused h = x + resid; y = rmsnorm(h) * w. Two outputs: (y, h) — h is
    the continuing residual stream, so its incoming gradient folds into the
    norm backward in the same kernel pass."""

    @staticmethod
    def forward(ctx, x, resid, w, eps):
        if _use_hip(x):
            h, y, invrms = hip_ops().rmsnorm_add_fwd(
                x.contiguous(), resid.contiguous(), w.contiguous(), eps
            )
            ctx.save_for_backward(h, w, invrms)
            ctx.use_hip = True
            return y, h
        hf = x.float() + resid.float()
        invrms = torch.rsqrt(hf.pow(2).mean(-1) + eps).reshape(-1)
        h = hf.to(x.dtype)
        y = rmsnorm_ref(h, w, eps)
        ctx.save_for_backward(h, w, invrms)
        ctx.use_hip = False
        return y, h

    @staticmethod
    def backward(ctx, dy, dh):
        h, w, invrms = ctx.saved_tensors
        if ctx.use_hip:
            dh_c = dh.contiguous() if dh is not None else None
            dx, dw = hip_ops().rmsnorm_bwd(dy.contiguous(), h, w, invrms, dh_c)
            return dx, dx, dw, None
        hid = h.shape[-1]
        hf, dyf, wf = h.float(), dy.float(), w.float()
        inv = invrms.view(*h.shape[:-1], 1)
        dot = (dyf * wf * hf).sum(-1, keepdim=True)
        dxf = dyf * wf * inv - hf * (dot * inv.pow(3) / hid)
        if dh is not None:
            dxf = dxf + dh.float()
        dw = (dyf * hf * inv).reshape(-1, hid).sum(0)
        dx = dxf.to(h.dtype)
        return dx, dx, dw.to(w.dtype), None


def rmsnorm_add(x: torch.Tensor, resid: torch.Tensor, w: torch.Tensor,
                eps: float = 1e-5):
    """(normed, new_residual) = fused residual-add + RMSNorm."""
    return _RMSNormAdd.apply(x, resid, w, eps)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up):
        ctx.save_for_backward(gate_up)
        if _use_hip(gate_up):
            return hip_ops().swiglu_fwd(gate_up.contiguous())
        return swiglu_ref(gate_up)

    @staticmethod
    def backward(ctx, dy):
        (gate_up,) = ctx.saved_tensors
        if _use_hip(gate_up):
            return hip_ops().swiglu_bwd(dy.contiguous(), gate_up.contiguous())
        gate, up = gate_up.float().chunk(2, dim=-1)
        sig = torch.sigmoid(gate)
        dyf = dy.float()
        dg = dyf * up * sig * (1 + gate * (1 - sig))
        du = dyf * gate * sig
        return torch.cat([dg, du], dim=-1).to(gate_up.dtype)


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """out = silu(gate_up[..., :I]) * gate_up[..., I:]"""
    return _SwiGLU.apply(gate_up)


def _rope_addressable(x: torch.Tensor) -> torch.Tensor:
    """The oop rope kernel addresses [tokens(strided), heads, head_dim] with
    heads*head_dim contiguous and a uniform token stride; anything else
    (rare) goes through one contiguous copy."""
    hd = x.size(-1)
    if x.stride(-1) != 1 or x.stride(-2) != hd:
        return x.contiguous()
    if x.dim() >= 3:
        tok_stride = x.stride(-3)
        rows = x.size(-3)
        for d in range(x.dim() - 4, -1, -1):
            if x.stride(d) != rows * tok_stride:
                return x.contiguous()
            rows *= x.size(d)
    return x


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, cos, sin):
        ctx.save_for_backward(pos, cos, sin)
        if _use_hip(x):
            # out-of-place kernel reads the strided view (e.g. a q/k slice
            # of the fused QKV projection) directly — no clone pass
            return hip_ops().rope_rotate_oop(
                _rope_addressable(x), pos.int(), cos, sin, False
            )
        return rope_ref(x, pos, cos, sin)

    @staticmethod
    def backward(ctx, dy):
        pos, cos, sin = ctx.saved_tensors
        if _use_hip(dy):
            dx = hip_ops().rope_rotate_oop(
                _rope_addressable(dy), pos.int(), cos, sin, True
            )
            return dx, None, None, None
        # inverse rotation
        return rope_ref(dy, pos, cos, -sin), None, None, None


def rope_rotate(
    x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor
) -> torch.Tensor:
    """Apply rotate-half RoPE. x: [..., n_tokens, n_heads, head_dim]."""
    return _RoPE.apply(x, pos, cos, sin)


def build_rope_cache(
    max_pos: int, head_dim: int, base: float = 500000.0, device="cpu"
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-precomputed fp32 cos/sin tables [max_pos, head_dim/2]
    (on-device trig would turn RoPE VALU-bound — guide Appendix B)."""
    inv_freq = 1.0 / (
        base ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim)
    )
    t = torch.arange(max_pos, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)
    return freqs.cos().to(device), freqs.sin().to(device)


class _CausalSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, scale, q_offset, q_len):
        q_len = q_len or scores.shape[-2]
        if _use_hip(scores):
            probs = scores.contiguous()
            hip_ops().causal_softmax_fwd(probs, q_len, q_offset, scale)
        else:
            probs = causal_softmax_ref(scores, scale, q_offset, q_len)
        ctx.save_for_backward(probs)
        ctx.scale = scale
        return probs

    @staticmethod
    def backward(ctx, dprobs):
        (probs,) = ctx.saved_tensors
        if _use_hip(probs):
            ds = dprobs.contiguous().clone()
            hip_ops().causal_softmax_bwd(ds, probs, ctx.scale)
            return ds, None, None, None
        pf, df = probs.float(), dprobs.float()
        dot = (pf * df).sum(-1, keepdim=True)
        return (pf * (df - dot) * ctx.scale).to(probs.dtype), None, None, None


def causal_softmax(
    scores: torch.Tensor, scale: float, q_offset: int = 0, q_len: int = 0
) -> torch.Tensor:
    """In one fused pass: probs = softmax(scale * scores + causal_mask).

    q_len: the true sequence length when rows fold multiple query-head
    blocks (GQA grouped layout) — row r is query position r % q_len.
    NOTE (GPU path): consumes ``scores`` in place — do not reuse it.
    """
    return _CausalSoftmax.apply(scores, scale, q_offset, q_len)


# ---------------------------------------------------------------------------
# document masks for packed sequences
#
# One int32 tensor doc_start[B, S]: entry [b, i] is the index of the first
# token of the document that holds position i. Invariants: non-decreasing
# along i, 0 <= doc_start[b, i] <= i, and constant within a document
# (doc_start[b, doc_start[b, i]] == doc_start[b, i]). Query i attends key j
# iff doc_start[b, i] <= j <= i, so every row sees at least itself.
# ---------------------------------------------------------------------------


def validate_doc_start(doc_start: torch.Tensor) -> None:
    """Raise ValueError unless doc_start [B, S] keeps the invariants above.
    Reads the answer on the host: one device sync."""
    if doc_start.dim() != 2:
        raise ValueError("doc_start must be [B, S]")
    ds = doc_start.long()
    S = ds.shape[1]
    idx = torch.arange(S, device=ds.device).expand_as(ds)
    in_range = (ds >= 0) & (ds <= idx)
    monotone = ds[:, 1:] >= ds[:, :-1]
    # a document starts where its start points (gather only at clamped indices)
    own = ds.gather(1, ds.clamp(0, S - 1)) == ds
    ok = torch.stack([in_range.all(), monotone.all(), own.all()]).tolist()
    if not ok[0]:
        raise ValueError("doc_start: need 0 <= doc_start[b, i] <= i")
    if not ok[1]:
        raise ValueError("doc_start: must be non-decreasing along the sequence")
    if not ok[2]:
        raise ValueError("doc_start: must point at the first token of a document")


def _doc_start_from_new(new: torch.Tensor, validate: bool) -> torch.Tensor:
    """new [B, S] bool, True where a document begins (column 0 always does)."""
    S = new.shape[1]
    idx = torch.arange(S, device=new.device, dtype=torch.int32).expand_as(new)
    start = torch.where(new, idx, torch.zeros_like(idx))
    out = torch.cummax(start, dim=1).values.contiguous()
    if validate:
        validate_doc_start(out)
    return out


def doc_start_from_ids(doc_ids: torch.Tensor, validate: bool = False) -> torch.Tensor:
    """doc_start [B, S] (int32) from per-token document ids [B, S]: a new
    document begins wherever the id changes. Pure torch, no host sync unless
    ``validate``."""
    new = torch.ones_like(doc_ids, dtype=torch.bool)
    new[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    return _doc_start_from_new(new, validate)


def doc_start_from_eos(
    tokens: torch.Tensor, eos_id: int, validate: bool = False
) -> torch.Tensor:
    """doc_start [B, S] (int32) from token ids [B, S]: an EOS token ends its
    document and the next token starts a new one (an EOS in the last position
    starts nothing). Pure torch, no host sync unless ``validate``."""
    new = torch.ones_like(tokens, dtype=torch.bool)
    new[:, 1:] = tokens[:, :-1] == eos_id
    return _doc_start_from_new(new, validate)


def doc_positions(doc_start: torch.Tensor) -> torch.Tensor:
    """Position of every token inside its own document: arange(S) - doc_start,
    int32 [B, S] — the RoPE positions of a packed batch."""
    S = doc_start.shape[1]
    idx = torch.arange(S, device=doc_start.device, dtype=torch.int32)
    return (idx - doc_start.int()).contiguous()


def doc_end_from_start(doc_start: torch.Tensor) -> torch.Tensor:
    """doc_end [B, S] (int32): the exclusive end of the document holding each
    position, i.e. the next larger doc_start value, or S. Key j is visible to
    exactly the queries j <= i < doc_end[b, j] — the bound the kv-major
    backward kernels need. Torch ops on doc_start's device, no host sync."""
    ds = doc_start.int()
    B, S = ds.shape
    idx = torch.arange(S, device=ds.device, dtype=torch.int32).expand(B, S)
    # where a document begins its start is its own index; elsewhere "none yet"
    nxt = torch.where(ds == idx, idx, torch.full_like(idx, S))
    # doc_end[i] = min over j > i of nxt[j] (or S): a reversed running minimum
    shifted = torch.cat([nxt[:, 1:], torch.full_like(idx[:, :1], S)], dim=1)
    return torch.cummin(shifted.flip(1), dim=1).values.flip(1).contiguous()


def flash_attention_supports_doc_mask(q: torch.Tensor) -> bool:
    """True when the document-masked HIP kernels can take q [B,H,S,D]: on the
    GPU, D == 128 and S % 256 == 0 (the 32x32-MFMA kernels' shapes)."""
    return bool(q.is_cuda and q.shape[-1] == 128 and q.shape[-2] % 256 == 0)


def flash_attention_ref(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: float,
    doc_start: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """fp32 composite reference: q [B,H,S,D], k/v [B,HKV,S,D], causal; with
    doc_start [B,S] additionally restricted to the query's own document."""
    B, H, S, D = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, 1)
    vf = v.float().repeat_interleave(rep, 1)
    s_ = torch.matmul(q.float(), kf.transpose(-1, -2)) * scale
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1)
    if doc_start is not None:
        kpos = torch.arange(S, device=q.device)
        # [B, 1, S(q), S(k)]: keys before the query's document
        mask = mask | (kpos[None, None, None, :] < doc_start.long()[:, None, :, None])
    s_ = s_.masked_fill(mask, float("-inf"))
    p = torch.softmax(s_, -1)
    return torch.matmul(p, vf).to(q.dtype)


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, doc_start=None):
        ctx.has_doc = doc_start is not None
        if _use_hip(q):
            # strided [B,H,S,D] views are fine (kernels are stride-aware);
            # only the head dim must be contiguous
            if q.stride(-1) != 1:
                q = q.contiguous()
            if k.stride(-1) != 1:
                k = k.contiguous()
            if v.stride(-1) != 1:
                v = v.contiguous()
            if doc_start is not None:
                if not flash_attention_supports_doc_mask(q):
                    raise ValueError(
                        "flash_attention: doc_start needs D == 128 and "
                        f"S % 256 == 0 on the GPU, got D={q.shape[-1]} "
                        f"S={q.shape[-2]}"
                    )
                ds = doc_start.to(device=q.device, dtype=torch.int32).contiguous()
                de = doc_end_from_start(ds)
                out, lse = hip_ops().flash_attn_doc_fwd(q, k, v, scale, ds)
                ctx.save_for_backward(q, k, v, out, lse, ds, de)
            else:
                out, lse = hip_ops().flash_attn_fwd(q, k, v, scale)
                ctx.save_for_backward(q, k, v, out, lse)
            ctx.scale = scale
            ctx.use_hip = True
            return out
        ctx.use_hip = False
        q32 = q.detach().clone().requires_grad_(True)
        k32 = k.detach().clone().requires_grad_(True)
        v32 = v.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            out = flash_attention_ref(q32, k32, v32, scale, doc_start)
        ctx.saved_ref = (q32, k32, v32, out)
        return out.detach()

    @staticmethod
    def backward(ctx, dout):
        if ctx.use_hip:
            if ctx.has_doc:
                q, k, v, out, lse, ds, de = ctx.saved_tensors
                dq, dk, dv = hip_ops().flash_attn_doc_bwd(
                    q, k, v, out, dout.contiguous(), lse, ctx.scale, ds, de
                )
                return dq, dk, dv, None, None
            q, k, v, out, lse = ctx.saved_tensors
            dq, dk, dv = hip_ops().flash_attn_bwd(
                q, k, v, out, dout.contiguous(), lse, ctx.scale
            )
            return dq, dk, dv, None, None
        q32, k32, v32, out = ctx.saved_ref
        torch.autograd.backward(out, dout)
        return q32.grad, k32.grad, v32.grad, None, None


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: float,
    doc_start: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fused causal GQA attention. q [B,H,S,D], k/v [B,HKV,S,D], D=128,
    S % 64 == 0. Never materializes the S^2 score matrix (hand-written MFMA
    kernels, ops/csrc/attention*.hip).

    doc_start [B,S] (int32, see ``doc_start_from_ids`` / ``_from_eos``) adds
    the document mask of packed sequences: query i attends key j iff
    doc_start[b,i] <= j <= i. On the GPU that is the DOC variant of the v3
    kernels (D == 128, S % 256 == 0 — ``flash_attention_supports_doc_mask``;
    other shapes raise ValueError), which also skips the K/V tiles outside a
    block's documents. ``None`` is the causal path, unchanged."""
    if doc_start is None:
        return _FlashAttention.apply(q, k, v, scale)
    return _FlashAttention.apply(q, k, v, scale, doc_start)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        n_valid = int((targets != ignore_index).sum())
        grad_scale = 1.0 / max(n_valid, 1)
        if _use_hip(logits):
            work = logits.contiguous()
            losses = hip_ops().cross_entropy_fwd_bwd(
                work, targets.int(), ignore_index, grad_scale, True
            )
            ctx.save_for_backward(work)  # now holds dlogits (pre-scaled)
            ctx.use_hip = True
        else:
            lf = logits.float()
            losses = torch.nn.functional.cross_entropy(
                lf.view(-1, lf.shape[-1]),
                targets.view(-1).long(),
                ignore_index=ignore_index,
                reduction="none",
            )
            dl = torch.softmax(lf, dim=-1)
            t = targets.view(-1)
            valid = t != ignore_index
            onehot = torch.zeros_like(dl.view(-1, dl.shape[-1]))
            onehot[valid, t[valid].long()] = 1.0
            dl = (dl.view(-1, dl.shape[-1]) - onehot) * grad_scale
            dl[~valid] = 0
            ctx.save_for_backward(dl.to(logits.dtype).view_as(logits))
            ctx.use_hip = False
        ctx.n_valid = n_valid
        return losses.sum() * grad_scale

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None, None


def cross_entropy_loss(
    logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100
) -> torch.Tensor:
    """Mean CE over non-ignored tokens. GPU path fuses loss+grad in one
    kernel and reuses the logits buffer for dlogits (no extra V-sized
    allocation). The logits tensor is consumed."""
    return _CrossEntropy.apply(logits, targets, ignore_index)


# ---------------------------------------------------------------------------
# vocab-parallel cross-entropy: the softmax split around one all-gather
# ---------------------------------------------------------------------------


def ce_shard_stats(
    logits_shard: torch.Tensor,
    targets: torch.Tensor,
    vocab_start: int,
    ignore_index: int = -100,
) -> torch.Tensor:
    """Stage 1 of the vocab-parallel CE on one ``[N, Vs]`` column shard of
    the logits: fp32 ``stats[N, 3] = (m, s, t)`` per row — the shard max,
    ``sum exp(x - m)`` over the shard, and the target's logit when
    ``vocab_start <= target < vocab_start + Vs`` (else 0). ``targets`` hold
    GLOBAL vocabulary ids. Every row gets defined values, ignored rows too
    (the buffer goes through a collective). GPU: one read of the shard."""
    vs = logits_shard.shape[-1]
    if _use_hip(logits_shard):
        return hip_ops().ce_shard_stats(
            logits_shard.view(-1, vs), targets.reshape(-1).int(), vocab_start,
            ignore_index,
        )
    x = logits_shard.detach().reshape(-1, vs).float()
    t = targets.reshape(-1).long()
    m = x.amax(-1)
    s = torch.exp(x - m[:, None]).sum(-1)
    local = t - vocab_start
    owns = (t != ignore_index) & (local >= 0) & (local < vs)
    # never index with an out-of-shard target: clamp it to column 0 first
    picked = x.gather(1, torch.where(owns, local, 0)[:, None]).squeeze(1)
    return torch.stack([m, s, torch.where(owns, picked, 0.0)], dim=1)


def ce_shard_finish(
    logits_shard: torch.Tensor,
    targets: torch.Tensor,
    vocab_start: int,
    stats_all: torch.Tensor,
    grad_scale: float,
    ignore_index: int = -100,
    compute_grad: bool = True,
) -> torch.Tensor:
    """Stage 2: combine ``stats_all[tp, N, 3]`` (every shard's stats in rank
    order) into the per-row loss and overwrite ``logits_shard`` in place with
    ``(softmax - onehot) * grad_scale`` for this shard's columns. The combine
    runs in rank order r = 0..tp-1, so every shard that is handed the same
    ``stats_all`` returns bitwise the same losses. Ignored rows: loss 0 and
    zero gradients. The logits shard is consumed."""
    vs = logits_shard.shape[-1]
    if _use_hip(logits_shard):
        return hip_ops().ce_shard_finish(
            logits_shard.view(-1, vs), targets.reshape(-1).int(), vocab_start,
            stats_all, grad_scale, ignore_index, compute_grad,
        )
    t = targets.reshape(-1).long()
    n = t.numel()
    sa = stats_all.reshape(-1, n, 3).float()
    tp = sa.shape[0]
    gm = sa[0, :, 0]
    for r in range(1, tp):
        gm = torch.maximum(gm, sa[r, :, 0])
    gs = torch.zeros_like(gm)
    gt = torch.zeros_like(gm)
    for r in range(tp):
        gs = gs + sa[r, :, 1] * torch.exp(sa[r, :, 0] - gm)
        gt = gt + sa[r, :, 2]
    lse = gm + torch.log(gs)
    valid = t != ignore_index
    losses = torch.where(valid, lse - gt, 0.0)
    if compute_grad:
        x = logits_shard.detach().reshape(-1, vs).float()
        dl = torch.exp(x - lse[:, None])
        local = t - vocab_start
        owns = valid & (local >= 0) & (local < vs)
        rows = owns.nonzero().squeeze(1)
        dl[rows, local[rows]] -= 1.0
        dl = dl * grad_scale
        dl[~valid] = 0
        with torch.no_grad():
            logits_shard.copy_(dl.view_as(logits_shard))
    return losses


class _VocabParallelCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_shard, targets, vocab_start, tp_group, ignore_index):
        n_valid = int((targets != ignore_index).sum())
        grad_scale = 1.0 / max(n_valid, 1)
        if _use_hip(logits_shard):
            work = logits_shard.contiguous()  # consumed, as cross_entropy_loss
            tgt = targets.reshape(-1).int().contiguous()
        else:
            work = logits_shard.detach().float().clone()
            tgt = targets.reshape(-1)
        stats = ce_shard_stats(work, tgt, vocab_start, ignore_index)
        if tp_group is None:  # tp degenerate (parallel/tp.py): no collective
            stats_all = stats[None]
        else:
            import torch.distributed as dist

            tp = dist.get_world_size(tp_group)
            # gathered concatenated along dim 0 (the layout every backend
            # accepts), which IS [tp, N, 3] in rank order
            flat = stats.new_empty((tp * stats.shape[0], 3))
            dist.all_gather_into_tensor(flat, stats, group=tp_group)
            stats_all = flat.view(tp, stats.shape[0], 3)
        losses = ce_shard_finish(
            work, tgt, vocab_start, stats_all, grad_scale, ignore_index, True
        )
        # work now holds this shard's dlogits (pre-scaled)
        ctx.save_for_backward(work.to(logits_shard.dtype).view_as(logits_shard))
        return losses.sum() * grad_scale

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None, None, None, None


def vocab_parallel_cross_entropy(
    logits_shard: torch.Tensor,
    targets: torch.Tensor,
    vocab_start: int,
    tp_group=None,
    ignore_index: int = -100,
) -> torch.Tensor:
    """Mean CE over non-ignored tokens when the vocabulary dimension is split
    across a tensor-parallel group: ``logits_shard`` is this rank's
    ``[tokens, V/tp]`` columns starting at global id ``vocab_start``,
    ``targets`` hold global ids. One collective (an all-gather of the
    ``[N, 3]`` row statistics) and two kernels; every rank combines the same
    gathered buffer in the same order, so the loss is bitwise identical across
    the group. ``tp_group=None`` is the degenerate single-shard case. The GPU
    path consumes ``logits_shard`` (reused for dlogits)."""
    return _VocabParallelCrossEntropy.apply(
        logits_shard, targets, vocab_start, tp_group, ignore_index
    )


def fused_adamw_step(
    param_f32: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    param_bf16: Optional[torch.Tensor],
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step: int,
    grad_scale: float = 1.0,
):
    """Single fused AdamW update; see FusedAdamW for the optimizer class."""
    if param_f32.is_cuda:
        hip_ops().adamw_step(
            param_f32,
            grad.contiguous(),
            exp_avg,
            exp_avg_sq,
            param_bf16,
            lr,
            beta1,
            beta2,
            eps,
            weight_decay,
            step,
            grad_scale,
        )
        return
    # CPU reference
    g = grad.float() * grad_scale
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (exp_avg_sq / bc2).sqrt().add_(eps)
    param_f32.add_(
        exp_avg / bc1 / denom + weight_decay * param_f32, alpha=-lr
    )
    if param_bf16 is not None:
        param_bf16.copy_(param_f32.to(param_bf16.dtype))


# ---------------------------------------------------------------------------
# multi-tensor ops: global gradient norm + batched AdamW
# ---------------------------------------------------------------------------


def grad_sq_norm_slots(tensors, span_elems: int = 0) -> int:
    """How many fp32 partial slots ``grad_sq_norm`` needs for this tensor
    list at this span (0 = automatic). The CPU reference needs none."""
    tensors = list(tensors)
    if _use_hip(*tensors):
        return int(hip_ops().multi_tensor_num_partials(tensors, span_elems))
    return 0


def grad_sq_norm(
    tensors,
    out: Optional[torch.Tensor] = None,
    partials: Optional[torch.Tensor] = None,
    span_elems: int = 0,
) -> torch.Tensor:
    """Sum of squares over every element of every tensor (bf16 or fp32,
    contiguous, any element offset) into ``out[0]`` (fp32). No host sync.

    GPU: two kernels, no atomics — bitwise reproducible. ``partials`` is the
    caller-owned fp32 workspace of ``grad_sq_norm_slots`` elements and
    ``out`` a caller-owned fp32 tensor; both are allocated here when omitted
    (pass them to stay allocation-free, e.g. under graph capture)."""
    tensors = list(tensors)
    if _use_hip(*tensors, out):
        dev = next(t.device for t in tensors + [out] if t is not None and t.is_cuda)
        if out is None:
            out = torch.empty(1, device=dev, dtype=torch.float32)
        if partials is None:
            n = hip_ops().multi_tensor_num_partials(tensors, span_elems)
            partials = torch.empty(max(int(n), 1), device=dev, dtype=torch.float32)
        hip_ops().multi_tensor_sq_norm(tensors, partials, out, span_elems)
        return out
    # CPU reference
    total = torch.zeros((), dtype=torch.float64)
    for t in tensors:
        if t.numel():
            total = total + t.detach().float().pow(2).sum(dtype=torch.float64)
    if out is None:
        out = torch.empty(1, dtype=torch.float32)
    out.view(-1)[0] = total.float()
    return out


def fused_adamw_multi_step(
    masters,
    grads,
    exp_avgs,
    exp_avg_sqs,
    params_bf16,
    lrs,
    weight_decays,
    steps,
    beta1: float,
    beta2: float,
    eps: float,
    grad_scale: float = 1.0,
    norm_sq: Optional[torch.Tensor] = None,
    max_norm: float = float("inf"),
    skip_nonfinite: bool = True,
    span_elems: int = 0,
):
    """AdamW over a list of tensors in a few batched launches.

    Per-tensor: master/grad/moments, optional bf16 working copy (``None``
    entries, or ``params_bf16=None`` for none at all), lr, weight decay and
    step. Per call: betas, eps, one gradient dtype.

    With ``norm_sq`` (fp32 tensor holding the global squared gradient norm)
    every gradient is additionally multiplied by
    ``min(1, max_norm / (sqrt(norm_sq) + 1e-6))`` — torch's
    ``clip_grad_norm_`` coefficient — computed on the device. If ``norm_sq``
    is not finite and ``skip_nonfinite`` is set nothing is written at all."""
    masters = list(masters)
    if not masters:
        return
    if params_bf16 is None:
        params_bf16 = [None] * len(masters)
    if masters[0].is_cuda:
        hip_ops().multi_tensor_adamw(
            masters,
            [g.contiguous() for g in grads],
            list(exp_avgs),
            list(exp_avg_sqs),
            list(params_bf16),
            [float(x) for x in lrs],
            [float(x) for x in weight_decays],
            [int(x) for x in steps],
            beta1,
            beta2,
            eps,
            grad_scale,
            norm_sq,
            max_norm,
            skip_nonfinite,
            span_elems,
        )
        return
    # CPU reference: the per-tensor reference with the clip folded into the
    # gradient scale
    scale = grad_scale
    if norm_sq is not None:
        nsq = norm_sq.detach().reshape(-1)[0].float()
        if skip_nonfinite and not bool(torch.isfinite(nsq)):
            return
        coef = torch.clamp(max_norm / (nsq.sqrt() + 1e-6), max=1.0)
        scale = coef * grad_scale
    for i, master in enumerate(masters):
        fused_adamw_step(
            master,
            grads[i],
            exp_avgs[i],
            exp_avg_sqs[i],
            params_bf16[i],
            lrs[i],
            beta1,
            beta2,
            eps,
            weight_decays[i],
            steps[i],
            scale,
        )


# ---------------------------------------------------------------------------
# FP8 block-scaled optimizer moments
#
# A block is 256 consecutive elements of a contiguous tensor whose last dim
# is a multiple of 256. Per block: scale = absmax / 448 (fp32 division),
# code = RNE_e4m3fn(x / scale) stored as uint8, dequant = float(code) * scale.
# A block whose scale would be below the smallest normal fp32 (absmax under
# about 5.3e-36, the all-zero block included) is flushed: scale 0, codes 0. A
# subnormal scale has too few bits to keep x / scale within +-448. A NaN or
# inf element makes the scale NaN or inf, and with it its whole block.
# ---------------------------------------------------------------------------

FP8_BLOCK = 256
FP8_E4M3_MAX = 448.0
FP8_MIN_SCALE = 1.1754943508222875e-38  # FLT_MIN


def _fp8_blocks(t: torch.Tensor) -> torch.Tensor:
    if t.dim() < 1 or t.shape[-1] % FP8_BLOCK:
        raise ValueError(
            f"fp8 blocks: the last dim must be a multiple of {FP8_BLOCK}, "
            f"got shape {tuple(t.shape)}"
        )
    return t.reshape(*t.shape[:-1], t.shape[-1] // FP8_BLOCK, FP8_BLOCK)


def fp8_block_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``[..., C]`` -> ``(codes, scales)``: OCP e4m3fn bit patterns as
    uint8 ``[..., C]`` (``codes.view(torch.float8_e4m3fn)`` decodes them) and
    fp32 scales ``[..., C/256]``, by the definition above."""
    x = x.detach().float().contiguous()
    xb = _fp8_blocks(x)
    if _use_hip(x):
        return tuple(hip_ops().fp8_block_quantize(x))
    # CPU reference: the definition
    scales = xb.abs().amax(-1) / FP8_E4M3_MAX
    # degenerate blocks are flushed; a NaN scale is not below FP8_MIN_SCALE
    scales = torch.where(scales < FP8_MIN_SCALE, torch.zeros_like(scales), scales)
    s = scales.unsqueeze(-1)
    y = torch.where(s != 0, xb / s, torch.zeros_like(xb))
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(x.shape)
    return codes, scales


def fp8_block_dequantize(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Inverse of ``fp8_block_quantize``: fp32 ``float(code) * scale``."""
    cb = _fp8_blocks(codes)
    if _use_hip(codes, scales):
        return hip_ops().fp8_block_dequantize(codes.contiguous(), scales.contiguous())
    vals = cb.contiguous().view(torch.float8_e4m3fn).float() * scales.unsqueeze(-1)
    return vals.reshape(codes.shape)


# ---------------------------------------------------------------------------
# FP8 linear layers: tensor-wise scaled GEMM operands
#
# "Current" scaling of a 2-D tensor t[R, C] (bf16 or fp32), one scale per
# tensor, by the convention of the block quantiser above: FMAX is 448 for
# e4m3 (float8_e4m3fn) and 57344 for e5m2; scale = absmax(t) / FMAX (fp32
# division, NaN-propagating absmax); a scale below FLT_MIN (the all-zero
# tensor included) is flushed to 0 with all codes 0; otherwise
# code = RNE(float(t) / scale) and the dequantised value is
# float(code) * scale. An inf or NaN element makes the scale inf or NaN, and
# since the scale multiplies every output of a product, a non-finite input
# gives a non-finite output everywhere. The scale is a 1-element fp32 tensor
# on the tensor's device; nothing is read on the host.
#
# The GEMM is the library's (torch._scaled_mm, a row-major and b
# column-major), so the dgrad and wgrad products need transposed codes; the
# HIP cast kernel writes both layouts from one read of the tensor.
# ---------------------------------------------------------------------------

FP8_FORMATS = {
    "e4m3": (torch.float8_e4m3fn, 448.0),
    "e5m2": (torch.float8_e5m2, 57344.0),
}

# calls of fp8_linear that took plain F.linear because M, N or K is not a
# multiple of 16
fp8_linear_fallbacks = 0

_FP8_MM_OK = {}


def _fp8_format(fmt: str):
    try:
        return FP8_FORMATS[fmt]
    except KeyError:
        raise ValueError(f"fp8 format must be 'e4m3' or 'e5m2', got {fmt!r}") from None


def fp8_quantize(
    t: torch.Tensor,
    fmt: str = "e4m3",
    rowwise: bool = True,
    colwise: bool = False,
    scale: Optional[torch.Tensor] = None,
    partials: Optional[torch.Tensor] = None,
):
    """``t[R, C]`` (bf16 or fp32) -> ``(codes | None, codes_t | None, scale)``.

    ``codes`` is ``[R, C]`` (``rowwise``) and ``codes_t`` ``[C, R]``, the same
    codes transposed (``colwise``), both ``torch.float8_*`` and contiguous:
    ``codes`` is a ready ``a`` operand of ``torch._scaled_mm`` and
    ``codes_t.t()`` a ready ``b`` operand. ``scale`` is the 1-element fp32
    scale by the definition above; pass a saved one to reuse it without a
    second absmax pass.

    GPU: a two-stage absmax (no atomics; ``partials`` is its int32 workspace
    of ``hip_ops().fp8_amax_slots(t)`` elements, allocated here when omitted)
    and one cast kernel that reads ``t`` once for both layouts. No host sync.
    CPU: the definition in torch ops."""
    dtype, fmax = _fp8_format(fmt)
    if t.dim() != 2:
        raise ValueError(f"fp8_quantize: expected a 2-D tensor, got {tuple(t.shape)}")
    if t.shape[0] % 16 or t.shape[1] % 16 or t.numel() == 0:
        raise ValueError(
            "fp8_quantize: both dimensions must be positive multiples of 16, "
            f"got {tuple(t.shape)}"
        )
    if t.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"fp8_quantize: expected bf16 or fp32, got {t.dtype}")
    if scale is not None and (scale.dtype != torch.float32 or scale.numel() != 1):
        raise ValueError("fp8_quantize: scale must be a 1-element fp32 tensor")
    t = t.detach()
    if _use_hip(t):
        ext = hip_ops()
        t = t.contiguous()
        if t.data_ptr() % 16:  # a view at an odd offset: the kernels load 16 B
            t = t.clone()
        if scale is None:
            scale = torch.empty(1, device=t.device, dtype=torch.float32)
            if partials is None:
                partials = torch.empty(
                    ext.fp8_amax_slots(t), device=t.device, dtype=torch.int32
                )
            ext.fp8_amax_scale(t, fmt, partials, scale)
        else:
            scale = scale.reshape(1)
        codes, codes_t = ext.fp8_cast_transpose(t, scale, fmt, rowwise, colwise)
        return (
            codes.view(dtype) if codes is not None else None,
            codes_t.view(dtype) if codes_t is not None else None,
            scale,
        )
    # CPU reference: the definition
    tf = t.float()
    if scale is None:
        scale = (tf.abs().amax() / fmax).reshape(1)
        # a NaN scale is not below FP8_MIN_SCALE
        scale = torch.where(scale < FP8_MIN_SCALE, torch.zeros_like(scale), scale)
    else:
        scale = scale.reshape(1)
    y = torch.where(scale != 0, tf / scale, torch.zeros_like(tf))
    codes = y.to(dtype)
    return (
        codes if rowwise else None,
        codes.t().contiguous() if colwise else None,
        scale,
    )


def _fp8_mm(a, b, scale_a, scale_b, out_dtype):
    """``(a * scale_a) @ (b * scale_b)``: ``a`` fp8 row-major, ``b`` e4m3
    column-major. GPU: the library's scaled GEMM. CPU: an fp32 matmul of the
    dequantised operands, rounded to ``out_dtype`` (the oracle)."""
    if a.is_cuda:
        return torch._scaled_mm(
            a, b, scale_a=scale_a, scale_b=scale_b, out_dtype=out_dtype,
            use_fast_accum=False,
        )
    return ((a.float() * scale_a) @ (b.float() * scale_b)).to(out_dtype)


def fp8_linear_supported(
    grad_format: str = "e5m2", device: Optional[torch.device] = None
) -> bool:
    """Whether ``torch._scaled_mm`` takes the products ``fp8_linear`` needs on
    this device: e4m3 x e4m3 (forward) and ``grad_format`` x e4m3 (backward).
    One 16x16x16 product each, run once and cached. A rejection by the library
    is a Python exception; that is all this guards against. The CPU path
    needs no scaled GEMM and is always supported."""
    _fp8_format(grad_format)
    if device is None:
        if not torch.cuda.is_available():
            return True
        device = "cuda"
    dev = torch.device(device)
    if dev.type != "cuda":
        return True
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    ok = True
    for fmt in ("e4m3", grad_format):
        key = (index, fmt)
        if key not in _FP8_MM_OK:
            try:
                a = torch.ones(16, 16, device=dev).to(FP8_FORMATS[fmt][0])
                b = torch.ones(16, 16, device=dev).to(torch.float8_e4m3fn)
                one = torch.ones(1, device=dev)
                _fp8_mm(a, b.t(), one, one, torch.bfloat16)
                _FP8_MM_OK[key] = True
            except Exception:  # noqa: BLE001 - any rejection by the library
                _FP8_MM_OK[key] = False
        ok = ok and _FP8_MM_OK[key]
    return ok


class _Fp8Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, grad_format):
        K = x.shape[-1]
        N = weight.shape[0]
        xq, xq_t, sx = fp8_quantize(x.reshape(-1, K), "e4m3", True, True)
        wq, _, sw = fp8_quantize(weight, "e4m3", True, False)
        y = _fp8_mm(xq, wq.t(), sx, sw, x.dtype)
        # the weight itself, not its codes: under FSDP2 the unsharded weight
        # is freed between forward and backward, a saved 8-bit copy would
        # keep 1 byte per parameter of every layer alive
        ctx.save_for_backward(xq_t, sx, sw, weight)
        ctx.grad_format = grad_format
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xq_t, sx, sw, weight = ctx.saved_tensors
        N, K = weight.shape
        lead = dy.shape[:-1]
        gq, gq_t, sg = fp8_quantize(
            dy.reshape(-1, N), ctx.grad_format, True, ctx.needs_input_grad[1]
        )
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # the forward's scale: no second absmax over the weight
            _, wq_t, _ = fp8_quantize(weight, "e4m3", False, True, scale=sw)
            dx = _fp8_mm(gq, wq_t.t(), sg, sw, dy.dtype).view(*lead, K)
        if ctx.needs_input_grad[1]:
            dw = _fp8_mm(gq_t, xq_t.t(), sg, sx, weight.dtype)
        return dx, dw, None


def fp8_linear(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    grad_format: str = "e5m2",
) -> torch.Tensor:
    """``F.linear`` with FP8 GEMM operands: ``x`` (flattened to ``[M, K]``)
    and ``weight[N, K]`` as e4m3, the output gradient as ``grad_format``, each
    with one current absmax scale; accumulation in fp32, outputs in the input
    dtypes. The bias is a separate add; its gradient is the plain sum.

    If M, N or K is not a multiple of 16 the call is plain ``F.linear`` and
    ``fp8_linear_fallbacks`` counts it."""
    global fp8_linear_fallbacks
    _fp8_format(grad_format)
    N, K = weight.shape
    M = x.numel() // K if K else 0
    if M % 16 or N % 16 or K % 16 or M == 0 or N == 0:
        fp8_linear_fallbacks += 1
        return torch.nn.functional.linear(x, weight, bias)
    if x.is_cuda and not fp8_linear_supported(grad_format, x.device):
        raise RuntimeError(
            "fp8_linear: torch._scaled_mm rejects the e4m3 x e4m3 or "
            f"{grad_format} x e4m3 product on this device"
        )
    y = _Fp8Linear.apply(x, weight, grad_format)
    if bias is not None:
        y = y + bias
    return y


def fused_adamw_fp8_multi_step(
    masters,
    grads,
    exp_avgs,
    exp_avg_scales,
    exp_avg_sq_roots,
    exp_avg_sq_root_scales,
    params_bf16,
    lrs,
    weight_decays,
    steps,
    beta1: float,
    beta2: float,
    eps: float,
    grad_scale: float = 1.0,
    norm_sq: Optional[torch.Tensor] = None,
    max_norm: float = float("inf"),
    skip_nonfinite: bool = True,
    span_elems: int = 0,
):
    """``fused_adamw_multi_step`` on FP8 block-scaled moments: ``exp_avgs``
    and ``exp_avg_sq_roots`` are uint8 e4m3fn codes shaped like their master,
    with one fp32 scale per 256-block; the second moment is kept as its
    square root. Every master's last dim must be a multiple of 256.

    The update uses the fresh fp32 moments; quantisation error enters only
    through the state the next step loads. Clipping and the non-finite skip
    work as in ``fused_adamw_multi_step``. ``span_elems`` (0 = automatic) is
    a multiple of 256."""
    masters = list(masters)
    if not masters:
        return
    if params_bf16 is None:
        params_bf16 = [None] * len(masters)
    if masters[0].is_cuda:
        hip_ops().multi_tensor_adamw_fp8(
            masters,
            [g.contiguous() for g in grads],
            list(exp_avgs),
            list(exp_avg_scales),
            list(exp_avg_sq_roots),
            list(exp_avg_sq_root_scales),
            list(params_bf16),
            [float(x) for x in lrs],
            [float(x) for x in weight_decays],
            [int(x) for x in steps],
            beta1,
            beta2,
            eps,
            grad_scale,
            norm_sq,
            max_norm,
            skip_nonfinite,
            span_elems,
        )
        return
    # CPU reference: the fp32 reference step on the dequantised state, then
    # the definition of the format
    if norm_sq is not None and skip_nonfinite:
        if not bool(torch.isfinite(norm_sq.detach().reshape(-1)[0])):
            return
    ms = [fp8_block_dequantize(c, s) for c, s in zip(exp_avgs, exp_avg_scales)]
    vs = [
        fp8_block_dequantize(c, s).square_()
        for c, s in zip(exp_avg_sq_roots, exp_avg_sq_root_scales)
    ]
    fused_adamw_multi_step(
        masters, grads, ms, vs, params_bf16, lrs, weight_decays, steps,
        beta1, beta2, eps, grad_scale, norm_sq, max_norm, skip_nonfinite,
    )
    for i in range(len(masters)):
        for x, codes, scales in (
            (ms[i], exp_avgs[i], exp_avg_scales[i]),
            (vs[i].sqrt_(), exp_avg_sq_roots[i], exp_avg_sq_root_scales[i]),
        ):
            c, s = fp8_block_quantize(x)
            codes.copy_(c)
            scales.copy_(s)


# ---------------------------------------------------------------------------
# checkpoint integrity: per-tensor checksums, fused pack / unpack
# ---------------------------------------------------------------------------

_U64 = (1 << 64) - 1


def _as_byte_array(buf):
    """1-D uint8 numpy view of a CPU tensor, numpy array or bytes-like."""
    import numpy as np

    if isinstance(buf, torch.Tensor):
        t = buf.detach()
        if t.is_cuda:
            t = t.cpu()
        return t.contiguous().reshape(-1).view(torch.uint8).numpy()
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    return np.frombuffer(buf, dtype=np.uint8)


def ckpt_checksum_ref(buf, chunk_words: int = 1 << 20) -> Tuple[int, int]:
    """Checksum ``(A, B)`` of a buffer's bytes (CPU tensor, numpy array or
    bytes-like), as two Python ints below 2**64.

    The bytes are extended with zero bytes to a multiple of 4 and read as
    little-endian u32 words ``w_0 .. w_{W-1}``; ``A = sum w_i`` and
    ``B = sum (2i+1) * w_i``, both mod 2**64. A single flipped bit always
    changes ``A``; a swap of two different words always changes ``B`` (the
    weights are odd and distinct); zero words contribute nothing, so padding
    never matters; and any partition of the words gives the same bits, which
    is what lets the device kernel (``ckpt_checksum``) spread them over blocks
    and launches. This is an error-detection code against torn, stale or
    damaged payloads, NOT a cryptographic hash: it offers no protection
    against deliberate tampering.

    numpy, in chunks of ``chunk_words`` so temporaries stay bounded. It serves
    CPU tensors, the CPU tests and as the oracle of the device kernel; it is
    not a path for large payloads: measured at about 0.2 GB/s on one host
    core (256 MiB buffer), which is minutes for a 100 GB state."""
    import numpy as np

    raw = _as_byte_array(buf)
    n = raw.size
    full = n // 4
    words = raw[: 4 * full].view("<u4")
    a = 0
    b = 0
    chunk_words = max(int(chunk_words), 1)
    with np.errstate(over="ignore"):
        for c0 in range(0, full, chunk_words):
            w = words[c0 : c0 + chunk_words].astype(np.uint64)
            idx = np.arange(c0, c0 + w.size, dtype=np.uint64)
            a += int(w.sum(dtype=np.uint64))
            b += int(((idx * np.uint64(2) + np.uint64(1)) * w).sum(dtype=np.uint64))
    if n > 4 * full:
        last = int.from_bytes(raw[4 * full :].tobytes(), "little")
        a += last
        b += (2 * full + 1) * last
    return a & _U64, b & _U64


def ckpt_sums_to_ints(sums: torch.Tensor):
    """``[N, 2]`` int64 sums (device or host) -> list of ``(A, B)`` Python
    ints below 2**64. Reads the tensor on the host (synchronises a GPU)."""
    return [(int(a) & _U64, int(b) & _U64) for a, b in sums.reshape(-1, 2).tolist()]


def _ckpt_nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def ckpt_sum_slots(nbytes_list, span_bytes: int = 0) -> int:
    """How many ``[slot, 2]`` int64 partial slots the device pack / unpack /
    checksum needs for tensors of these byte sizes at this span (0 =
    automatic). The CPU fallbacks need none."""
    return int(hip_ops().ckpt_sum_slots([int(n) for n in nbytes_list], span_bytes))


def _ckpt_workspace(tensors, dev, sums, partials, span_bytes):
    n = len(tensors)
    if sums is None:
        sums = torch.empty((n, 2), device=dev, dtype=torch.int64)
    if partials is None:
        slots = ckpt_sum_slots([_ckpt_nbytes(t) for t in tensors], span_bytes)
        partials = torch.empty((max(slots, 1), 2), device=dev, dtype=torch.int64)
    return sums, partials


def _ckpt_sums_cpu(tensors, sums):
    """CPU fallback: the reference checksum of every tensor into sums."""
    import numpy as np

    vals = np.zeros((len(tensors), 2), dtype=np.uint64)
    for i, t in enumerate(tensors):
        vals[i] = ckpt_checksum_ref(t)
    out = torch.from_numpy(vals.view(np.int64))
    if sums is None:
        return out
    sums.reshape(-1)[: out.numel()].copy_(out.reshape(-1))
    return sums


def _ckpt_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().reshape(-1).view(torch.uint8)


def ckpt_pack(
    tensors,
    offsets,
    staging: torch.Tensor,
    sums: Optional[torch.Tensor] = None,
    partials: Optional[torch.Tensor] = None,
    span_bytes: int = 0,
) -> torch.Tensor:
    """Copy the bytes of ``tensors[i]`` to ``staging[offsets[i]:...]`` (a flat
    uint8 buffer) and return the checksums ``sums[N, 2]`` (int64, see
    ``ckpt_checksum_ref``; row i belongs to tensor i). The ranges must not
    overlap. Non-contiguous tensors are made contiguous first.

    GPU: a few batched launches of one copy-with-checksum kernel plus a
    finalize, no atomics, no allocation when ``sums`` and ``partials``
    (``ckpt_sum_slots`` slots) are passed, no host sync: graph-capturable.
    ``span_bytes`` (0 = automatic) is the bytes one block handles."""
    tensors = [t.detach() for t in tensors]
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(tensors):
        raise ValueError("ckpt_pack: one offset per tensor")
    if _use_hip(staging, *tensors):
        tensors = [t if t.numel() == 0 else t.contiguous() for t in tensors]
        sums, partials = _ckpt_workspace(
            tensors, staging.device, sums, partials, span_bytes
        )
        hip_ops().ckpt_copy_sum(0, tensors, staging, offsets, partials, sums, span_bytes)
        return sums
    for t, off in zip(tensors, offsets):
        staging[off : off + _ckpt_nbytes(t)].copy_(_ckpt_bytes(t.contiguous()))
    return _ckpt_sums_cpu(tensors, sums)


def ckpt_unpack(
    staging: torch.Tensor,
    offsets,
    tensors,
    sums: Optional[torch.Tensor] = None,
    partials: Optional[torch.Tensor] = None,
    span_bytes: int = 0,
) -> torch.Tensor:
    """Inverse of ``ckpt_pack``: copy ``staging[offsets[i]:...]`` into the
    (contiguous) ``tensors[i]`` and return the checksums of the bytes moved,
    to be compared with the ones recorded at pack time."""
    tensors = [t.detach() for t in tensors]
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(tensors):
        raise ValueError("ckpt_unpack: one offset per tensor")
    for t in tensors:
        if t.numel() and not t.is_contiguous():
            raise ValueError("ckpt_unpack: destination tensors must be contiguous")
    if _use_hip(staging, *tensors):
        sums, partials = _ckpt_workspace(
            tensors, staging.device, sums, partials, span_bytes
        )
        hip_ops().ckpt_copy_sum(1, tensors, staging, offsets, partials, sums, span_bytes)
        return sums
    for t, off in zip(tensors, offsets):
        _ckpt_bytes(t).copy_(staging[off : off + _ckpt_nbytes(t)])
    return _ckpt_sums_cpu(tensors, sums)


def ckpt_checksum(
    tensors,
    sums: Optional[torch.Tensor] = None,
    partials: Optional[torch.Tensor] = None,
    span_bytes: int = 0,
) -> torch.Tensor:
    """Checksums ``sums[N, 2]`` (int64) of a tensor list without copying
    anything: the verify pass of a restore. GPU tensors are read once by the
    pack kernel with no destination; CPU tensors go through
    ``ckpt_checksum_ref``. ``ckpt_sums_to_ints`` turns the result into
    Python ints."""
    tensors = [t.detach() for t in tensors]
    if _use_hip(*tensors):
        tensors = [t if t.numel() == 0 else t.contiguous() for t in tensors]
        dev = next(t.device for t in tensors if t.is_cuda)
        sums, partials = _ckpt_workspace(tensors, dev, sums, partials, span_bytes)
        hip_ops().ckpt_copy_sum(2, tensors, None, [], partials, sums, span_bytes)
        return sums
    return _ckpt_sums_cpu(tensors, sums)
