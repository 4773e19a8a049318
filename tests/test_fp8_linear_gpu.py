"""GPU: the FP8 linear path — the conversions exhaustively and bitwise, the
fused cast + transpose and the two-stage absmax against the CPU definition,
``fp8_linear`` against an oracle built from the device's own codes, no host
sync, a small model.

Small shapes on purpose: the cast kernel's tile is 128 x 128, so 272 and 1040
give several tiles with a partial one on that axis, and 16 x 262400 has more
tiles (and the absmax more blocks) than the grid cap of 2048, which makes
both kernels stride.
"""

import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FMTS = {"e4m3": (torch.float8_e4m3fn, 448.0), "e5m2": (torch.float8_e5m2, 57344.0)}
SHAPES = [(16, 16), (16, 48), (64, 64), (80, 272), (272, 80), (1040, 64)]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from dlrover_amd.ops.api import hip_ops

    hip_ops()  # raises on a GPU box if the extension didn't build


@pytest.fixture
def scaled_mm():
    from dlrover_amd.ops import fp8_linear_supported

    if not fp8_linear_supported("e4m3"):
        pytest.skip("torch._scaled_mm rejects FP8 operands on this device")


def _dev():
    return torch.device("cuda:0")


def _bits(codes):
    return codes.view(torch.uint8)


def _wide(shape, dtype, seed):
    """Values over eight decades, so fp8 subnormals and zeros occur."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * 10 ** (
        torch.rand(shape, generator=gen) * 8 - 6)
    return x.to(dtype)


# ---------------------------------------------------------------------------
# 1. conversions
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_encode_matches_torch_bitwise(fmt):
    from dlrover_amd.ops import fp8_quantize

    fdtype, fmax = FMTS[fmt]
    vals = torch.arange(256, dtype=torch.uint8).view(fdtype).float()
    vals = vals[torch.isfinite(vals)]  # +-0 and +-FMAX among them
    pos = vals[vals >= 0].sort().values
    pos = pos[1:] if pos[0] == 0 and pos[1] == 0 else pos
    mids = (pos[:-1] + pos[1:]) / 2  # exact in fp32
    inf = torch.tensor(float("inf"))
    around = torch.cat([mids, torch.nextafter(mids, inf), torch.nextafter(mids, -inf)])
    x = torch.cat([vals, around, -around])
    assert (x == fmax).any() and (x == -fmax).any() and (x == 0).any()
    assert (x.abs() <= fmax).all()
    n = -(-x.numel() // 256) * 256
    flat = torch.zeros(n)
    flat[: x.numel()] = x
    t = flat.view(-1, 16)
    codes, codes_t, scale = fp8_quantize(t.to(_dev()), fmt, colwise=True)
    assert scale.item() == 1.0  # +-FMAX is planted
    ref = _bits(t.to(fdtype))
    got = _bits(codes).cpu()
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, [
        (float(t[i, j]), int(got[i, j]), int(ref[i, j])) for i, j in bad[:8]
    ]
    assert torch.equal(_bits(codes_t).cpu(), ref.t())


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_encode_nan_decodes_to_nan(fmt):
    from dlrover_amd.ops import fp8_quantize

    fdtype, _ = FMTS[fmt]
    t = _wide((16, 32), torch.float32, 3).clamp(-400, 400)
    t[0, 0] = t[7, 19] = t[15, 31] = float("nan")
    one = torch.ones(1, device=_dev())
    codes, codes_t, _ = fp8_quantize(t.to(_dev()), fmt, colwise=True, scale=one)
    nan = torch.isnan(t)
    assert torch.equal(torch.isnan(codes.float().cpu()), nan)
    assert torch.equal(torch.isnan(codes_t.float().cpu()), nan.t())
    assert torch.equal(_bits(codes).cpu()[~nan], _bits(t.to(fdtype))[~nan])


# ---------------------------------------------------------------------------
# 2. cast + transpose, absmax
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES + [(16, 262400)])
def test_cast_transpose_matches_definition(shape, dtype, fmt):
    from dlrover_amd.ops import fp8_quantize

    x = _wide(shape, dtype, 0)
    ref, _, ref_scale = fp8_quantize(x, fmt)  # CPU: the definition
    xd = x.to(_dev())
    codes, codes_t, scale = fp8_quantize(xd, fmt, rowwise=True, colwise=True)
    assert codes.dtype == ref.dtype and codes_t.dtype == ref.dtype
    assert codes.shape == shape and codes_t.shape == shape[::-1]
    assert codes.is_contiguous() and codes_t.is_contiguous()
    assert torch.equal(scale.cpu(), ref_scale)
    assert torch.equal(_bits(codes).cpu(), _bits(ref))
    assert torch.equal(_bits(codes_t), _bits(codes).t())
    # either layout alone, from the saved scale
    only_r, none_t, s2 = fp8_quantize(xd, fmt, rowwise=True, colwise=False, scale=scale)
    none_r, only_t, _ = fp8_quantize(xd, fmt, rowwise=False, colwise=True, scale=scale)
    assert none_t is None and none_r is None and s2.data_ptr() == scale.data_ptr()
    assert torch.equal(_bits(only_r), _bits(codes))
    assert torch.equal(_bits(only_t), _bits(codes_t))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("where", ["first", "last", "negative", "middle"])
def test_absmax_finds_the_planted_maximum(where, dtype):
    from dlrover_amd.ops import fp8_quantize

    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2048, 272, generator=gen).to(dtype)  # |x| < 7
    flat = x.view(-1)
    at = {"first": 0, "last": -1, "negative": 12345, "middle": 300001}[where]
    flat[at] = -96.0 if where == "negative" else 96.0
    for fmt, (_, fmax) in FMTS.items():
        _, _, scale = fp8_quantize(x.to(_dev()), fmt)
        assert scale.dtype == torch.float32 and scale.shape == (1,)
        assert scale.item() == (torch.tensor(96.0) / fmax).item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_absmax_propagates_nonfinite(bad, dtype):
    from dlrover_amd.ops import fp8_quantize

    x = torch.randn(2048, 272).to(dtype)
    x[1777, 133] = bad
    codes, _, scale = fp8_quantize(x.to(_dev()), "e4m3")
    if bad != bad:
        assert torch.isnan(scale).all()
        assert torch.isnan(codes.float()).all()
    else:
        assert torch.isinf(scale).all() and scale.item() > 0
        # finite / inf = 0, inf / inf = NaN: no silently finite large value
        dec = codes.float().cpu()
        assert torch.isnan(dec[1777, 133]) and int((dec != 0).sum()) == 1


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_zero_and_tiny_tensors_are_flushed(fmt):
    from dlrover_amd.ops import fp8_quantize

    for x in (torch.zeros(2048, 272), torch.full((64, 64), 1e-37),
              torch.zeros(80, 272, dtype=torch.bfloat16)):
        codes, codes_t, scale = fp8_quantize(x.to(_dev()), fmt, colwise=True)
        assert scale.item() == 0.0
        assert not _bits(codes).any() and not _bits(codes_t).any()


def test_quantize_rejects_bad_input():
    from dlrover_amd.ops import fp8_quantize

    with pytest.raises(ValueError):
        fp8_quantize(torch.zeros(24, 16, device=_dev()))
    with pytest.raises(ValueError):
        fp8_quantize(torch.zeros(16, device=_dev()))
    with pytest.raises(ValueError):
        fp8_quantize(torch.zeros(16, 16, device=_dev(), dtype=torch.float16))


def test_quantize_unaligned_view():
    """A contiguous view that starts 2 bytes into an allocation."""
    from dlrover_amd.ops import fp8_quantize

    base = _wide((16 * 32 + 1,), torch.bfloat16, 5).to(_dev())
    x = base[1:].view(16, 32)
    assert x.data_ptr() % 16 != 0
    ref, _, ref_scale = fp8_quantize(x.cpu())
    codes, codes_t, scale = fp8_quantize(x, colwise=True)
    assert torch.equal(scale.cpu(), ref_scale)
    assert torch.equal(_bits(codes).cpu(), _bits(ref))
    assert torch.equal(_bits(codes_t), _bits(codes).t())


# ---------------------------------------------------------------------------
# 3. fp8_linear
# ---------------------------------------------------------------------------


# Coefficient of the accumulation term below. With 1 (any-order fp32
# accumulation) the MI355X library misses the bound: measured worst
# error / bound 1.226, at dx of (32, 64, 48) with e5m2 gradients, on an
# element whose products nearly cancel; the smallest coefficient that holds
# all cases of this file is 1.27, and ACC_COEF is twice that. The cause is the
# library's accumulator, not the codes: the same products with fp32 output
# are off by up to 2.7e-5 A at every contraction length from 32 to 128
# (5e-6 A at 1024, 2e-6 A at 4096), which fp32 accumulation (2^-24 A per add)
# cannot produce, while small-integer operands give exact results. hipBLASLt
# runs these products on the 128-deep FP8 MFMA forms, which appear to align
# the products of one instruction to the largest and drop low bits. On the CPU
# torch._scaled_mm stays within the bound with coefficient 1.
ACC_COEF = 2.54


def _within(got, a, sa, b, sb, k):
    """|got - ref| <= 2^-7 |ref| + ACC_COEF k 2^-23 A for ref = (a sa) @ (b sb)
    in fp64 and A = (|a| @ |b|) sa sb: one bf16 ulp of the output plus the
    error of accumulating over the contraction length k. Returns the worst
    ratio of the error to the bound, and the smallest coefficient that would
    hold."""
    a, b = a.double().cpu(), b.double().cpu()
    s = sa.double().cpu() * sb.double().cpu()
    ref = (a @ b) * s
    acc = (k * 2.0 ** -23 * (a.abs() @ b.abs()) * s).clamp_min(1e-300)
    err = (got.double().cpu() - ref).abs()
    ratio = err / (2.0 ** -7 * ref.abs() + ACC_COEF * acc)
    need = (err - 2.0 ** -7 * ref.abs()) / acc
    return float(ratio.max()), float(need.max())


@pytest.mark.parametrize("grad_format", ["e5m2", "e4m3"])
@pytest.mark.parametrize("mkn", [(32, 64, 48), (256, 512, 128)])
def test_linear_matches_oracle_of_own_codes(scaled_mm, mkn, grad_format):
    from dlrover_amd.ops import fp8_linear, fp8_linear_supported, fp8_quantize

    if not fp8_linear_supported(grad_format):
        pytest.skip(f"torch._scaled_mm rejects {grad_format} x e4m3 on this device")
    M, K, N = mkn
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(M, K, generator=gen).bfloat16().to(_dev()).requires_grad_()
    w = (torch.randn(N, K, generator=gen) * 0.05).bfloat16().to(_dev()).requires_grad_()
    b = torch.randn(N, generator=gen).bfloat16().to(_dev()).requires_grad_()
    dy = torch.randn(M, N, generator=gen).bfloat16().to(_dev())

    y = fp8_linear(x, w, None, grad_format=grad_format)
    y.backward(dy)
    assert y.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16
    assert w.grad.dtype == torch.bfloat16

    xq, xq_t, sx = fp8_quantize(x.detach(), "e4m3", colwise=True)
    wq, wq_t, sw = fp8_quantize(w.detach(), "e4m3", colwise=True)
    gq, gq_t, sg = fp8_quantize(dy, grad_format, colwise=True)
    ratios = {
        "y": _within(y.detach(), xq, sx, wq.t(), sw, K),
        "dx": _within(x.grad, gq, sg, wq_t.t(), sw, N),
        "dw": _within(w.grad, gq_t, sg, xq_t.t(), sx, M),
    }
    print(f"fp8_linear {mkn} {grad_format}: (error / bound, coefficient "
          f"needed) = {ratios}")
    assert all(r <= 1.0 for r, _ in ratios.values()), ratios

    # the bias is a separate add and its gradient the plain sum
    x.grad = w.grad = None
    yb = fp8_linear(x, w, b, grad_format=grad_format)
    assert torch.equal(yb, y.detach() + b.detach())
    yb.backward(dy)
    assert torch.equal(b.grad, dy.sum(0))


def test_linear_fallback_shape_is_plain_linear():
    from dlrover_amd.ops import api, fp8_linear

    gen = torch.Generator().manual_seed(7)
    x = torch.randn(24, 64, generator=gen).bfloat16().to(_dev())  # M = 24
    w = torch.randn(48, 64, generator=gen).bfloat16().to(_dev())
    b = torch.randn(48, generator=gen).bfloat16().to(_dev())
    before = api.fp8_linear_fallbacks
    y = fp8_linear(x, w, b)
    assert api.fp8_linear_fallbacks == before + 1
    assert torch.equal(y, F.linear(x, w, b))


def test_linear_nan_input_poisons_every_output(scaled_mm):
    from dlrover_amd.ops import fp8_linear

    x = torch.randn(32, 64, device=_dev(), dtype=torch.bfloat16)
    x[5, 9] = float("nan")
    w = torch.randn(48, 64, device=_dev(), dtype=torch.bfloat16)
    assert torch.isnan(fp8_linear(x, w)).all()


def test_linear_does_not_sync_the_host(scaled_mm):
    from dlrover_amd.ops import fp8_linear

    x = torch.randn(64, 128, device=_dev(), dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(96, 128, device=_dev(), dtype=torch.bfloat16, requires_grad=True)
    b = torch.randn(96, device=_dev(), dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(64, 96, device=_dev(), dtype=torch.bfloat16)
    fp8_linear(x, w, b).backward(dy)  # warm-up: library handles, the probe
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            dy[0, 0].item()
        except RuntimeError:
            honoured = True
        if honoured:
            fp8_linear(x, w, b).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this build does not honour set_sync_debug_mode('error')")
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all() and torch.isfinite(w.grad).all()


def test_tiny_model_trains_on_device(scaled_mm):
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import Fp8Linear, FusedAdamW, api

    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512, n_layers=2,
        n_heads=2, n_kv_heads=2, max_seq_len=64, rope_base=10000.0,
        linear_precision="fp8",
    )
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(_dev()).bfloat16()
    proj = [model.blocks[0].attn.qkv_proj, model.blocks[0].attn.o_proj,
            model.blocks[1].mlp.gate_up_proj, model.blocks[1].mlp.down_proj]
    assert all(type(m) is Fp8Linear for m in proj)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    ids = torch.randint(0, cfg.vocab_size, (2, 64), device=_dev())
    before = api.fp8_linear_fallbacks
    losses = []
    for _ in range(20):
        loss = model(ids, ids.clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss)
    losses = [v.item() for v in losses]
    assert all(v == v and abs(v) != float("inf") for v in losses), losses
    assert losses[-1] < losses[0], losses
    for m in proj:
        assert torch.isfinite(m.weight.grad).all() and m.weight.grad.abs().max() > 0
    assert api.fp8_linear_fallbacks == before

    # the bf16 model's checkpoint loads into it
    ref = LlamaForCausalLM(dataclasses.replace(cfg, linear_precision="bf16"))
    model.load_state_dict(ref.state_dict(), strict=True)
