"""GPU: FP8 block-scaled moments — the e4m3 conversions exhaustively and
bitwise, one fused step against fp32 torch, clipping / skipping, a model.

Small shapes on purpose: span_elems=512 makes tensors continue across spans,
and more tensors than one launch takes force a second launch.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SPAN = 512
SHAPES = [(1, 256), (3, 256), (2, 512), (9, 256), (0, 256)]
BETA1, BETA2, EPS = 0.9, 0.95, 1e-8


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from dlrover_amd.ops.api import hip_ops

    hip_ops()  # raises on a GPU box if the extension didn't build


def _dev():
    return torch.device("cuda:0")


def _f8(codes):
    """uint8 codes -> their e4m3fn values in fp32 (torch's own decode)."""
    return codes.view(torch.float8_e4m3fn).float()


def _torch_encode(x):
    """The definition with scale 1, on the CPU."""
    return x.cpu().to(torch.float8_e4m3fn).view(torch.uint8)


# ---------------------------------------------------------------------------
# 1. format
# ---------------------------------------------------------------------------


def test_decode_all_codes():
    from dlrover_amd.ops import fp8_block_dequantize

    codes = torch.arange(256, dtype=torch.uint8, device=_dev()).view(1, 256)
    got = fp8_block_dequantize(codes, torch.ones(1, 1, device=_dev())).cpu()
    ref = _f8(codes.cpu())
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert int(torch.isnan(ref).sum()) == 2  # 0x7f and 0xff
    ok = ~torch.isnan(ref)
    # bit patterns: the sign of -0 counts
    assert torch.equal(got[ok].view(torch.int32), ref[ok].view(torch.int32))


def test_encode_matches_torch_bitwise():
    from dlrover_amd.ops import fp8_block_quantize

    all_codes = torch.arange(256, dtype=torch.uint8)
    vals = _f8(all_codes)
    vals = vals[~torch.isnan(vals)]  # 254 values, +-0 and +-448 among them
    pos = vals[vals >= 0].sort().values
    pos = pos[1:] if pos[0] == 0 and pos[1] == 0 else pos
    mids = (pos[:-1] + pos[1:]) / 2  # exact in fp32: neighbours share 4 bits
    assert mids.numel() == 126
    inf = torch.tensor(float("inf"))
    around = torch.cat([mids, torch.nextafter(mids, inf), torch.nextafter(mids, -inf)])
    x = torch.cat([vals, around, -around])
    assert ((x == 448).any() and (x == -448).any() and (x == 0).any())
    assert (x.abs() <= 448).all()
    # every block of 256 gets one 448 so that its scale is exactly 1
    n_blocks = -(-x.numel() // 255)
    padded = torch.zeros(n_blocks * 255)
    padded[: x.numel()] = x
    blocks = torch.cat([padded.view(n_blocks, 255), torch.full((n_blocks, 1), 448.0)], 1)
    codes, scales = fp8_block_quantize(blocks.to(_dev()))
    assert torch.equal(scales.cpu(), torch.ones(n_blocks, 1))
    ref = _torch_encode(blocks)
    got = codes.cpu()
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, [
        (float(blocks[i, j]), int(got[i, j]), int(ref[i, j])) for i, j in bad[:8]
    ]


def test_block_quantize_matches_definition_bitwise():
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    gen = torch.Generator().manual_seed(0)
    x = torch.randn(5, 512, generator=gen) * 10 ** (
        torch.rand(5, 512, generator=gen) * 8 - 6
    )
    ref_codes, ref_scales = fp8_block_quantize(x)  # CPU: the definition
    assert ((ref_codes & 0x78) == 0).any()  # subnormals and flushes occur
    codes, scales = fp8_block_quantize(x.to(_dev()))
    assert codes.dtype == torch.uint8 and codes.shape == (5, 512)
    assert scales.dtype == torch.float32 and scales.shape == (5, 2)
    assert torch.equal(scales.cpu(), ref_scales)
    assert torch.equal(codes.cpu(), ref_codes)
    assert torch.equal(
        fp8_block_dequantize(codes, scales).cpu(),
        fp8_block_dequantize(ref_codes, ref_scales),
    )


def test_zero_block():
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    x = torch.randn(2, 512, device=_dev())
    x[1, :256] = 0.0
    x[0, 300] = -0.0
    codes, scales = fp8_block_quantize(x)
    assert scales[1, 0] == 0 and not codes[1, :256].any()
    assert torch.isfinite(scales).all()
    deq = fp8_block_dequantize(codes, scales)
    assert torch.isfinite(deq).all() and not deq[1, :256].any()


# ---------------------------------------------------------------------------
# 2. one fused step against fp32 torch on the same device
# ---------------------------------------------------------------------------


def _max_tensors():
    from dlrover_amd.ops.api import hip_ops

    return hip_ops().F8_MAX_TENSORS


def _quantize_ref(x):
    """The definition (the CPU reference), results on x's device."""
    from dlrover_amd.ops import fp8_block_quantize

    codes, scales = fp8_block_quantize(x.cpu())
    return codes.to(x.device), scales.to(x.device)


def _dequantize_ref(codes, scales):
    return _f8(codes) * scales.repeat_interleave(256, dim=-1)


def _step_case(gdtype):
    """Old state (quantised random moments), gradients and hyper-parameters
    of the issue's shape list."""
    gen = torch.Generator(device=_dev()).manual_seed(3)
    shapes = list(SHAPES)
    while len(shapes) <= _max_tensors():  # a second launch is needed
        shapes.append((1, 256))
    case = dict(shapes=shapes, masters=[], grads=[], m=[], ms=[], r=[], rs=[],
                lrs=[], wds=[], steps=[])
    for i, shape in enumerate(shapes):
        rnd = lambda: torch.randn(shape, device=_dev(), generator=gen)  # noqa: E731
        m, root, g = rnd() * 1e-2, rnd().abs() * 1e-2, rnd() * 1e-2
        if shape == (9, 256):
            # one block with zero gradient and zero state
            m[4], root[4], g[4] = 0.0, 0.0, 0.0
            # one block whose gradients span more than 2**19, over fresh
            # (zero) state: some new moments are subnormal or flush to zero
            m[7], root[7] = 0.0, 0.0
            g[7] = torch.sign(g[7]) * 2.0 ** -(
                torch.arange(256, device=_dev()) % 23
            ).float()
        if shape == (2, 512):
            # a 2-byte (bf16) or 4-byte (fp32) aligned offset view
            buf = torch.zeros(g.numel() + 16, device=_dev(), dtype=gdtype)
            view = buf[1 : 1 + g.numel()].view(shape)
            view.copy_(g)
            assert view.data_ptr() % 8 != 0 and view.is_contiguous()
            g = view
        else:
            g = g.to(gdtype)
        mc, ms = _quantize_ref(m)
        rc, rs = _quantize_ref(root)
        case["masters"].append(rnd())
        case["grads"].append(g)
        case["m"].append(mc)
        case["ms"].append(ms)
        case["r"].append(rc)
        case["rs"].append(rs)
        case["lrs"].append(1e-2 if i != 3 else 3e-3)
        case["wds"].append(0.1 if i != 3 else 0.0)
        case["steps"].append(2 + i % 5)
    return case


def _run_fused(case):
    from dlrover_amd.ops import fused_adamw_fp8_multi_step

    clone = lambda ts: [t.clone() for t in ts]  # noqa: E731
    st = dict(masters=clone(case["masters"]), m=clone(case["m"]),
              ms=clone(case["ms"]), r=clone(case["r"]), rs=clone(case["rs"]))
    st["bf16"] = [torch.zeros_like(p, dtype=torch.bfloat16) for p in st["masters"]]
    fused_adamw_fp8_multi_step(
        st["masters"], case["grads"], st["m"], st["ms"], st["r"], st["rs"],
        st["bf16"], case["lrs"], case["wds"], case["steps"], BETA1, BETA2, EPS,
        span_elems=SPAN,
    )
    return st


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_fused_step_matches_fp32_torch(gdtype):
    case = _step_case(gdtype)
    assert len(case["shapes"]) > _max_tensors()
    got = _run_fused(case)
    again = _run_fused(case)
    # 1 - beta as the kernel forms it: in fp32
    one = torch.tensor(1.0)
    omb1 = float(one - torch.tensor(BETA1))
    omb2 = float(one - torch.tensor(BETA2))
    for i, shape in enumerate(case["shapes"]):
        g = case["grads"][i].float()
        p = case["masters"][i]
        t = case["steps"][i]
        m = BETA1 * _dequantize_ref(case["m"][i], case["ms"][i]) + omb1 * g
        v = BETA2 * _dequantize_ref(case["r"][i], case["rs"][i]) ** 2 + omb2 * g * g
        denom = (v / (1 - BETA2**t)).sqrt() + EPS
        ref_p = p - case["lrs"][i] * (
            m / (1 - BETA1**t) / denom + case["wds"][i] * p
        )
        torch.testing.assert_close(got["masters"][i], ref_p, rtol=1e-4, atol=1e-5)
        assert torch.equal(got["bf16"][i], got["masters"][i].bfloat16())
        for x, codes, scales in ((m, got["m"][i], got["ms"][i]),
                                 (v.sqrt(), got["r"][i], got["rs"][i])):
            assert codes.shape == shape and scales.shape == (shape[0], shape[1] // 256)
            ref_scales = x.view(shape[0], shape[1] // 256, 256).abs().amax(-1) / 448
            torch.testing.assert_close(scales, ref_scales, rtol=1e-6, atol=0)
            # half an e4m3 step of y = x / scale, normals and subnormals
            s = ref_scales.repeat_interleave(256, dim=-1)
            y = torch.where(s != 0, x / s, torch.zeros_like(x))
            bound = s * torch.maximum(
                y.abs() * 2.0**-4, torch.full_like(y, 2.0**-10)
            ) * (1 + 1e-5)
            err = (_dequantize_ref(codes, scales) - x).abs()
            assert (err <= bound).all(), (i, float((err / bound)[bound > 0].max()))
        for key in ("masters", "m", "ms", "r", "rs", "bf16"):
            assert torch.equal(got[key][i], again[key][i]), (key, i)
    # the special blocks are what they claim to be
    nine = case["shapes"].index((9, 256))
    assert not got["m"][nine][4].any() and not got["r"][nine][4].any()
    assert got["ms"][nine][4] == 0 and got["rs"][nine][4] == 0
    wide = got["m"][nine][7]
    assert ((wide & 0x78) == 0).any() and ((wide & 0x7F) == 0).any()


# ---------------------------------------------------------------------------
# 3. clipping and skipping
# ---------------------------------------------------------------------------


def _two_linear():
    return torch.nn.Sequential(
        torch.nn.Linear(256, 256), torch.nn.Linear(256, 256)
    )


def test_clip_norm_covers_both_kinds():
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    model = _two_linear().to(_dev()).bfloat16()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0, moments="fp8")
    refs = [p.detach().float().clone().requires_grad_(True) for p in model.parameters()]
    x = torch.randn(16, 256, device=_dev(), dtype=torch.bfloat16)
    totals = []
    for scale in (100.0, 1e-3):
        opt.zero_grad()
        (model(x).float().pow(2).mean() * scale).backward()
        for r, p in zip(refs, model.parameters()):
            r.grad = p.grad.float()
        total = torch.nn.utils.clip_grad_norm_(refs, 1.0)
        opt.step()
        torch.testing.assert_close(opt.last_grad_norm, total, rtol=1e-5, atol=0)
        totals.append(float(total))
    assert totals[0] > 1.0 and totals[-1] < 1.0, totals
    kinds = {("exp_avg_sq_root" in opt.state[p]) for p in model.parameters()}
    assert kinds == {True, False}  # weights fp8, biases fp32


def test_nonfinite_skips_update_fp8():
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    model = _two_linear().to(_dev()).bfloat16()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0, moments="fp8")
    x = torch.randn(16, 256, device=_dev(), dtype=torch.bfloat16)

    def backward():
        opt.zero_grad()
        model(x).float().pow(2).mean().backward()

    def snapshot():
        snap = []
        for p in model.parameters():
            snap.append(p.detach().clone())
            snap += [v.clone() for v in opt.state[p].values() if torch.is_tensor(v)]
        return snap

    backward()
    opt.step()  # state exists, moments non-zero
    before = snapshot()
    assert len(before) == 2 * 6 + 2 * 4
    backward()
    model[1].weight.grad.view(-1)[5] = float("inf")
    opt.step()
    assert not torch.isfinite(opt.last_grad_norm)
    for s, t in zip(snapshot(), before):
        assert torch.equal(s, t)
    # a following finite step updates normally
    backward()
    opt.step()
    assert torch.isfinite(opt.last_grad_norm)
    after = snapshot()
    assert all(not torch.equal(s, t) for s, t in zip(after, before))
    for s in after:
        if s.dtype == torch.uint8:
            s = _f8(s)
        assert torch.isfinite(s.float()).all()


# ---------------------------------------------------------------------------
# 4. model
# ---------------------------------------------------------------------------


def test_llama_fp8_moments_train_gpu():
    """10 clipped steps with FP8 moments against an fp32-moment twin on the
    same seeds. Measured with the CPU reference on these seeds: final loss
    1.49364 (fp32 moments) and 1.49964 (fp8), a gap of 0.0060 (0.0029 and
    0.0034 on seeds 1 and 2); twice that, 0.012, is allowed here."""
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import FusedAdamW

    def run(moments):
        torch.manual_seed(0)
        cfg = LlamaConfig(
            vocab_size=512, hidden_size=256, intermediate_size=512, n_layers=2,
            n_heads=4, n_kv_heads=2, max_seq_len=128, rope_base=10000.0,
        )
        model = LlamaForCausalLM(cfg).to(_dev()).bfloat16()
        model.rope_cos = model.rope_cos.float()
        model.rope_sin = model.rope_sin.float()
        opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.0,
                         max_grad_norm=1.0, moments=moments)
        ids = torch.randint(0, cfg.vocab_size, (2, 32), device=_dev())
        first = last = None
        for _ in range(10):
            loss = model(ids, ids.clone())
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert torch.isfinite(opt.last_grad_norm)
            first = first or loss.item()
            last = loss.item()
        return first, last, opt.state_nbytes()

    first32, last32, bytes32 = run("fp32")
    first8, last8, bytes8 = run("fp8")
    print(f"fp32 moments {first32:.5f} -> {last32:.5f}, {bytes32} B; "
          f"fp8 {first8:.5f} -> {last8:.5f}, {bytes8} B")
    assert last8 < first8 * 0.9, (first8, last8)
    # 6.03 / 12 for eligible parameters; the rest is a few hundred elements
    assert bytes8 < 0.55 * bytes32, (bytes8, bytes32)
    assert abs(last8 - last32) <= 0.012, (last8, last32)


# ---------------------------------------------------------------------------
# 5. degenerate blocks: tiny absmax, NaN
# ---------------------------------------------------------------------------


def _tiny_blocks():
    """[12, 256]: blocks whose absmax lies in or next to the range where
    absmax / 448 is a subnormal fp32 (or rounds to zero)."""
    edge = torch.tensor(448 * 2.0**-126, dtype=torch.float32)
    inf = torch.tensor(float("inf"))
    absmax = torch.stack([
        torch.tensor(v, dtype=torch.float32)
        for v in (1.4e-45, 3e-43, 1e-40, 1e-38, 5e-36, 6e-36, 1e-35, 1e-30)
    ] + [
        torch.nextafter(edge, -inf), edge, torch.nextafter(edge, inf),
        torch.nextafter(torch.nextafter(edge, inf), inf),
    ])
    gen = torch.Generator().manual_seed(5)
    u = (torch.rand(12, 256, generator=gen, dtype=torch.float64) * 2 - 1) * 10 ** (
        -3 * torch.rand(12, 256, generator=gen, dtype=torch.float64)
    )
    x = (u * absmax.double()[:, None]).float()
    x[:, 0] = absmax  # exactly
    return x


def test_quantize_subnormal_range_matches_reference_bitwise():
    from dlrover_amd.ops import fp8_block_quantize

    x = _tiny_blocks()
    ref_codes, ref_scales = fp8_block_quantize(x)  # CPU: the definition
    flushed = ref_scales[:, 0] == 0
    assert flushed.any() and not flushed.all()
    assert (x[flushed] != 0).any()  # flushed, not merely zero
    codes, scales = fp8_block_quantize(x.to(_dev()))
    assert torch.equal(scales.cpu().view(torch.int32), ref_scales.view(torch.int32))
    assert torch.equal(codes.cpu(), ref_codes)
    assert ((codes & 0x7F) != 0x7F).all()  # no NaN code


def test_nan_poisons_its_block_like_the_reference():
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    gen = torch.Generator().manual_seed(6)
    x = torch.randn(3, 256, generator=gen)
    x[1, 77] = float("nan")
    ref_codes, ref_scales = fp8_block_quantize(x)
    codes, scales = fp8_block_quantize(x.to(_dev()))
    assert torch.isnan(ref_scales[1]) and torch.isnan(scales[1])
    deq = fp8_block_dequantize(codes, scales).cpu()
    assert torch.isnan(deq[1]).all()
    assert torch.isnan(fp8_block_dequantize(ref_codes, ref_scales)[1]).all()
    for row in (0, 2):
        assert torch.equal(codes[row].cpu(), ref_codes[row])
        assert torch.equal(scales[row].cpu(), ref_scales[row])


def test_fused_step_flushes_decayed_moments():
    """Zero gradient on state whose exp_avg scale sits just above the
    smallest normal fp32: one more decay takes it below, the block is
    flushed, and the kernel agrees bitwise with the CPU reference step."""
    from dlrover_amd.ops import fp8_block_quantize, fused_adamw_fp8_multi_step

    gen = torch.Generator().manual_seed(7)
    m = torch.randn(2, 256, generator=gen)
    m = m / m.abs().amax(-1, keepdim=True) * torch.tensor([[5.5e-36], [1e-3]])
    root = torch.rand(2, 256, generator=gen) * 1e-3
    master = torch.randn(2, 256, generator=gen)

    def run(dev):
        mc, ms = (t.to(dev) for t in fp8_block_quantize(m))
        rc, rs = (t.to(dev) for t in fp8_block_quantize(root))
        p = master.clone().to(dev)
        pb = torch.zeros_like(p, dtype=torch.bfloat16)
        fused_adamw_fp8_multi_step(
            [p], [torch.zeros(2, 256, device=dev)], [mc], [ms], [rc], [rs], [pb],
            [1e-3], [0.1], [800], BETA1, BETA2, EPS,
        )
        return [t.cpu() for t in (p, mc, ms, rc, rs, pb)]

    assert fp8_block_quantize(m)[1][0, 0] >= 2.0**-126  # not flushed yet
    got, ref = run(_dev()), run("cpu")
    assert got[2][0, 0] == 0 and not got[1][0].any()  # flushed now
    assert got[2][1, 0] > 0 and got[1][1].any()
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    torch.testing.assert_close(got[4], ref[4], rtol=1e-6, atol=0)
    torch.testing.assert_close(got[0], ref[0], rtol=1e-4, atol=1e-5)
    assert all(torch.isfinite(t.float()).all() for t in (got[0], got[2], got[4], got[5]))
