"""GPU: stochastic rounding bitwise against the CPU definition, its mean, the
master-free optimizer step against an fp32 torch reference, and its
independence of the launch split and of a save / resume."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA1, BETA2, EPS = 0.9, 0.95, 1e-8
SHAPES = [(256, 256), (3, 256)]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from dlrover_amd.ops.api import hip_ops

    hip_ops()  # raises on a GPU box if the extension didn't build


@pytest.mark.parametrize("numel", [1, 7, 8, 9, 4099])
@pytest.mark.parametrize("key", [(3, 0, 0), (2**40 + 12345, 17, 1000)])
def test_round_matches_cpu_bitwise(numel, key):
    from dlrover_amd.ops import stochastic_round_bf16

    gen = torch.Generator().manual_seed(numel)
    buf = torch.randn(numel + 1, generator=gen) * 10 ** (
        torch.rand(numel + 1, generator=gen) * 84 - 44  # subnormals included
    )
    big = torch.finfo(torch.float32).max
    special = torch.tensor([big, -big, float("inf"), -float("inf"), float("nan"),
                            0.0, -0.0, 1.0, 1e-45])
    for offset in (0, 1):  # 1: a view that is not 16-byte aligned
        x = buf[offset : offset + numel]
        x[:: max(numel // special.numel(), 1)][: special.numel()] = special[:numel]
        ref = stochastic_round_bf16(x, *key)
        xd = buf.to(DEV)[offset : offset + numel]
        assert xd.data_ptr() % 16 == 4 * offset
        got = stochastic_round_bf16(xd, *key)
        assert torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))


def test_unbiased_where_nearest_is_not():
    from dlrover_amd.ops import stochastic_round_bf16

    n = 2**20
    x = torch.full((n,), 1 + 2.0**-9, device=DEV)
    assert (x.bfloat16() == 1).all()  # round-to-nearest moves none of them
    got = stochastic_round_bf16(x, seed=1).float()
    assert ((got == 1) | (got == 1 + 2.0**-7)).all()
    frac = float((got != 1).float().mean())
    assert abs(frac - 0.25) <= 4 * (0.25 * 0.75 / n) ** 0.5, frac


# ---------------------------------------------------------------------------
# the optimizer
# ---------------------------------------------------------------------------


def _grads(step, gdtype, shapes=SHAPES):
    gen = torch.Generator(device=DEV).manual_seed(100 + step)
    return [(torch.randn(s, device=DEV, generator=gen) * 1e-2).to(gdtype) for s in shapes]


def _make(init, offset=0, **kw):
    """Parameters holding copies of ``init`` (at ``offset`` elements into a
    larger buffer: 1 makes them misaligned) and their optimizer."""
    from dlrover_amd.ops import FusedAdamW

    ps = []
    for w in init:
        buf = torch.empty(w.numel() + offset, device=w.device, dtype=w.dtype)
        ps.append(torch.nn.Parameter(buf[offset:].view(w.shape).copy_(w)))
        ps[-1].grad_dtype = None  # fp32 gradients on bf16 weights are allowed
    return ps, FusedAdamW(ps, lr=kw.pop("lr", 1e-2), betas=(BETA1, BETA2), eps=EPS, **kw)


def _moments(st, like):
    """fp32 (exp_avg, exp_avg_sq) of a state entry in either format."""
    from dlrover_amd.ops import fp8_block_dequantize

    if "exp_avg" not in st:
        return torch.zeros_like(like), torch.zeros_like(like)
    if "exp_avg_sq_root" in st:
        root = fp8_block_dequantize(st["exp_avg_sq_root"], st["exp_avg_sq_root_scale"])
        return fp8_block_dequantize(st["exp_avg"], st["exp_avg_scale"]), root**2
    return st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def _reference_step(w, g, m, v, t, lr, wd):
    """One AdamW step in fp32 torch; 1 - beta as the kernels form it."""
    one = torch.tensor(1.0)
    g = g.float()
    m = BETA1 * m + float(one - torch.tensor(BETA1)) * g
    v = BETA2 * v + float(one - torch.tensor(BETA2)) * g * g
    return w - lr * (m / (1 - BETA1**t) / ((v / (1 - BETA2**t)).sqrt() + EPS) + wd * w)


def _bf16_ulp(*ws):
    """Spacing of bf16 at the largest magnitude of the arguments."""
    big = torch.stack([w.abs() for w in ws]).amax(0)
    return (big.view(torch.int32) & 0x7F800000).view(torch.float32) * 2.0**-7


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("moments", ["fp32", "fp8"])
def test_step_matches_fp32_reference(moments, gdtype, steps):
    gen = torch.Generator(device=DEV).manual_seed(0)
    init = [torch.randn(s, device=DEV, generator=gen).bfloat16() for s in SHAPES]
    kw = dict(moments=moments, weight_decay=0.1, multi_tensor=True)
    ps, opt = _make(init, master_weights=False, sr_seed=9, **kw)
    qs, base = _make(init, **kw)
    for t in range(1, steps + 1):
        gs = _grads(t, gdtype)
        refs = []
        for p, g in zip(ps, gs):
            w = p.detach().float()
            refs.append(_reference_step(w, g, *_moments(opt.state[p], w), t, 1e-2, 0.1))
        for p, q, g in zip(ps, qs, gs):
            p.grad, q.grad = g, g
        opt.step()
        base.step()
        for p, w_ref in zip(ps, refs):
            got = p.detach().float()
            tol = _bf16_ulp(w_ref, got) + 1e-4 * w_ref.abs() + 1e-5
            assert ((got - w_ref).abs() <= tol).all()
            assert not torch.equal(got, w_ref.bfloat16().float())  # not RNE
    # the gradients were given, so the moments do not depend on the weights
    for p, q in zip(ps, qs):
        assert "master_param" not in opt.state[p] and "master_param" in base.state[q]
        assert ("exp_avg_sq_root" in opt.state[p]) == (moments == "fp8")
        pairs = zip(_moments(opt.state[p], p), _moments(base.state[q], q))
        for second, (a, b) in enumerate(pairs):
            if moments == "fp32":
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
                continue
            # codes at most one e4m3 step apart: 2**-3 of the value, or
            # 2**-9 of the block scale among subnormals (roots compared)
            a, b = (a.sqrt(), b.sqrt()) if second else (a, b)
            b = b.view(-1, 256)
            scale = b.abs().amax(-1, keepdim=True) / 448
            tol = (2.0**-3 * b.abs() + 2.0**-9 * scale) * (1 + 1e-5)
            assert ((a.view(-1, 256) - b).abs() <= tol).all()


@pytest.mark.parametrize("moments", ["fp32", "fp8"])
def test_sub_ulp_updates_move_the_mean(moments):
    """Weights all 1 and lr = 2**-10: every first-step update is at most
    2**-10, an eighth (upwards) or a quarter (downwards) of the bf16 spacing,
    which round-to-nearest loses entirely."""
    init = [torch.ones(s, device=DEV, dtype=torch.bfloat16) for s in SHAPES]
    ps, opt = _make(init, lr=2.0**-10, weight_decay=0.0, moments=moments,
                    master_weights=False, sr_seed=4)
    gs = _grads(1, torch.bfloat16)
    w_ref = torch.cat([
        _reference_step(torch.ones_like(g, dtype=torch.float32), g,
                        torch.zeros_like(g, dtype=torch.float32),
                        torch.zeros_like(g, dtype=torch.float32), 1, 2.0**-10, 0.0).reshape(-1)
        for g in gs
    ])
    assert ((w_ref - 1).abs() <= 2.0**-9).all() and (w_ref.bfloat16() == 1).all()
    for p, g in zip(ps, gs):
        p.grad = g
    opt.step()
    got = torch.cat([p.detach().float().reshape(-1) for p in ps])
    # per element: up (away from zero) with probability q, else truncation
    q = (w_ref.view(torch.int32) & 0xFFFF).double() / 65536
    ulp = torch.where(w_ref < 1, 2.0**-8, 2.0**-7).double()
    sigma = float((q * (1 - q) * ulp**2).sum().sqrt()) / w_ref.numel()
    moved, want = float((got.double() - 1).mean()), float((w_ref.double() - 1).mean())
    print(f"mean change {moved:.3e}, fp32 update {want:.3e}, sigma {sigma:.2e}")
    assert (got != 1).any() and abs(moved - want) <= 4 * sigma


def test_split_invariance_and_resume():
    shapes = SHAPES + [(300,)]  # fp8 and fp32 moments, a tail shorter than 8
    gen = torch.Generator(device=DEV).manual_seed(2)
    init = [torch.randn(s, device=DEV, generator=gen).bfloat16() for s in shapes]

    def run(seed, spans=(0, 0), resume=False, offset=0):
        kw = dict(moments="fp8", master_weights=False, sr_seed=seed)
        ps, opt = _make(init, offset, **kw)
        opt._span_elems, opt._span_elems_fp8 = spans
        for t in range(1, 4):
            if resume and t == 3:
                sd = opt.state_dict()
                ps, opt = _make([p.detach() for p in ps], **kw)
                opt.load_state_dict(sd)
            for p, g in zip(ps, _grads(t, torch.bfloat16, shapes)):
                p.grad = g
            opt.step()
        state = [v for p in ps for v in opt.state[p].values() if torch.is_tensor(v)]
        return [p.detach() for p in ps] + state

    whole = run(11)
    # other spans with misaligned weights (scalar accesses), and a resume
    for other in (run(11, spans=(64, 256), offset=1), run(11, resume=True)):
        assert len(other) == len(whole)
        assert all(torch.equal(a, b) for a, b in zip(whole, other))
    assert not any(torch.equal(a, b) for a, b in zip(whole[:3], run(12)[:3]))
