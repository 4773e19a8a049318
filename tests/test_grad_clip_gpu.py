"""GPU: multi-tensor squared norm, batched AdamW and clipped FusedAdamW.

Small shapes on purpose: span_elems=2048 forces several spans per tensor,
tails that are no multiple of 8, a 2-byte-aligned view (scalar path) and
more tensors than one launch takes.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SPAN = 2048
NUMELS = [0, 1, 7, 8, 9, 255, 2048, 2049, 5003]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from dlrover_amd.ops.api import hip_ops

    hip_ops()  # raises on a GPU box if the extension didn't build


def _dev():
    return torch.device("cuda:0")


def _max_tensors():
    from dlrover_amd.ops.api import hip_ops

    return hip_ops().MT_MAX_TENSORS


def _offset_view(n, dtype, gen):
    """Contiguous n-element view one element into a larger buffer: 2-byte
    (bf16) or 4-byte (fp32) aligned only."""
    buf = torch.randn(n + 16, device=_dev(), generator=gen).to(dtype)
    view = buf[1 : 1 + n]
    assert view.data_ptr() % 16 != 0
    return view


def _tensor_list(gen, dtype_of):
    """The shape list of the issue; dtype_of(i) picks each tensor's dtype."""
    ts = [
        torch.randn(n, device=_dev(), generator=gen).to(dtype_of(i))
        for i, n in enumerate(NUMELS)
    ]
    ts.append(_offset_view(2049, dtype_of(1), gen))
    while len(ts) <= _max_tensors():  # a second launch is needed
        ts.append(torch.randn(3, device=_dev(), generator=gen).to(dtype_of(len(ts))))
    return ts


def test_sq_norm_small_shapes():
    from dlrover_amd.ops import grad_sq_norm
    from dlrover_amd.ops.api import grad_sq_norm_slots

    gen = torch.Generator(device=_dev()).manual_seed(0)
    alt = lambda i: torch.bfloat16 if i % 2 else torch.float32  # noqa: E731
    ts = _tensor_list(gen, alt)
    assert ts[len(NUMELS)].dtype == torch.bfloat16  # the 2-byte-aligned view
    ts.append(_offset_view(2049, torch.float32, gen))
    assert len(ts) > _max_tensors()

    slots = grad_sq_norm_slots(ts, SPAN)
    assert slots == sum(-(-t.numel() // SPAN) for t in ts)
    outs = []
    for _ in range(2):
        # NaN everywhere: every consumed slot must have been written, and
        # nothing may rely on zero-initialised memory
        partials = torch.full((slots,), float("nan"), device=_dev())
        out = torch.full((1,), float("nan"), device=_dev())
        grad_sq_norm(ts, out=out, partials=partials, span_elems=SPAN)
        assert not torch.isnan(partials).any()
        outs.append(out)
    ref = sum(t.double().pow(2).sum() for t in ts).sqrt()
    torch.testing.assert_close(outs[0][0].sqrt().double(), ref, rtol=1e-5, atol=0)
    assert torch.equal(outs[0], outs[1])  # bitwise reproducible

    # automatic span: same value, own workspace size
    auto = grad_sq_norm(ts)
    torch.testing.assert_close(auto[0].sqrt().double(), ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_mt_adamw_matches_per_param_kernel(gdtype):
    from dlrover_amd.ops import fused_adamw_multi_step, fused_adamw_step

    gen = torch.Generator(device=_dev()).manual_seed(1)
    shapes = [t.numel() for t in _tensor_list(gen, lambda i: torch.float32)]
    view_at = len(NUMELS)  # the gradient that is an offset view
    odd = 8  # the 5003-element tensor: its own step, lr and weight decay
    n = len(shapes)
    assert n > _max_tensors()

    def state():
        g2 = torch.Generator(device=_dev()).manual_seed(2)
        masters = [torch.randn(k, device=_dev(), generator=g2) for k in shapes]
        ms = [torch.zeros_like(p) for p in masters]
        vs = [torch.zeros_like(p) for p in masters]
        pbs = [p.bfloat16() for p in masters]
        return masters, ms, vs, pbs

    a, b = state(), state()
    lrs = [1e-2] * n
    wds = [0.1] * n
    lrs[odd], wds[odd] = 3e-3, 0.0
    for step in range(1, 5):
        grads = [
            torch.randn(k, device=_dev(), generator=gen).to(gdtype) for k in shapes
        ]
        view = _offset_view(shapes[view_at], gdtype, gen)
        grads[view_at] = view
        steps = [step] * n
        steps[odd] = step + 7
        fused_adamw_multi_step(
            a[0], grads, a[1], a[2], a[3], lrs, wds, steps, 0.9, 0.95, 1e-8,
            span_elems=SPAN,
        )
        for i in range(n):
            if shapes[i] == 0:
                continue
            # the per-parameter kernel gets an aligned copy of the view
            g = grads[i].clone() if i == view_at else grads[i]
            fused_adamw_step(
                b[0][i], g, b[1][i], b[2][i], b[3][i], lrs[i], 0.9, 0.95,
                1e-8, wds[i], steps[i],
            )
    for i in range(n):
        for x, y in zip(a[:3], b[:3]):
            torch.testing.assert_close(x[i], y[i], rtol=1e-6, atol=1e-7)
        # bf16 copy is the kernel's own master rounded to bf16, exactly
        assert torch.equal(a[3][i], a[0][i].bfloat16())


def _two_linear():
    return torch.nn.Sequential(
        torch.nn.Linear(256, 256), torch.nn.Linear(256, 256)
    )


def test_clip_matches_torch_gpu():
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    hp = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    model = _two_linear().to(_dev()).bfloat16()
    opt = FusedAdamW(model.parameters(), max_grad_norm=1.0, **hp)
    refs = [p.detach().float().clone().requires_grad_(True) for p in model.parameters()]
    ref_opt = torch.optim.AdamW(refs, **hp)
    x = torch.randn(16, 256, device=_dev(), dtype=torch.bfloat16)
    totals = []
    for scale in (100.0, 100.0, 100.0, 1e-3, 1e-3):
        opt.zero_grad()
        (model(x).float().pow(2).mean() * scale).backward()
        for r, p in zip(refs, model.parameters()):
            r.grad = p.grad.float()  # the same bf16 gradients, upcast
        total = torch.nn.utils.clip_grad_norm_(refs, 1.0)
        ref_opt.step()
        opt.step()
        torch.testing.assert_close(opt.last_grad_norm, total, rtol=1e-5, atol=0)
        totals.append(float(total))
        for r, p in zip(refs, model.parameters()):
            torch.testing.assert_close(
                opt.state[p]["master_param"], r.detach(), rtol=1e-4, atol=1e-5
            )
            assert torch.equal(p.detach(), opt.state[p]["master_param"].bfloat16())
    assert totals[0] > 1.0 and totals[-1] < 1.0, totals


def test_nonfinite_skips_update_gpu():
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    model = _two_linear().to(_dev()).bfloat16()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0)
    x = torch.randn(16, 256, device=_dev(), dtype=torch.bfloat16)

    def backward():
        opt.zero_grad()
        model(x).float().pow(2).mean().backward()

    def snapshot():
        snap = []
        for p in model.parameters():
            st = opt.state[p]
            snap += [p.detach().clone(), st["master_param"].clone(),
                     st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
        return snap

    backward()
    opt.step()  # state exists, moments non-zero
    before = snapshot()
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
    assert all(torch.isfinite(s).all() for s in after)


def test_clip_graph_capture_gpu():
    """capture_graph=True with clipping: the coefficient lives on the device,
    so the replayed graph recomputes it every step. Inputs alternate between
    two scales so that, replayed steps included, some steps clip and some do
    not (threshold 0.03 sits between the two groups' norms, about 0.045 and
    0.018 at step 110 on the fp32 reference path)."""
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    max_norm = 0.03
    m1 = torch.nn.Linear(64, 64).cuda().bfloat16()
    m2 = torch.nn.Linear(64, 64).cuda().bfloat16()
    m2.load_state_dict(m1.state_dict())
    o1 = FusedAdamW(m1.parameters(), lr=1e-3, weight_decay=0.0,
                    max_grad_norm=max_norm)
    o2 = FusedAdamW(m2.parameters(), lr=1e-3, weight_decay=0.0,
                    max_grad_norm=max_norm, capture_graph=True)
    x = torch.randn(8, 64).bfloat16().cuda()
    xs = (x * 4.0, x)

    def one(i):
        for m, o in ((m1, o1), (m2, o2)):
            loss = m(xs[i % 2]).float().pow(2).mean()
            o.zero_grad()
            loss.backward()
            o.step()

    for i in range(110):
        one(i)
    assert o2._graph is not None, "graph was never captured"
    replayed = []
    for i in range(110, 115):
        one(i)
        replayed.append(torch.stack([o1.last_grad_norm, o2.last_grad_norm]))
    torch.testing.assert_close(
        m1.weight.float(), m2.weight.float(), rtol=2e-2, atol=2e-3
    )
    assert o2.state[m2.weight]["step"] == 115
    replayed = torch.stack(replayed)  # [5, 2]
    torch.testing.assert_close(replayed[:, 0], replayed[:, 1], rtol=2e-2, atol=2e-3)
    assert (replayed > max_norm).any() and (replayed < max_norm).any(), replayed


def test_llama_tiny_clip_step_gpu():
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import FusedAdamW

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    model = LlamaForCausalLM(cfg).to(_dev()).bfloat16()
    model.rope_cos = model.rope_cos.float()
    model.rope_sin = model.rope_sin.float()
    opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.0,
                     max_grad_norm=1.0)
    ids = torch.randint(0, cfg.vocab_size, (2, 32), device=_dev())
    first = last = None
    norms = []
    for _ in range(10):
        loss = model(ids, ids.clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        norms.append(opt.last_grad_norm.clone())
        first = first or loss.item()
        last = loss.item()
    assert torch.isfinite(torch.stack(norms)).all(), norms
    assert last < first * 0.9, (first, last)
