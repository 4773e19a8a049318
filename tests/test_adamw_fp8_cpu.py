"""CPU: FP8 block-scaled moments of FusedAdamW — the reference quantiser, the
optimizer's state layout, its conversions and its way through checkpoints."""

import os
import time

import torch

from dlrover_amd.ops import FusedAdamW

FP8_KEYS = (
    "exp_avg", "exp_avg_scale", "exp_avg_sq_root", "exp_avg_sq_root_scale",
)


def _rounding_bound(x, scales):
    """Half an e4m3 step of y = x / scale (normals: |y| * 2**-4 bounds half
    a step of 2**(e-3); subnormals: half of 2**-9), back in x's units."""
    s = scales.repeat_interleave(256, dim=-1)
    y = torch.where(s != 0, x / s, torch.zeros_like(x))
    return s * torch.maximum(y.abs() * 2.0**-4, torch.full_like(y, 2.0**-10)) * (
        1 + 1e-5
    )


def test_reference_quantiser_rounding_bound():
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    gen = torch.Generator().manual_seed(0)
    # 8 decades inside every block, so subnormals and flushes occur
    x = torch.randn(64, 1024, generator=gen) * 10 ** (
        torch.rand(64, 1024, generator=gen) * 8 - 6
    )
    x[3, 256:512] = 0.0  # an all-zero block
    codes, scales = fp8_block_quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape
    assert scales.dtype == torch.float32 and scales.shape == (64, 4)
    torch.testing.assert_close(
        scales, x.view(64, 4, 256).abs().amax(-1) / 448, rtol=0, atol=0
    )
    assert scales[3, 1] == 0 and not codes[3, 256:512].any()
    deq = fp8_block_dequantize(codes, scales)
    assert torch.isfinite(deq).all()
    err = (deq - x).abs()
    assert (err <= _rounding_bound(x, scales)).all()
    # the block maximum itself is represented by +-448
    assert ((codes & 0x7F) == 0x7E).view(64, 4, 256).any(-1)[scales != 0].all()
    # subnormal codes were produced, i.e. the bound's second branch was used
    assert ((codes & 0x78) == 0).any()


def _params():
    torch.manual_seed(0)
    shapes = {"w": (4, 256), "norm": (256,), "odd": (4, 128), "empty": (0, 256)}
    return {k: torch.nn.Parameter(torch.randn(*s)) for k, s in shapes.items()}


def _step(opt, params, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen)
    opt.step()


def test_eligibility_and_steps_cpu():
    ps = _params()
    opt = FusedAdamW(ps.values(), lr=1e-2, moments="fp8")
    before = {k: p.detach().clone() for k, p in ps.items()}
    for seed in range(3):
        _step(opt, ps.values(), seed)
    for k in ("w", "empty"):
        st = opt.state[ps[k]]
        rows = ps[k].shape[0]
        assert set(st) == {"step", "master_param", *FP8_KEYS}, k
        assert st["master_param"].dtype == torch.float32
        for key in ("exp_avg", "exp_avg_sq_root"):
            assert st[key].dtype == torch.uint8
            assert st[key].shape == (rows, 256)
            assert st[key + "_scale"].dtype == torch.float32
            assert st[key + "_scale"].shape == (rows, 1)
    for k in ("norm", "odd"):
        st = opt.state[ps[k]]
        assert set(st) == {"step", "master_param", "exp_avg", "exp_avg_sq"}, k
        assert st["exp_avg"].dtype == torch.float32
    for k in ("w", "norm", "odd"):
        assert not torch.equal(ps[k].detach(), before[k])
        assert torch.isfinite(ps[k]).all()
        assert opt.state[ps[k]]["step"] == 3
    assert opt.state[ps["w"]]["exp_avg"].any()
    # 4 + 1 + 1 bytes per element and two scales per block, against 12
    w_bytes = 4 * 256 * 6 + 4 * 2 * 4
    rest = (256 + 4 * 128) * 12
    assert opt.state_nbytes() == w_bytes + rest

    # the default keeps its state keys
    ps32 = _params()
    opt32 = FusedAdamW(ps32.values(), lr=1e-2)
    _step(opt32, ps32.values(), 0)
    for p in ps32.values():
        assert set(opt32.state[p]) == {"step", "master_param", "exp_avg", "exp_avg_sq"}


def test_fp8_tracks_fp32_moments_cpu():
    """Three steps with the same gradients: the stored moments stay within
    the rounding bound (growing by at most beta per step of carried error) of
    the fp32-moment optimizer's."""
    from dlrover_amd.ops import fp8_block_dequantize

    a, b = _params(), _params()
    o8 = FusedAdamW([a["w"]], lr=1e-2, moments="fp8")
    o32 = FusedAdamW([b["w"]], lr=1e-2, multi_tensor=True)
    for seed in range(3):
        _step(o8, [a["w"]], seed)
        _step(o32, [b["w"]], seed)
    s8, s32 = o8.state[a["w"]], o32.state[b["w"]]
    m = fp8_block_dequantize(s8["exp_avg"], s8["exp_avg_scale"])
    r = fp8_block_dequantize(s8["exp_avg_sq_root"], s8["exp_avg_sq_root_scale"])
    # three roundings, each at most 2**-4 relative to the block's absmax
    for got, ref in ((m, s32["exp_avg"]), (r, s32["exp_avg_sq"].sqrt())):
        tol = 3 * 2.0**-4 * ref.abs().amax(-1, keepdim=True)
        assert ((got - ref).abs() <= tol).all()
    torch.testing.assert_close(a["w"], b["w"], rtol=0, atol=3e-2)


def test_state_dict_roundtrip(tmp_path):
    ps = _params()
    opt = FusedAdamW(ps.values(), lr=1e-2, moments="fp8")
    _step(opt, ps.values(), 0)
    path = tmp_path / "opt.pt"
    torch.save(opt.state_dict(), path)
    fresh = FusedAdamW(_params().values(), lr=1e-2, moments="fp8")
    fresh.load_state_dict(torch.load(path, weights_only=False))
    for p, q in zip(ps.values(), fresh.param_groups[0]["params"]):
        st, new = opt.state[p], fresh.state[q]
        assert set(st) == set(new)
        for k, v in st.items():
            if torch.is_tensor(v):
                assert new[k].dtype == v.dtype and torch.equal(new[k], v), k
            else:
                assert new[k] == v


def test_load_converts_between_formats():
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    ps32 = _params()
    opt32 = FusedAdamW(ps32.values(), lr=1e-2)
    _step(opt32, ps32.values(), 0)
    _step(opt32, ps32.values(), 1)
    w32 = opt32.state[ps32["w"]]

    # fp32 checkpoint -> fp8 optimizer: quantised, exp_avg_sq through sqrt
    ps8 = _params()
    opt8 = FusedAdamW(ps8.values(), lr=1e-2, moments="fp8")
    opt8.load_state_dict(opt32.state_dict())
    w8 = opt8.state[ps8["w"]]
    assert set(w8) == {"step", "master_param", *FP8_KEYS}
    assert torch.equal(w8["master_param"], w32["master_param"])
    assert w8["step"] == 2
    for key, src in (("exp_avg", w32["exp_avg"]),
                     ("exp_avg_sq_root", w32["exp_avg_sq"].sqrt())):
        codes, scales = fp8_block_quantize(src)
        assert torch.equal(w8[key], codes)
        assert torch.equal(w8[key + "_scale"], scales)
    # ineligible parameters are untouched
    for k in ("norm", "odd"):
        for key in ("master_param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt8.state[ps8[k]][key], opt32.state[ps32[k]][key])
    _step(opt8, ps8.values(), 2)  # and the optimizer goes on from there

    # fp8 checkpoint -> fp32 optimizer: dequantised and squared
    opt8b = FusedAdamW(_params().values(), lr=1e-2, moments="fp8")
    opt8b.load_state_dict(opt32.state_dict())
    back_ps = _params()
    back = FusedAdamW(back_ps.values(), lr=1e-2)
    back.load_state_dict(opt8b.state_dict())
    wb = back.state[back_ps["w"]]
    assert set(wb) == {"step", "master_param", "exp_avg", "exp_avg_sq"}
    codes, scales = fp8_block_quantize(w32["exp_avg"])
    assert torch.equal(wb["exp_avg"], fp8_block_dequantize(codes, scales))
    codes, scales = fp8_block_quantize(w32["exp_avg_sq"].sqrt())
    assert torch.equal(wb["exp_avg_sq"], fp8_block_dequantize(codes, scales) ** 2)
    assert wb["exp_avg"].dtype == wb["exp_avg_sq"].dtype == torch.float32
    _step(back, back_ps.values(), 2)


def test_ucp_concat_restores_unsplit_state():
    from dlrover_amd.trainer.flash_checkpoint import ucp

    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(8, 256))
    opt = FusedAdamW([p], lr=1e-2, moments="fp8")
    _step(opt, [p], 0)
    full = opt.state_dict()

    def shard(lo, hi):
        st = {
            k: (v[lo:hi].clone() if torch.is_tensor(v) else v)
            for k, v in full["state"][0].items()
        }
        return {"optimizer": {"state": {0: st},
                              "param_groups": full["param_groups"]}}

    merged = ucp._concat_optim_states([shard(0, 5), shard(5, 8)])
    assert set(merged["state"][0]) == set(full["state"][0])
    for k, v in full["state"][0].items():
        got = merged["state"][0][k]
        if torch.is_tensor(v):
            assert got.dtype == v.dtype and torch.equal(got, v), k
        else:
            assert got == v
    # and a rank's new slice is a row range of every tensor
    for k in FP8_KEYS:
        piece = ucp._slice_for_rank(merged["state"][0][k], [0, 3], 1, 5)
        assert torch.equal(piece, full["state"][0][k][3:8])


def test_checkpoint_engine_roundtrip(tmp_path, monkeypatch):
    from dlrover_amd.trainer.flash_checkpoint.engine import (
        ShardedCheckpointEngine,
    )

    # a shared-memory segment of this test's own
    monkeypatch.setenv("ELASTIC_JOB_NAME", f"fp8{os.getpid()}_{time.time_ns()}")
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        torch.nn.Linear(256, 8, bias=True), torch.nn.Linear(8, 4)
    ).bfloat16()
    opt = FusedAdamW(model.parameters(), lr=1e-2, moments="fp8")
    x = torch.randn(4, 256).bfloat16()
    for _ in range(2):
        opt.zero_grad()
        model(x).float().pow(2).mean().backward()
        opt.step()
    w = model[0].weight
    assert "exp_avg_sq_root" in opt.state[w]
    saved = {
        p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
        for p, st in opt.state.items()
    }
    weights = [p.detach().clone() for p in model.parameters()]

    eng = ShardedCheckpointEngine(str(tmp_path / "ckpt"))
    try:
        eng.save_to_memory(3, eng.gather_state_dict(model, opt))
        # move on, so that the restore has something to undo
        opt.zero_grad()
        model(x * 2).float().pow(2).mean().backward()
        opt.step()
        assert not torch.equal(opt.state[w]["exp_avg"], saved[w]["exp_avg"])
        assert eng.restore_into(model, opt) is not None
    finally:
        eng.shm_handler.unlink()
    for p, st in saved.items():
        assert set(opt.state[p]) == set(st)
        for k, v in st.items():
            got = opt.state[p][k]
            if torch.is_tensor(v):
                assert got.dtype == v.dtype and torch.equal(got, v), k
            else:
                assert got == v
    for p, before in zip(model.parameters(), weights):
        assert torch.equal(p.detach(), before)


def test_small_second_moment_does_not_flush():
    """The hazard that storing sqrt(v) instead of v removes. A 64x256
    least-squares layer whose input features span 3.5 decades (so v spans 7
    inside every block) and whose gradient vanishes on two steps of three (so
    both moments decay between refreshes). Stored directly, a small v would
    flush to zero while its m survives and the update m_hat / (0 + eps)
    would be 10^3-10^4 times the fp32 one; with the root stored, the largest
    per-element |dp| / lr must stay within 2x of the fp32-moment run."""
    lr = 1e-3

    def run(moments):
        gen = torch.Generator().manual_seed(0)
        feat = 10 ** (-3.5 * torch.arange(256) / 255)
        x = torch.randn(32, 256, generator=gen) * feat
        w_true = torch.randn(64, 256, generator=gen)
        y = x @ w_true.t()
        w = torch.nn.Parameter(torch.zeros(64, 256))
        kw = dict(moments="fp8") if moments == "fp8" else dict(multi_tensor=True)
        opt = FusedAdamW([w], lr=lr, weight_decay=0.0, **kw)
        worst = 0.0
        for step in range(90):
            opt.zero_grad()
            loss = (w @ x.t() - y.t()).pow(2).mean()
            # the gradient is exactly zero on two steps of three
            (loss * (1.0 if step % 3 == 0 else 0.0)).backward()
            before = w.detach().clone()
            opt.step()
            worst = max(worst, float((w.detach() - before).abs().max()) / lr)
        return worst

    w32, w8 = run("fp32"), run("fp8")
    print(f"largest |dp|/lr: fp32 moments {w32:.4f}, fp8 moments {w8:.4f}")
    assert w32 > 0
    assert w8 <= 2 * w32, (w8, w32)


def _tiny_blocks():
    """[12, 256]: blocks whose absmax lies in or next to the range where
    absmax / 448 is a subnormal fp32 (or rounds to zero)."""
    flt_min = 2.0**-126
    edge = torch.tensor(448 * flt_min, dtype=torch.float32)
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
    u[:, 0] = 1.0
    x = (u * absmax.double()[:, None]).float()
    x[:, 0] = absmax  # exactly
    return x


def test_quantiser_flushes_degenerate_blocks():
    """absmax / 448 below the smallest normal fp32: the block is flushed
    (scale 0, codes 0); every other block keeps |x / scale| <= 448."""
    from dlrover_amd.ops import fp8_block_dequantize, fp8_block_quantize

    x = _tiny_blocks()
    codes, scales = fp8_block_quantize(x)
    flt_min = 2.0**-126
    want_zero = (x.abs().amax(-1) / 448 < flt_min)[:, None]
    assert want_zero.any() and not want_zero.all()
    assert torch.equal(scales == 0, want_zero)
    assert (scales[~want_zero] >= flt_min).all()
    assert not codes[want_zero[:, 0]].any()
    assert ((codes & 0x7F) != 0x7F).all()  # no NaN code
    # kept blocks: the maximum is +-448 and the rounding bound holds
    assert ((codes[~want_zero[:, 0], 0] & 0x7F) == 0x7E).all()
    deq = fp8_block_dequantize(codes, scales)
    assert torch.isfinite(deq).all()
    keep = ~want_zero[:, 0]
    assert ((deq - x).abs()[keep] <= _rounding_bound(x, scales)[keep]).all()


def test_zero_gradient_decay_stays_finite():
    """A row that gets a gradient once and then none (a token that stops
    occurring): its moments decay through fp32's subnormal range. State and
    weights must stay finite, and the row ends flushed."""
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(2, 256))
    opt = FusedAdamW([p], lr=1e-3, moments="fp8")
    gen = torch.Generator().manual_seed(1)
    for step in range(1600):
        g = torch.randn(2, 256, generator=gen)
        if step > 0:
            g[1] = 0.0
        p.grad = g
        opt.step()
        if step % 100 == 0 or step > 700:
            st = opt.state[p]
            for key in ("exp_avg", "exp_avg_sq_root"):
                assert ((st[key] & 0x7F) != 0x7F).all(), (step, key)
                assert torch.isfinite(st[key + "_scale"]).all(), (step, key)
            assert torch.isfinite(p).all(), step
    st = opt.state[p]
    assert st["exp_avg_scale"][1, 0] == 0 and not st["exp_avg"][1].any()
    assert st["exp_avg_scale"][0, 0] > 0 and st["exp_avg"][0].any()
    assert torch.isfinite(st["master_param"]).all()


def test_zero_row_dtensor_shard_is_eligible():
    """Eligibility comes from the GLOBAL shape: rank 1 of a Shard(0)
    placement of a [1, 256] parameter over two ranks holds 0 rows and must
    still keep fp8 state (shaped like its empty shard)."""
    import torch.distributed as dist
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import DTensor, Shard
    from torch.testing._internal.distributed.fake_pg import FakeStore

    assert not dist.is_initialized()
    dist.init_process_group("fake", store=FakeStore(), rank=1, world_size=2)
    try:
        mesh = init_device_mesh("cpu", (2,))

        def shard(cols):
            return DTensor.from_local(
                torch.zeros(0, cols), mesh, [Shard(0)], run_check=False,
                shape=torch.Size([1, cols]), stride=(cols, 1),
            )

        wide, narrow = torch.nn.Parameter(shard(256)), torch.nn.Parameter(shard(128))
        assert wide.shape == (1, 256) and wide.to_local().shape == (0, 256)
        opt = FusedAdamW([wide, narrow], lr=1e-3, moments="fp8")
        wide.grad, narrow.grad = shard(256), shard(128)
        opt.step()
        st = opt.state[wide]
        assert set(st) == {"step", "master_param", *FP8_KEYS}
        assert st["exp_avg"].shape == (0, 256) and st["exp_avg"].dtype == torch.uint8
        assert st["exp_avg_scale"].shape == (0, 1)
        assert st["exp_avg_sq_root_scale"].shape == (0, 1)
        assert set(opt.state[narrow]) == {"step", "master_param", "exp_avg", "exp_avg_sq"}
    finally:
        dist.destroy_process_group()
