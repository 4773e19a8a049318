"""CPU: stochastic rounding to bf16 and the master-free FusedAdamW — the
Philox reference, the rounding's definition, state conversions, the
checkpoint engine and a small convergence comparison."""

import os
import time

import pytest
import torch

from dlrover_amd.ops import FusedAdamW, philox4x32_10, stochastic_round_bf16


def test_philox_known_answer():
    # Random123's known-answer vectors for philox4x32, 10 rounds
    kat = [
        ((0, 0, 0, 0), (0, 0),
         (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
         (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
         (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for counter, key, want in kat:
        got = philox4x32_10(torch.tensor(counter, dtype=torch.int64), key)
        assert got.tolist() == list(want)
    # batched: leading dimensions are independent counters
    both = torch.tensor([kat[0][0], (1, 0, 0, 0)], dtype=torch.int64)
    out = philox4x32_10(both, (0, 0))
    assert out[0].tolist() == list(kat[0][2]) and out[1].tolist() != out[0].tolist()


def test_rounding_follows_the_definition():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(4099, generator=gen) * 10 ** (
        torch.rand(4099, generator=gen) * 80 - 40
    )
    big = torch.finfo(torch.float32).max
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), big, -big,
                            1e-45, -3e-40, 1.0, -1.5, 2.0**-133])
    x[: special.numel()] = special
    x[100] = float("nan")
    got = stochastic_round_bf16(x, seed=7, stream=3, step=11)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    # exactly representable values, +-0 and inf as round-to-nearest would
    exact = x.bfloat16().float() == x
    assert exact[:4].all() and exact[8:11].all()
    assert torch.equal(got[exact].view(torch.int16), x[exact].bfloat16().view(torch.int16))
    assert torch.isnan(got[100]) and int(torch.isnan(got).sum()) == 1
    # every other result is one of the two bf16 neighbours of its input
    # (truncation towards zero and one step away from it), and both occur
    fin = torch.isfinite(x)
    lo = (x.view(torch.int32) >> 16).to(torch.int16)
    step = got.view(torch.int16)[fin].int() - lo[fin].int()
    assert ((step == 0) | (step == 1)).all()
    assert (step[~exact[fin]] == 0).any() and (step[~exact[fin]] == 1).any()
    # the noise is a function of seed, stream and step
    for other in (dict(seed=8, stream=3, step=11), dict(seed=7, stream=4, step=11),
                  dict(seed=7, stream=3, step=12), dict(seed=7 + 2**32, stream=3, step=11)):
        assert not torch.equal(
            stochastic_round_bf16(x, **other).view(torch.int16), got.view(torch.int16)
        )


def test_unbiased_where_nearest_is_not():
    n = 2**20
    x = torch.full((n,), 1 + 2.0**-9)  # a quarter of the bf16 ulp 2**-7 above 1
    assert (x.bfloat16() == 1).all()  # round-to-nearest moves none of them
    got = stochastic_round_bf16(x, seed=1).float()
    assert ((got == 1) | (got == 1 + 2.0**-7)).all()
    frac = float((got != 1).float().mean())
    bound = 4 * (0.25 * 0.75 / n) ** 0.5
    print(f"fraction rounded up {frac:.6f}, 0.25 +- {bound:.2e}")
    assert abs(frac - 0.25) <= bound


# ---------------------------------------------------------------------------
# the optimizer: state, conversions, checkpoint engine
# ---------------------------------------------------------------------------


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(
        torch.nn.Linear(256, 8, bias=True), torch.nn.Linear(8, 4)
    ).bfloat16()


def _train(model, opt, steps, scale=1.0):
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(4, 256, generator=gen) * scale).bfloat16()
    for _ in range(steps):
        opt.zero_grad()
        model(x).float().pow(2).mean().backward()
        opt.step()


@pytest.mark.parametrize("moments", ["fp32", "fp8"])
def test_state_and_conversions(moments):
    model = _model()
    opt = FusedAdamW(model.parameters(), lr=1e-2, moments=moments,
                     master_weights=False, sr_seed=5)
    before = [p.detach().clone() for p in model.parameters()]
    _train(model, opt, 2)
    w = model[0].weight
    moment_keys = (
        {"exp_avg", "exp_avg_scale", "exp_avg_sq_root", "exp_avg_sq_root_scale"}
        if moments == "fp8" else {"exp_avg", "exp_avg_sq"}
    )
    assert set(opt.state[w]) == {"step"} | moment_keys
    assert set(opt.state[model[0].bias]) == {"step", "exp_avg", "exp_avg_sq"}
    per_elem = 2 if moments == "fp8" else 8
    rest = sum(p.numel() for p in model.parameters()) - w.numel()
    assert opt.state_nbytes() == w.numel() * per_elem + rest * 8 + (
        2 * 4 * (w.numel() // 256) if moments == "fp8" else 0
    )
    for p, b in zip(model.parameters(), before):
        assert p.dtype == torch.bfloat16 and not torch.equal(p.detach(), b)

    # master-free -> masters: the master is the fp32 of the weight
    twin = _model()
    with_master = FusedAdamW(twin.parameters(), lr=1e-2, moments=moments)
    for p, q in zip(model.parameters(), twin.parameters()):
        q.data.copy_(p.data)
    with_master.load_state_dict(opt.state_dict())
    for p, q in zip(model.parameters(), twin.parameters()):
        st = with_master.state[q]
        assert torch.equal(st["master_param"], p.detach().float())
        assert st["step"] == 2
        for k in moment_keys & set(opt.state[p]):
            assert torch.equal(st[k], opt.state[p][k])
    _train(twin, with_master, 1)

    # masters -> master-free: the weight becomes RNE(master), the master goes
    masters = [with_master.state[q]["master_param"].clone() for q in twin.parameters()]
    back_model = _model()
    back = FusedAdamW(back_model.parameters(), lr=1e-2, moments=moments,
                      master_weights=False)
    back.load_state_dict(with_master.state_dict())
    for q, m in zip(back_model.parameters(), masters):
        assert "master_param" not in back.state[q] and back.state[q]["step"] == 3
        assert torch.equal(q.detach(), m.bfloat16())
    _train(back_model, back, 1)

    # fp32 parameters are their own master either way
    p32 = torch.nn.Parameter(torch.randn(3, 5))
    o32 = FusedAdamW([p32], lr=1e-2, master_weights=False)
    p32.grad = torch.randn(3, 5)
    o32.step()
    assert torch.equal(o32.state[p32]["master_param"], p32.detach())


def test_capture_graph_is_refused():
    with pytest.raises(ValueError, match="capture_graph"):
        FusedAdamW(_model().parameters(), master_weights=False, capture_graph=True)


def test_checkpoint_engine_roundtrip(tmp_path, monkeypatch):
    from dlrover_amd.trainer.flash_checkpoint.engine import (
        ShardedCheckpointEngine,
    )

    # a shared-memory segment of this test's own
    monkeypatch.setenv("ELASTIC_JOB_NAME", f"sr{os.getpid()}_{time.time_ns()}")
    model = _model()
    opt = FusedAdamW(model.parameters(), lr=1e-2, moments="fp8",
                     master_weights=False)
    _train(model, opt, 2)
    saved = {
        p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
        for p, st in opt.state.items()
    }
    weights = [p.detach().clone() for p in model.parameters()]
    eng = ShardedCheckpointEngine(str(tmp_path / "ckpt"))
    try:
        sd = eng.gather_state_dict(model, opt)
        assert sd["_derived"] == {}
        assert set(sd["model"]) == {n for n, _ in model.named_parameters()}
        eng.save_to_memory(3, sd)
        _train(model, opt, 1, scale=2.0)  # something for the restore to undo
        assert not torch.equal(model[0].weight.detach(), weights[0])
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


def test_convergence_least_squares():
    """The 64x256 least-squares layer of tests/test_adamw_fp8_cpu.py with a
    bf16 weight, 90 steps from the same initialisation, three ways: fp32
    master weights, no master with stochastic rounding, and no master with
    round-to-nearest (the fp32 copy restarts from the bf16 weight every
    step). Measured final losses: 12.282263 (masters), 12.282677 (SR, x1.00003)
    and 12.312158 (round-to-nearest, 0.0295 above SR). One seed is one
    sample: SR may be up to twice the measured ratio above the master run,
    and round-to-nearest must be worse than SR by half the measured margin."""
    lr, steps = 1e-3, 90

    def run(kind):
        gen = torch.Generator().manual_seed(0)
        feat = 10 ** (-3.5 * torch.arange(256) / 255)
        x = torch.randn(32, 256, generator=gen) * feat
        w_true = torch.randn(64, 256, generator=gen)
        y = x @ w_true.t()
        w = torch.nn.Parameter(torch.zeros(64, 256, dtype=torch.bfloat16))
        opt = FusedAdamW([w], lr=lr, weight_decay=0.0, multi_tensor=True,
                         master_weights=kind != "sr")
        loss = None
        for _ in range(steps):
            opt.zero_grad()
            loss = (w.float() @ x.t() - y.t()).pow(2).mean()
            loss.backward()
            if kind == "rne" and "master_param" in opt.state[w]:
                # no master: the fp32 copy restarts from the bf16 weight
                opt.state[w]["master_param"].copy_(w.detach().float())
            opt.step()
        return float((w.detach().float() @ x.t() - y.t()).pow(2).mean())

    master, sr, rne = run("master"), run("sr"), run("rne")
    print(f"final loss: masters {master:.6f}, SR {sr:.6f}, RNE no master {rne:.6f}")
    assert sr <= 2 * 1.00003 * master
    assert rne - sr >= 0.5 * 0.0295
