"""GPU numerics of the vocab-parallel cross-entropy kernels
(ops/csrc/vocab_parallel_ce.hip), all tensor-parallel shards simulated in one
process: ce_shard_stats per shard -> stack -> ce_shard_finish per shard.

Reference: torch fp32 F.cross_entropy on the concatenation of the bf16 shard
values, snapshotted before the op consumes them. Tolerances are those of the
full-vocab kernel's test (test_ops_gpu.py): loss rtol 1e-2 / atol 1e-3, grad
rtol 5e-2 / atol 1e-4 — gradients are stored in bf16 (2^-9 relative), sums
are fp32. max and gather are exact operations and are compared bitwise.

Shapes (block = 512 threads x 8 columns = 4096 columns per sweep, grid capped
at 2048 rows): Vs 8 / 520 / 4104 = less than one sweep / a partial sweep /
more than one sweep; N = 2051 strides rows past the grid cap; Vs = 16032 is
the Llama-3 shard width at tp = 8.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = -100
LOSS_TOL = dict(rtol=1e-2, atol=1e-3)
GRAD_TOL = dict(rtol=5e-2, atol=1e-4)

CASES = [(5, vs, tp) for vs in (8, 520, 4104) for tp in (1, 2, 8)] + [
    (11, 520, 8),  # enough rows to put a target in each of 8 shards
    (2051, 264, 2),
    (8, 16032, 2),
]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from dlrover_amd.ops.api import hip_ops

    hip_ops()  # raises on a GPU box if the extension didn't build


def _dev():
    return torch.device("cuda:0")


def _targets(n, vs, tp, gen):
    """Global ids. Row i targets shard i % tp: row 0 its column 0, row 1 its
    column Vs-1, the rest a random column; row 2 is ignored."""
    col = torch.randint(0, vs, (n,), generator=gen)
    col[0] = 0
    col[1] = vs - 1
    t = (torch.arange(n) % tp) * vs + col
    t[2] = IGN
    return t.int()


def _reference(full_bf16, targets):
    """fp32 reference on the bf16 values: per-row losses, mean loss, dlogits
    of the mean."""
    x = full_bf16.float().requires_grad_(True)
    rows = F.cross_entropy(x, targets.long(), ignore_index=IGN, reduction="none")
    n_valid = max(int((targets != IGN).sum()), 1)
    mean = rows.sum() / n_valid
    mean.backward()
    return rows.detach(), mean.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _case(n, vs, tp):
    """Inputs and reference of one shape, built once and never written to:
    the kernels only ever see clones of the shards."""
    gen = torch.Generator().manual_seed(1000 * n + vs + tp)
    full = (torch.randn(n, tp * vs, generator=gen) * 2.0).bfloat16().to(_dev())
    targets = _targets(n, vs, tp, gen).to(_dev())
    return full, targets, _reference(full, targets)


def _run_shards(full, targets, vs, tp):
    """The whole sequence on fresh clones of the shards. Returns stats_all
    [tp,N,3], the per-shard losses list and the concatenated dlogits."""
    from dlrover_amd.ops import ce_shard_finish, ce_shard_stats

    n = full.shape[0]
    # clone, not .contiguous(): at tp == 1 the view already is contiguous
    shards = [
        full.view(n, tp, vs)[:, r].clone(memory_format=torch.contiguous_format)
        for r in range(tp)
    ]
    stats_all = torch.stack(
        [ce_shard_stats(shards[r], targets, r * vs, IGN) for r in range(tp)]
    )
    n_valid = max(int((targets != IGN).sum()), 1)
    losses = [
        ce_shard_finish(shards[r], targets, r * vs, stats_all, 1.0 / n_valid, IGN)
        for r in range(tp)
    ]
    return stats_all, losses, torch.cat(shards, dim=1)


@pytest.mark.parametrize("n,vs,tp", CASES)
def test_shard_simulation_matches_fp32_reference(n, vs, tp):
    full, targets, (ref_rows, ref_mean, ref_grad) = _case(n, vs, tp)
    valid = targets != IGN
    tl = targets.long()

    # ---- placement the case is meant to have ----
    assert int((~valid).sum()) == 1 and not bool(valid[2])
    assert int(tl[0]) % vs == 0 and int(tl[1]) % vs == vs - 1
    if n >= tp + 3:
        assert set((tl[valid] // vs).tolist()) == set(range(tp))

    stats_all, losses, grad = _run_shards(full, targets, vs, tp)
    assert stats_all.shape == (tp, n, 3)
    assert torch.isfinite(stats_all).all()

    # ---- stage 1: exact max, exact gather, lse within the loss tolerance ----
    for r in range(tp):
        shard = full.view(n, tp, vs)[:, r].float()
        assert torch.equal(stats_all[r, :, 0], shard.amax(-1))
        local = tl - r * vs
        owns = valid & (local >= 0) & (local < vs)
        picked = shard.gather(1, local.clamp(0, vs - 1)[:, None]).squeeze(1)
        expect_t = torch.where(owns, picked, torch.zeros_like(picked))
        assert torch.equal(stats_all[r, :, 2], expect_t)
        lse = stats_all[r, :, 0] + torch.log(stats_all[r, :, 1])
        torch.testing.assert_close(lse, torch.logsumexp(shard, -1), **LOSS_TOL)

    # ---- stage 2 ----
    for r in range(1, tp):
        assert torch.equal(losses[r], losses[0])
    print(f"[{n}x{vs} tp{tp}] max |loss - ref| = "
          f"{float((losses[0] - ref_rows).abs().max()):.3e}, max |grad - ref| = "
          f"{float((grad.float() - ref_grad).abs().max()):.3e}")
    torch.testing.assert_close(losses[0], ref_rows, **LOSS_TOL)
    n_valid = int(valid.sum())
    torch.testing.assert_close(losses[0].sum() / n_valid, ref_mean, **LOSS_TOL)
    torch.testing.assert_close(grad.float(), ref_grad, **GRAD_TOL)
    # the ignored row: exactly zero loss and exactly zero gradient everywhere
    assert float(losses[0][2]) == 0.0
    assert int(torch.count_nonzero(grad[2])) == 0


@pytest.mark.parametrize("n,vs,tp", [(5, 4104, 8), (2051, 264, 2)])
def test_bitwise_reproducible(n, vs, tp):
    full, targets, _ = _case(n, vs, tp)
    a = _run_shards(full, targets, vs, tp)
    b = _run_shards(full, targets, vs, tp)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1][0], b[1][0])
    assert torch.equal(a[2], b[2])


@pytest.mark.parametrize("tp", [2, 8])
def test_dominant_shard_and_target_outside_max_shard(tp):
    """Row 0: shard 1 sits near +60, every other shard near -60, so
    exp(m_r - M) underflows to 0 for all shards but one — and the target lives
    in shard 0, so its (tiny) probability comes from a non-dominant shard.
    Row 1: ordinary values with the row maximum planted in shard 0 and the
    target in the last shard."""
    n, vs = 5, 520
    gen = torch.Generator().manual_seed(77 + tp)
    x = torch.randn(n, tp, vs, generator=gen)
    x[0] -= 60.0
    x[0, 1] += 120.0
    x[1, 0, 17] = 9.0
    full = x.view(n, tp * vs).bfloat16().to(_dev())
    targets = _targets(n, vs, tp, gen)
    targets[0] = 5  # shard 0
    targets[1] = (tp - 1) * vs + 3  # last shard
    targets = targets.to(_dev())
    ref_rows, ref_mean, ref_grad = _reference(full, targets)

    stats_all, losses, grad = _run_shards(full, targets, vs, tp)
    m = stats_all[:, :, 0]
    # the constructed properties really hold
    assert int(m[:, 0].argmax()) == 1
    others = [r for r in range(tp) if r != 1]
    assert (torch.exp(m[others, 0] - m[1, 0]) == 0).all()
    assert int(m[:, 1].argmax()) == 0 and int(targets[1]) // vs == tp - 1

    for r in range(1, tp):
        assert torch.equal(losses[r], losses[0])
    assert torch.isfinite(losses[0]).all() and torch.isfinite(grad.float()).all()
    torch.testing.assert_close(losses[0], ref_rows, **LOSS_TOL)
    torch.testing.assert_close(grad.float(), ref_grad, **GRAD_TOL)
    assert float(losses[0][0]) > 100.0  # lse ~ +60, target logit ~ -60


def test_all_rows_ignored():
    n, vs, tp = 5, 520, 2
    full, _, _ = _case(n, vs, tp)
    targets = torch.full((n,), IGN, dtype=torch.int32, device=_dev())
    stats_all, losses, grad = _run_shards(full, targets, vs, tp)
    assert torch.isfinite(stats_all).all()
    assert (stats_all[:, :, 2] == 0).all()
    for l in losses:
        assert int(torch.count_nonzero(l)) == 0
    assert int(torch.count_nonzero(grad)) == 0
    assert float(losses[0].sum()) == 0.0
    # and through the autograd op (n_valid == 0 -> scale 1/max(0, 1))
    from dlrover_amd.ops import vocab_parallel_cross_entropy

    logits = full.clone().requires_grad_(True)
    loss = vocab_parallel_cross_entropy(logits, targets, 0)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert int(torch.count_nonzero(logits.grad)) == 0


def test_autograd_single_shard_agrees_with_full_vocab_op():
    from dlrover_amd.ops import cross_entropy_loss, vocab_parallel_cross_entropy

    n, vs = 5, 4104
    full, targets, (_, ref_mean, ref_grad) = _case(n, vs, 1)
    a = full.clone().requires_grad_(True)
    b = full.clone().requires_grad_(True)
    loss_vp = vocab_parallel_cross_entropy(a, targets, 0, tp_group=None)
    loss_vp.backward()
    loss_full = cross_entropy_loss(b, targets)
    loss_full.backward()
    assert a.grad is not None and a.grad.shape == full.shape
    torch.testing.assert_close(loss_vp.float(), loss_full.float(), **LOSS_TOL)
    torch.testing.assert_close(a.grad.float(), b.grad.float(), **GRAD_TOL)
    torch.testing.assert_close(loss_vp.float(), ref_mean, **LOSS_TOL)
    torch.testing.assert_close(a.grad.float(), ref_grad, **GRAD_TOL)


def test_bindings_reject_bad_shapes():
    """Host-side checks: nothing is launched."""
    from dlrover_amd.ops import ce_shard_finish, ce_shard_stats

    n = 4
    targets = torch.zeros(n, dtype=torch.int32, device=_dev())
    odd = torch.zeros(n, 12, dtype=torch.bfloat16, device=_dev())
    with pytest.raises(RuntimeError):
        ce_shard_stats(odd, targets, 0)
    with pytest.raises(RuntimeError):
        ce_shard_finish(
            odd, targets, 0, torch.zeros(1, n, 3, device=_dev()), 1.0
        )
    ok = torch.zeros(n, 16, dtype=torch.bfloat16, device=_dev())
    with pytest.raises(RuntimeError):
        ce_shard_finish(
            ok, targets, 0, torch.zeros(2, n - 1, 3, device=_dev()), 1.0
        )
    with pytest.raises(RuntimeError):
        ce_shard_stats(ok, targets[:-1], 0)
