"""Global grad-norm clipping under FSDP2 over a real 2-process gloo group.

Each rank holds a shard of every gradient, so the optimizer has to sum the
squared norm across the mesh's group before it clips. Checked against the
full gradients and against a single-process run of the same model, seed and
batch.
"""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dlrover_amd.common.global_context import find_free_port

WS = 2
MAX_NORM = 0.5


def _worker(rank, port, results):
    os.environ.update(
        {
            "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": str(port),
            "RANK": str(rank),
            "LOCAL_RANK": str(rank),
            "WORLD_SIZE": str(WS),
        }
    )
    dist.init_process_group("gloo", rank=rank, world_size=WS)
    try:
        from torch.distributed.fsdp import fully_shard

        from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
        from dlrover_amd.ops import FusedAdamW

        cfg = LlamaConfig.tiny()

        def make():
            torch.manual_seed(0)
            model = LlamaForCausalLM(cfg)
            ids = torch.randint(0, cfg.vocab_size, (2, 16))
            return model, ids

        # single-process run: same model, seed, batch and clipping
        ref_model, ids = make()
        ref_opt = FusedAdamW(
            ref_model.parameters(), lr=1e-3, weight_decay=0.0,
            max_grad_norm=MAX_NORM,
        )
        ref_model(ids, ids.clone()).backward()
        ref_opt.step()

        model, ids = make()
        for blk in model.blocks:
            fully_shard(blk)
        fully_shard(model)
        opt = FusedAdamW(
            model.parameters(), lr=1e-3, weight_decay=0.0,
            max_grad_norm=MAX_NORM,
        )
        model(ids, ids.clone()).backward()
        full_sq = torch.zeros((), dtype=torch.float64)
        for p in model.parameters():
            full_sq += p.grad.full_tensor().double().pow(2).sum()
        want = full_sq.sqrt().float()
        opt.step()

        norm = opt.last_grad_norm
        torch.testing.assert_close(norm, want, rtol=1e-5, atol=0)
        torch.testing.assert_close(norm, ref_opt.last_grad_norm, rtol=1e-5, atol=0)
        assert float(norm) > MAX_NORM, "the step must actually clip"
        for (name, p), q in zip(model.named_parameters(), ref_model.parameters()):
            torch.testing.assert_close(
                p.full_tensor(), q.detach(), rtol=1e-4, atol=1e-5,
                msg=lambda m, name=name: f"{name}: {m}",
            )
        results[rank] = ("ok", float(norm))
    except Exception as e:  # noqa: BLE001
        import traceback

        results[rank] = (f"FAIL rank{rank}: {e}\n{traceback.format_exc()}", None)
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_fsdp2_global_norm_clip_two_ranks():
    port = find_free_port()
    ctx = mp.get_context("spawn")
    with mp.Manager() as mgr:
        results = mgr.dict()
        procs = [
            ctx.Process(target=_worker, args=(r, port, results)) for r in range(WS)
        ]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=240)
        for p in procs:
            if p.is_alive():
                p.kill()
        outcomes = dict(results)
    assert all(outcomes.get(r, ("missing",))[0] == "ok" for r in range(WS)), outcomes
    # both ranks hold the same global norm, bit for bit
    assert outcomes[0][1] == outcomes[1][1], outcomes
