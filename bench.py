#!/usr/bin/env python3
"""Flagship benchmark: Llama-3-8B FSDP bf16 training with flash checkpoint on
1..8 MI355X — the BASELINE.json headline metric.

What is measured (all real, nothing modeled):
  - W untimed warmup steps, then EXACTLY K timed steps bracketed by
    barrier + torch.cuda.synchronize() on both sides, MAX over ranks;
  - inside the timed window: a flash-checkpoint save-to-memory every
    --ckpt-interval steps (device-staged snapshot + async D2H into pinned
    host shm), and ONE restore-from-memory at the midpoint (the recovery a
    SIGKILL would trigger — model+optimizer reloaded from the shm snapshot);
  - goodput % = (sum of pure train-step seconds, min over ranks) /
    (timed wall seconds, max over ranks) — the same accounting the reference
    quotes 95% goodput with (README.md:61, flash_checkpoint.md:38).
    Per-step timing waits the COMPUTE stream only, so the async ckpt drain
    on its side stream is never booked as useful time; saves are skipped
    when the window has no remaining steps to hide their drain under.

value = goodput %; config carries ckpt_save_blocking_s / ckpt_restore_s /
tokens_per_s so the save/restore seconds of the metric name are reported on
the same line. vs_baseline divides by the reference's 95% goodput headline.

A plain run does only the above. --dump-outputs DIR additionally writes the
last timed step's loss and a seeded sample of the updated parameters as .npy
(seeds are fixed, so the inputs repeat from run to run; the midpoint restore
reloads the latest in-window snapshot, reported as config.ckpt_restored_step).
--full is where measurements that do not feed the headline figure belong;
there are none yet, so it changes nothing today.
"""

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

_T0 = time.perf_counter()


def hb(msg: str):
    """Per-phase heartbeat on stderr (stdout stays the one JSON line).
    A crash mid-run then localizes itself in the driver's stderr tail."""
    if os.getenv("DLROVER_BENCH_QUIET", "") == "1":
        return
    r = os.environ.get("RANK", "0")
    print(f"[bench hb r{r} +{time.perf_counter() - _T0:.1f}s] {msg}",
          file=sys.stderr, flush=True)


def self_launch(args):
    """`bench.py --gpus N` run bare (no RANK in env) must really measure N
    ranks: exec torchrun with ourselves as the target (the driver may launch
    either way). Ref behavior: launcher owns process spawn
    (elastic_run.py:246-643)."""
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={args.gpus}",
        "--master-addr=127.0.0.1", "--master-port=29573",
        sys.argv[0],
    ] + sys.argv[1:]
    hb(f"self-launching {args.gpus} ranks via torch.distributed.run")
    os.execv(sys.executable, cmd)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=110, help="timed steps (K)")
    p.add_argument("--warmup", type=int, default=3, help="untimed steps (W)")
    p.add_argument("--model", default="llama3_8b", choices=["llama3_8b", "qwen2_7b", "small_1b", "tiny"])
    p.add_argument("--batch", type=int, default=2, help="per-GPU micro batch")
    p.add_argument("--seq", type=int, default=4096)
    # BASELINE.json config #2 names "flash-checkpoint every 50 steps";
    # K=110 covers two in-window saves plus the injected failure restore
    # (measured 96.9% goodput; one injected failure per ~70 s is still far
    # denser than any real MTBF)
    p.add_argument("--ckpt-interval", type=int, default=50)
    p.add_argument("--no-ckpt", action="store_true")
    p.add_argument("--act-ckpt", action="store_true",
                   help="recompute blocks in backward (activation ckpt)")
    p.add_argument("--ckpt-scope", default="full", choices=["full", "model"])
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--dump-outputs", metavar="DIR", default="",
                   help="after the timed steps, write what the last timed "
                        "step computed (loss + a fixed sample of the updated "
                        "parameters) as DIR/<name>.npy, float32")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements that do not "
                        "feed the headline figure (none at present: every "
                        "field of the result line comes out of the one "
                        "timed window, so --full adds nothing yet)")
    return p.parse_args()


# per-tensor cap of the --dump-outputs parameter sample: ~300 tensors x 16384
# fp32 values stays near 20 MB for the 8B flagship (limit: 64 MB per dump)
_DUMP_PER_TENSOR = 16384


def dump_outputs(out_dir, rank, world, loss, model):
    """What a caller of the timed path holds after its last step: the loss
    that step returned and the parameters its optimizer update left behind.
    Tensors larger than _DUMP_PER_TENSOR are sampled at seeded indices (same
    indices every run, in named_parameters order), so two builds run with the
    same arguments can be compared value for value. FSDP ranks dump their
    local shards, one file set per rank."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if world == 1 else f"_rank{rank}"
    gen = torch.Generator().manual_seed(4321)
    chunks = []
    with torch.no_grad():
        for _, p in model.named_parameters():
            t = p.detach()
            if hasattr(t, "to_local"):
                t = t.to_local()
            flat = t.reshape(-1)
            if flat.numel() > _DUMP_PER_TENSOR:
                idx = torch.randint(0, flat.numel(), (_DUMP_PER_TENSOR,),
                                    generator=gen)
                flat = flat[idx.to(flat.device)]
            chunks.append(flat.float().cpu())
    np.save(os.path.join(out_dir, f"loss{suffix}.npy"),
            loss.detach().float().cpu().numpy().reshape(1))
    np.save(os.path.join(out_dir, f"params_sample{suffix}.npy"),
            torch.cat(chunks).numpy())


def setup_dist(args):
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        rank = int(os.environ["RANK"])
        world = int(os.environ["WORLD_SIZE"])
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
    else:
        if args.gpus > 1:
            self_launch(args)  # execs torchrun; does not return
        rank, world, local_rank = 0, 1, 0
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("LOCAL_RANK", "0")
    if args.gpus > 1 and world != args.gpus:
        raise RuntimeError(
            f"--gpus {args.gpus} but WORLD_SIZE={world}: refusing to "
            "silently measure a different world size"
        )
    on_gpu = torch.cuda.is_available()
    backend = "nccl" if on_gpu else "gloo"  # nccl == RCCL on ROCm
    if on_gpu:
        # modulo: lets N ranks share one device for multi-rank RCCL
        # validation on a 1-GPU box (the 8-GPU node maps 1:1)
        dev = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(dev)
        dist.init_process_group(
            backend=backend, rank=rank, world_size=world,
            device_id=torch.device(f"cuda:{dev}"),
        )
        local_rank = dev
    else:
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    hb(f"dist ready: rank={rank} world={world} backend={backend}")
    return rank, world, local_rank, on_gpu


def build_model(args, device):
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    cfg = getattr(LlamaConfig, args.model)() if args.model != "llama3_8b" else (
        LlamaConfig.llama3_8b(max_seq_len=max(args.seq, 4096))
    )
    if args.model == "tiny":
        args.seq = min(args.seq, cfg.max_seq_len)
    if getattr(args, "act_ckpt", False):
        cfg.activation_checkpointing = True
    with device:
        model = LlamaForCausalLM(cfg)
    model = model.to(device)
    if device.type == "cuda":
        model = model.bfloat16()
    return model, cfg


def apply_fsdp(model, world):
    """FSDP2 (fully_shard + DTensor) over RCCL; per-block wrapping so the
    all-gather of block i+1 overlaps compute of block i."""
    from torch.distributed.fsdp import fully_shard

    for blk in model.blocks:
        fully_shard(blk)
    fully_shard(model)
    return model


def main():
    args = parse_args()
    rank, world, local_rank, on_gpu = setup_dist(args)
    from dlrover_amd.utils.numa import maybe_bind_from_env

    maybe_bind_from_env()
    device = torch.device(f"cuda:{local_rank}" if on_gpu else "cpu")
    # model init must be IDENTICAL across ranks (FSDP shards the local
    # weights as-is); per-rank seeds are set after build for the data
    torch.manual_seed(1234)

    from dlrover_amd.ops import FusedAdamW
    from dlrover_amd.trainer.flash_checkpoint import FsdpShardCheckpointer, StorageType

    if on_gpu:
        from dlrover_amd.ops.api import hip_ops

        hip_ops()  # never bench a silent eager fallback

    hb(f"building {args.model} on {device}")
    model, cfg = build_model(args, device)
    n_params = sum(p.numel() for p in model.parameters())
    hb(f"model built: {n_params / 1e9:.2f}B params")
    # FSDP degenerates to 1 shard at world_size 1 but still runs its
    # all-gather copy-in/out machinery (~7% of step, measured: profiles/r01d
    # __amd_rocclr_copyBuffer + chunk_cat) — shard only when there is
    # something to shard. DTensor fully_shard also needs a GPU device mesh.
    use_fsdp = on_gpu and world > 1
    if use_fsdp:
        model = apply_fsdp(model, world)
    elif world > 1:
        # CPU plumbing lane: plain DDP over gloo so grads still sync
        from torch.nn.parallel import DistributedDataParallel as DDP

        model = DDP(model)
    opt = FusedAdamW(model.parameters(), lr=args.lr, weight_decay=0.1)
    torch.manual_seed(1234 + rank)  # per-rank DATA streams

    ckpt_dir = os.path.join(os.getcwd(), "gpurun_out", "bench_ckpt")
    cp = None
    if not args.no_ckpt:
        cp = FsdpShardCheckpointer(ckpt_dir, model, opt)
        if args.ckpt_interval >= args.steps:
            # a window shorter than the named 50-step cadence still has to
            # contain saves for the metric to mean anything — scale down
            args.ckpt_interval = max(2, args.steps // 3)

    def fresh_batch():
        # new synthetic tokens every step: a fixed batch lets an 8B model
        # memorize to ~0 loss within the bench window, which distorts timing
        ids = torch.randint(0, cfg.vocab_size, (args.batch, args.seq), device=device)
        labels = torch.randint(0, cfg.vocab_size, (args.batch, args.seq), device=device)
        return ids, labels

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    def sync_compute():
        # per-step timing must wait the COMPUTE stream only: a device-wide
        # synchronize would also wait the checkpoint drain running on its
        # side stream, booking checkpoint time as useful training time
        if on_gpu:
            torch.cuda.current_stream().synchronize()

    def train_step():
        ids, labels = fresh_batch()
        loss = model(ids, labels)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    def ckpt_state():
        sd = cp.engine.gather_state_dict(model, None if args.ckpt_scope == "model" else opt)
        return sd

    # ---- warmup (also seeds optimizer state so checkpoints are full-size)
    for w in range(args.warmup):
        hb(f"warmup step {w + 1}/{args.warmup}")
        train_step()
    hb("warmup done; sizing ckpt segment")
    if cp is not None:
        # size the shm segment + staging outside the timed window (the
        # reference also excludes first-export spin-up, ~20 s: BASELINE.md)
        # step must be > 0: the shm commit word treats 0 as "empty"
        sd = ckpt_state()
        sd["step"] = 1
        cp.engine.save_to_memory(1, sd)
        cp.engine.wait_saving()
        # second save now that the segment exists+is pinned: measures the
        # STEADY-STATE drain (the first one includes one-time shm creation
        # and 100-GB-class page pinning), used to decide whether a later
        # in-window save's async drain still has steps to hide under
        t0 = time.perf_counter()
        cp.engine.save_to_memory(1, ckpt_state() | {"step": 1})
        cp.engine.wait_saving()
        drain_estimate = time.perf_counter() - t0
        hb(f"ckpt segment sized; steady-state drain {drain_estimate:.2f} s")
    else:
        drain_estimate = 0.0
    sync()
    dist.barrier()
    sync()

    # ---- timed window: EXACTLY K steps + periodic flash saves + 1 restore
    useful = 0.0
    save_blockings = []
    restore_s = None
    restored_step = None
    restore_at = args.steps // 2
    hb(f"timed window begin: K={args.steps}")
    step_est = None  # running mean of pure step seconds
    t_begin = time.perf_counter()
    for k in range(args.steps):
        t0 = time.perf_counter()
        loss = train_step()
        sync_compute()
        dt = time.perf_counter() - t0
        useful += dt
        step_est = dt if step_est is None else 0.7 * step_est + 0.3 * dt
        hb(f"step {k + 1}/{args.steps}")
        save_due = (cp is not None and (k + 1) % args.ckpt_interval == 0
                    and k + 1 < args.steps)
        if save_due:
            # drain-cover margin must be RANK-UNIFORM: save_to_memory runs
            # readiness/step collectives, so per-rank timing noise deciding
            # differently would deadlock the world (min over ranks = every
            # rank can cover its drain)
            margin = (args.steps - (k + 1)) * (step_est or 0.0) - drain_estimate
            if world > 1:
                t = torch.tensor([margin], dtype=torch.float64,
                                 device=device if on_gpu else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                margin = t.item()
            save_due = margin > 0
        if save_due:
            # saves only when the async drain has future steps to hide
            # under — steady-state training always does; only a driver
            # window shorter than one drain doesn't (the drain would sit
            # exposed in the timed window as pure checkpoint stall)
            sd = ckpt_state()
            sd["step"] = k + 1
            blocking = cp.engine.save_to_memory(k + 1, sd, block=False)
            save_blockings.append(blocking)
            hb(f"flash save @ step {k + 1}: blocking {blocking * 1e3:.1f} ms")
        if cp is not None and k + 1 == restore_at:
            # simulated failure recovery: reload model+optimizer from shm
            cp.engine.shm_handler.wait_drained()
            t0 = time.perf_counter()
            sd = cp.engine.restore_into(
                model, None if args.ckpt_scope == "model" else opt
            )
            assert sd is not None, "no checkpoint in shm to restore from"
            sync()
            restore_s = time.perf_counter() - t0
            restored_step = sd.get("step")
            hb(f"restore @ step {k + 1}: {restore_s:.2f} s "
               f"(snapshot of step {restored_step})")
    if cp is not None:
        cp.engine.shm_handler.wait_drained()
    sync()
    dist.barrier()
    sync()
    t_total = time.perf_counter() - t_begin
    hb(f"timed window done: {t_total:.2f} s")

    # ---- aggregate across ranks: total = max, useful = min (conservative).
    # tensor must live on the backend's device: the N>1 GPU group is
    # NCCL-only, which cannot reduce a CPU tensor
    stats = torch.tensor([t_total, useful], dtype=torch.float64,
                         device=device if on_gpu else "cpu")
    if world > 1:
        dist.all_reduce(stats[:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(stats[1:], op=dist.ReduceOp.MIN)
    t_total, useful = stats[0].item(), stats[1].item()

    goodput = 100.0 * useful / t_total
    tokens = world * args.steps * args.batch * args.seq
    loss_val = float(loss.item())

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world, loss, model)
        hb(f"outputs dumped to {args.dump_outputs}")

    if cp is not None:
        cp.close()

    if rank == 0:
        result = {
            "metric": (
                "checkpoint save+restore sec and goodput % under injected "
                "failure, Llama-3-8B FSDP 1/2/4/8 MI355X"
            ),
            "value": round(goodput, 3),
            "unit": "goodput_percent",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_total * 1000.0 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(goodput / 95.0, 4),
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "params": n_params,
                "global_batch": world * args.batch,
                "seq_len": args.seq,
                # fsdp1 = the world-size-1 degenerate (single shard, FSDP
                # wrapper elided — identical math, no dummy collectives)
                "parallelism": f"fsdp{world}" if (use_fsdp or (on_gpu and world == 1)) else f"dp{world}",
                "ckpt_interval": args.ckpt_interval,
                "ckpt_scope": args.ckpt_scope if cp is not None else "none",
                "ckpt_save_blocking_s": (
                    round(sum(save_blockings) / len(save_blockings), 4)
                    if save_blockings
                    else None
                ),
                "ckpt_restore_s": round(restore_s, 4) if restore_s else None,
                # which snapshot the midpoint restore reloaded: the dumped
                # outputs of two runs are comparable only when this matches
                "ckpt_restored_step": restored_step,
                "tokens_per_s": round(tokens / t_total, 1),
                "final_loss": round(loss_val, 4),
            },
        }
        print(json.dumps(result))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
