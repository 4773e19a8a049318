#!/usr/bin/env python3
"""Llama-3 FSDP bf16 training under dlrover-run with flash checkpoint —
BASELINE config #2 ("Llama-3 8B FSDP bf16 on 8xMI355X, flash-checkpoint every
50 steps + 1 injected SIGKILL").

Run on one 8-GPU MI355X node:
    dlrover-run --standalone --nproc-per-node 8 examples/train_llama_fsdp.py \
        --model llama3_8b --steps 200 --ckpt-interval 50

Fault injection: DLROVER_TEST_KILL_AT_STEP=<n> SIGKILLs rank 0 at step n on
the first incarnation; the agent persists the last shm snapshot, restarts
workers, and training resumes from the latest committed checkpoint.
"""

import argparse
import dataclasses
import json
import os
import signal
import time

import torch
import torch.distributed as dist


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3_8b",
                   choices=["llama3_8b", "small_1b", "tiny"])
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--seq", type=int, default=4096)
    p.add_argument("--ckpt-interval", type=int, default=50)
    p.add_argument("--ckpt-dir", default="/tmp/dlrover_amd_ckpt/llama")
    p.add_argument("--ckpt-verify", action="store_true",
                   help="checksum every checkpoint tensor inside the fused "
                        "device snapshot and verify it on restore")
    p.add_argument("--progress-file", default="")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--grad-clip", type=float, default=0.0,
                   help="clip the global gradient norm at this value inside "
                        "the fused optimizer (0 = off)")
    p.add_argument("--optim-moments", choices=("fp32", "fp8"), default="fp32",
                   help="fp8: keep the Adam moments of every weight whose "
                        "last dim is a multiple of 256 as e4m3 codes with "
                        "per-256-element scales (half the checkpointed state)")
    p.add_argument("--linear", choices=("bf16", "fp8"), default="bf16",
                   help="fp8: the qkv, o, gate_up and down projections run "
                        "their GEMMs on FP8 operands (e4m3 activations and "
                        "weights, e5m2 gradients, one current scale per "
                        "tensor); parameters and checkpoints stay bf16")
    p.add_argument("--act-ckpt", action="store_true",
                   help="recompute transformer blocks in backward")
    p.add_argument("--doc-len", type=int, default=0,
                   help="pack every synthetic sequence from documents of this "
                        "many tokens: attention and RoPE positions stay "
                        "inside a document, the label of each document's "
                        "last token is ignored (0 = one document)")
    args = p.parse_args()

    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM
    from dlrover_amd.ops import FusedAdamW
    from dlrover_amd.trainer.elastic import ElasticTrainer
    from dlrover_amd.trainer.flash_checkpoint import (
        FsdpShardCheckpointer,
        StorageType,
    )

    use_gpu = torch.cuda.is_available()
    local_rank = int(os.getenv("LOCAL_RANK", "0"))
    if use_gpu:
        torch.cuda.set_device(local_rank)
        from dlrover_amd.ops.api import hip_ops

        hip_ops()  # fail loudly without the native extension
    dist.init_process_group("nccl" if use_gpu else "gloo")
    rank = dist.get_rank()
    device = torch.device(f"cuda:{local_rank}" if use_gpu else "cpu")

    torch.manual_seed(0)
    cfg = (
        LlamaConfig.llama3_8b(max_seq_len=max(args.seq, 4096))
        if args.model == "llama3_8b"
        else getattr(LlamaConfig, args.model)()
    )
    if args.model == "tiny":
        args.seq = min(args.seq, cfg.max_seq_len)
    cfg = dataclasses.replace(cfg, activation_checkpointing=args.act_ckpt,
                              linear_precision=args.linear)
    with device:
        model = LlamaForCausalLM(cfg)
    model = model.to(device)
    use_fsdp = use_gpu or os.getenv("DLROVER_FSDP_CPU", "") == "1"
    if use_gpu:
        model = model.bfloat16()
    if use_fsdp:
        # fully_shard even at world 1: DTensor shard0 tags keep checkpoints
        # UCP-reshardable in BOTH scale directions (grow needs the ws-1 ckpt
        # tagged shard0, not replicated)
        from torch.distributed.fsdp import fully_shard

        for blk in model.blocks:
            fully_shard(blk)
        fully_shard(model)
    clip_kw = {"max_grad_norm": args.grad_clip} if args.grad_clip > 0 else {}
    opt = FusedAdamW(model.parameters(), lr=args.lr, weight_decay=0.1,
                     moments=args.optim_moments, **clip_kw)
    trainer = ElasticTrainer(model)

    cp = FsdpShardCheckpointer(
        args.ckpt_dir, model, opt, checksum=True if args.ckpt_verify else None
    )
    start_step = 0
    restored = cp.load_checkpoint()
    if restored is not None:
        start_step = int(restored.get("step", 0))
        if rank == 0:
            print(f"[train] resumed from step {start_step}", flush=True)

    kill_at = int(os.getenv("DLROVER_TEST_KILL_AT_STEP", "0"))
    incarnation = int(os.getenv("TORCHELASTIC_RESTART_COUNT", "0"))

    torch.manual_seed(1 + rank)
    ids = torch.randint(0, cfg.vocab_size, (args.batch, args.seq), device=device)
    labels = torch.randint(0, cfg.vocab_size, (args.batch, args.seq), device=device)

    doc_start = None
    if args.doc_len > 0:
        from dlrover_amd.ops import doc_start_from_ids

        idx = torch.arange(args.seq, device=device)
        doc_start = doc_start_from_ids(
            (idx // args.doc_len).expand(args.batch, args.seq))
        # a document's last token has no next token of its own to predict
        last = (idx % args.doc_len == args.doc_len - 1) | (idx == args.seq - 1)
        labels[:, last] = -100

    for step in range(start_step + 1, args.steps + 1):
        t0 = time.perf_counter()
        with trainer.step():
            loss = model(ids, labels, doc_start=doc_start)
            loss.backward()
        opt.step()
        opt.zero_grad()
        extra = {}
        if args.grad_clip > 0 and args.progress_file and rank == 0:
            # reading the device-side norm is this script's sync, next to
            # the loss.item() the record already pays for
            extra["grad_norm"] = round(float(opt.last_grad_norm), 4)
        if step % args.ckpt_interval == 0:
            blocking = cp.save_checkpoint(step, storage_type=StorageType.DISK)
            if rank == 0:
                print(f"[train] ckpt@{step} blocked {blocking * 1e3:.1f} ms",
                      flush=True)
        if args.progress_file and rank == 0:
            with open(args.progress_file, "a") as f:
                f.write(json.dumps({
                    "step": step, "loss": round(float(loss.item()), 4),
                    "step_s": round(time.perf_counter() - t0, 3),
                    "ts": round(time.time(), 3),
                    "incarnation": incarnation, "resumed_from": start_step,
                    "world": dist.get_world_size(),
                    "device": str(device),
                    **extra,
                }) + "\n")
        if kill_at and step == kill_at and incarnation == 0 and rank == 0:
            print(f"[train] injecting SIGKILL at step {step}", flush=True)
            os.kill(os.getpid(), signal.SIGKILL)

    cp.wait_latest_checkpoint()
    if rank == 0:
        peak = (f" peak_allocated={torch.cuda.max_memory_allocated() / 2**30:.2f}GiB"
                if use_gpu else "")
        print(f"[train] done at step {args.steps} loss={loss.item():.4f}{peak}",
              flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
