"""Microbenchmark: vocab-parallel cross-entropy (one tp=2 shard) against the
full-vocab fused kernel, on the same commit and in one process.

GPU only — there is no CPU fallback; without a device this script fails.

  shard  ce_shard_stats + ce_shard_finish on bf16 logits [N, Vs]
         (default N=4096, Vs=64128: one rank's half of the Llama-3 vocab)
  full   cross_entropy_fwd_bwd on bf16 logits [N, V] (V = 2 * Vs = 128256)

Both consume their logits, so every timed call starts from a pristine copy
restored outside the timed window. Each call is timed with its own pair of
device events; the variants alternate inside every repetition and the median
over all calls is reported with the min and max.

GB/s is algorithmic traffic over the median time: the bytes each algorithm
asks for (shard: two reads + one write of N*Vs bf16; full: three reads + one
write of N*V bf16), not a hardware counter — re-reads of a row may be served
by a cache. From traffic alone the shard path should take about
(3 * V/2) / (4 * V) = 0.375 of the full kernel's time.

    python scripts/bench_vocab_parallel_ce.py

The printed lines are also written to --out when given; a recorded run is in
profiles/vocab_parallel_ce.md.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, restore):
    restore()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    return start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--shard-width", type=int, default=64128)
    ap.add_argument("--tp", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocab_parallel_ce: needs a GPU (no CPU fallback)")
    from dlrover_amd.ops import ce_shard_finish, ce_shard_stats
    from dlrover_amd.ops.api import hip_ops

    ext = hip_ops()
    dev = torch.device("cuda:0")
    n, vs, tp = args.rows, args.shard_width, args.tp
    v = vs * tp
    gen = torch.Generator(device=dev).manual_seed(0)
    full_src = (torch.randn(n, v, device=dev, generator=gen) * 2.0).bfloat16()
    shard_src = full_src[:, :vs].contiguous()  # rank 0's columns
    full = torch.empty_like(full_src)
    shard = torch.empty_like(shard_src)
    targets = torch.randint(0, v, (n,), device=dev, generator=gen).int()
    targets[::97] = -100
    scale = 1.0 / max(int((targets != -100).sum()), 1)
    # the other ranks' stats only enter the [tp, N, 3] combine: take them from
    # the real columns once, outside the timed region
    other = [
        ce_shard_stats(full_src[:, r * vs:(r + 1) * vs].contiguous(), targets, r * vs)
        for r in range(1, tp)
    ]
    state = {}

    def run_stats():
        state["stats"] = ce_shard_stats(shard, targets, 0)

    def run_finish():
        ce_shard_finish(shard, targets, 0, state["stats_all"], scale)

    def run_shard():
        stats = ce_shard_stats(shard, targets, 0)
        ce_shard_finish(shard, targets, 0, torch.stack([stats] + other), scale)

    def run_full():
        ext.cross_entropy_fwd_bwd(full, targets, -100, scale, True)

    def restore_shard():
        shard.copy_(shard_src)

    def restore_full():
        full.copy_(full_src)

    run_stats()
    state["stats_all"] = torch.stack([state["stats"]] + other)
    variants = [
        ("shard stats", run_stats, restore_shard, 1 * n * vs * 2),
        ("shard finish", run_finish, restore_shard, 2 * n * vs * 2),
        ("shard stats+finish", run_shard, restore_shard, 3 * n * vs * 2),
        ("full-vocab fused", run_full, restore_full, 4 * n * v * 2),
    ]
    for _, fn, restore, _ in variants:
        for _ in range(args.warmup):
            restore()
            fn()
    events = {name: [] for name, *_ in variants}
    for _ in range(args.reps):
        for name, fn, restore, _ in variants:
            for _ in range(args.iters):
                events[name].append(timed(fn, restore))
    torch.cuda.synchronize()

    lines = [
        f"bench_vocab_parallel_ce: {torch.cuda.get_device_name(0)}, N={n}, "
        f"Vs={vs}, tp={tp}, V={v}, bf16 logits",
        f"{args.reps} alternating repetitions x {args.iters} calls, "
        f"{args.warmup} warm-up calls; device events per call; "
        "GB/s = algorithmic bytes / median",
    ]
    med = {}
    for name, _, _, nbytes in variants:
        us = sorted(s.elapsed_time(e) * 1e3 for s, e in events[name])
        med[name] = us[len(us) // 2]
        lines.append(
            f"{name:<20} median {med[name]:9.1f} us  min {us[0]:9.1f}  "
            f"max {us[-1]:9.1f}  {nbytes / med[name] / 1e3:7.0f} GB/s"
        )
    ratio = med["shard stats+finish"] / med["full-vocab fused"]
    lines.append(
        f"shard stats+finish / full-vocab fused = {ratio:.3f} "
        f"(from traffic alone: {3 * vs / (4 * v):.3f})"
    )
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
