"""FP8 block-scaled moments against fp32 moments: optimizer step, blocking
checkpoint save and device restore.

GPU only — there is no CPU fallback; without a device this script fails.

Allocates optimizer state for the parameter shapes of LlamaConfig.small_1b()
(no model forward), bf16 params and bf16 gradients, for two optimizers:

  (a) multi_tensor  FusedAdamW(multi_tensor=True): fp32 moments, the batched
                    path this feature leaves untouched
  (b) fp8           FusedAdamW(moments="fp8")

Step: opt.step() timed with device events, the two alternating in one
process; the alternation runs --reps times and the spread over the
repetitions is reported next to the medians. Expected from bytes alone: 16
B/param against 28.

Checkpoint: each optimizer's state_dict is saved to a shared-memory segment
with block=False (the time the training loop is stalled) and restored to the
device, --ckpt-reps times each after a warm-up. Expected from bytes alone:
6.03 / 12. Nothing here is enforced; the numbers are reported.

    python scripts/bench_adamw_fp8.py --out profiles/adamw_fp8.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.adamw_bench import make_variant, param_shapes, time_steps  # noqa: E402


def time_checkpoint(variant, reps):
    from dlrover_amd.trainer.flash_checkpoint.shm_handler import SharedMemoryHandler

    handler = SharedMemoryHandler(f"adamw_fp8_bench_{os.getpid()}_{variant['name']}")
    state = {"optimizer": variant["opt"].state_dict(), "step": 1}
    dev = torch.device("cuda:0")
    saves, restores = [], []
    try:
        # warm-up: sizes and pins the segment, allocates the staging buffer
        handler.save_state_dict(1, state, block=False)
        handler.wait_drained()
        payload = handler.read_meta().payload_bytes
        for r in range(reps):
            torch.cuda.synchronize()
            saves.append(handler.save_state_dict(2 + r, state, block=False))
            handler.wait_drained()
        out = handler.load_state_dict(device=dev)  # warm-up
        del out
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = handler.load_state_dict(device=dev)
            torch.cuda.synchronize()
            restores.append(time.perf_counter() - t0)
            del out
    finally:
        handler.unlink()
    variant.update(payload=payload, save_ms=[s * 1e3 for s in saves],
                   restore_ms=[s * 1e3 for s in restores])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ckpt-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16,
                    help="upper bound on CPU threads")
    ap.add_argument("--out", default="profiles/adamw_fp8.txt")
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(args.threads, 16, torch.get_num_threads())))
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_fp8: needs a GPU (no CPU fallback)")
    from dlrover_amd.ops.api import hip_ops

    hip_ops()
    dev = torch.device("cuda:0")
    shapes = param_shapes()
    n_elem = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [
        (torch.randn(s, device=dev, generator=gen) * 1e-2).bfloat16()
        for s in shapes
    ]
    variants = [
        make_variant("multi_tensor", shapes, grads, dev, multi_tensor=True),
        make_variant("fp8", shapes, grads, dev, moments="fp8"),
    ]
    for v in variants:
        for _ in range(args.warmup):
            v["opt"].step()
    for _ in range(args.reps):
        for v in variants:
            time_steps(v, args.steps)
    n_fp8 = sum(
        p.numel() for p in variants[1]["params"]
        if "exp_avg_sq_root" in variants[1]["opt"].state[p]
    )
    for v in variants:
        time_checkpoint(v, args.ckpt_reps)

    def med(xs):
        return statistics.median(xs)

    def spread(xs):
        return (max(xs) - min(xs)) / med(xs) * 100

    lines = [
        f"bench_adamw_fp8: {torch.cuda.get_device_name(0)}, small_1b shapes, "
        f"{len(shapes)} tensors, {n_elem / 1e9:.3f} G params "
        f"({n_fp8 / n_elem * 100:.2f}% with fp8 moments), bf16 grads",
        f"step: {args.steps} steps per window, {args.reps} alternating "
        f"repetitions, {args.warmup} warm-up steps; device-event ms per step",
    ]
    base = variants[0]
    for v in variants:
        d = v["dev_ms"]
        bpp = 28 if v is base else (16 + 8 / 256)
        lines.append(
            f"  {v['name']:<14}" + " ".join(f"{x:8.3f}" for x in d)
            + f"   median {med(d):8.3f}  spread {spread(d):5.1f}%"
            + f"  x{med(d) / med(base['dev_ms']):5.3f} of multi_tensor"
            + f"  {n_elem * bpp / med(d) / 1e6:7.0f} GB/s"
        )
    lines.append(
        f"state: multi_tensor {base['opt'].state_nbytes() / 1e9:.3f} GB, "
        f"fp8 {variants[1]['opt'].state_nbytes() / 1e9:.3f} GB "
        f"(x{variants[1]['opt'].state_nbytes() / base['opt'].state_nbytes():.4f})"
    )
    lines.append(
        f"checkpoint: optimizer state_dict through a shared-memory segment, "
        f"{args.ckpt_reps} repetitions after a warm-up; ms"
    )
    for key, label in (("save_ms", "blocking save"), ("restore_ms", "device restore")):
        for v in variants:
            d = v[key]
            lines.append(
                f"  {label:<15}{v['name']:<14}" + " ".join(f"{x:9.1f}" for x in d)
                + f"   median {med(d):9.1f}  spread {spread(d):5.1f}%"
                + f"  x{med(d) / med(base[key]):5.3f} of multi_tensor"
                + f"  payload {v['payload'] / 1e9:.3f} GB"
            )
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
