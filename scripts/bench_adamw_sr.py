"""Master-free FusedAdamW (stochastic rounding) against fp32 master weights:
optimizer step, state size and device restore, for both moment formats.

GPU only — there is no CPU fallback; without a device this script fails.

Allocates optimizer state for the parameter shapes of LlamaConfig.small_1b()
(no model forward), bf16 params and bf16 gradients, for four optimizers:

  multi_tensor   FusedAdamW(multi_tensor=True): fp32 master, fp32 moments
  sr             the same with master_weights=False
  fp8            FusedAdamW(moments="fp8"): fp32 master, FP8 moments
  fp8_sr         the same with master_weights=False

Step: opt.step() timed with device events, all four alternating in one
process; the alternation runs --reps times and medians are reported with the
spread of each base. Bytes moved per parameter, from the formats alone: 28
and 18 (fp32 moments), 16.03 and 10.03 (FP8 moments).

Restore: what a checkpoint must hold to rebuild weights and optimizer — the
optimizer's state_dict, plus the bf16 weights where no master holds them — is
saved to a shared-memory segment and restored to the device, --ckpt-reps
times after a warm-up. Nothing here is enforced; the numbers are reported.

    python scripts/bench_adamw_sr.py --out profiles/adamw_sr.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.adamw_bench import make_variant, param_shapes, time_steps  # noqa: E402

# (name, base, optimizer arguments, bytes the update moves per parameter)
VARIANTS = [
    ("multi_tensor", None, dict(multi_tensor=True), 28.0),
    ("sr", "multi_tensor", dict(master_weights=False), 18.0),
    ("fp8", None, dict(moments="fp8"), 16 + 8 / 256),
    ("fp8_sr", "fp8", dict(moments="fp8", master_weights=False), 10 + 8 / 256),
]


def time_restore(variant, reps):
    from dlrover_amd.trainer.flash_checkpoint.shm_handler import SharedMemoryHandler

    handler = SharedMemoryHandler(f"adamw_sr_bench_{os.getpid()}_{variant['name']}")
    opt = variant["opt"]
    state = {"optimizer": opt.state_dict(), "step": 1}
    if not opt.master_weights:
        state["model"] = [p.detach() for p in variant["params"]]
    dev = torch.device("cuda:0")
    restores = []
    try:
        handler.save_state_dict(1, state, block=False)
        handler.wait_drained()
        payload = handler.read_meta().payload_bytes
        out = handler.load_state_dict(device=dev)  # warm-up
        del out
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = handler.load_state_dict(device=dev)
            torch.cuda.synchronize()
            restores.append((time.perf_counter() - t0) * 1e3)
            del out
    finally:
        handler.unlink()
    variant.update(payload=payload, restore_ms=restores)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ckpt-reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16,
                    help="upper bound on CPU threads")
    ap.add_argument("--out", default="profiles/adamw_sr.txt")
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(args.threads, 16, torch.get_num_threads())))
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_sr: needs a GPU (no CPU fallback)")
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
    variants = {
        name: dict(make_variant(name, shapes, grads, dev, **kw), base=base, bpp=bpp)
        for name, base, kw, bpp in VARIANTS
    }
    for v in variants.values():
        for _ in range(args.warmup):
            v["opt"].step()
    for _ in range(args.reps):
        for v in variants.values():
            time_steps(v, args.steps)
    for v in variants.values():
        time_restore(v, args.ckpt_reps)

    med = statistics.median

    def spread(xs):
        return (max(xs) - min(xs)) / med(xs) * 100

    lines = [
        f"bench_adamw_sr: {torch.cuda.get_device_name(0)}, small_1b shapes, "
        f"{len(shapes)} tensors, {n_elem / 1e9:.3f} G params, bf16 grads",
        f"step: {args.steps} steps per window, {args.reps} alternating "
        f"repetitions, {args.warmup} warm-up steps; device-event ms per step; "
        "GB/s = derived bytes per parameter over the median",
    ]
    for v in variants.values():
        d = v["dev_ms"]
        ref = variants[v["base"]] if v["base"] else v
        lines.append(
            f"  {v['name']:<13}" + " ".join(f"{x:7.3f}" for x in d)
            + f"   median {med(d):7.3f}  spread {spread(d):5.1f}%"
            + f"  x{med(d) / med(ref['dev_ms']):5.3f} of {ref['name']}"
            + f"  {v['bpp']:5.2f} B/param {n_elem * v['bpp'] / med(d) / 1e6:6.0f} GB/s"
        )
    lines.append("state_nbytes (optimizer state; the bf16 weights are 2 B/param more "
                 "in every variant):")
    for v in variants.values():
        ref = variants[v["base"]] if v["base"] else v
        nb, rb = v["opt"].state_nbytes(), ref["opt"].state_nbytes()
        lines.append(
            f"  {v['name']:<13}{nb / 1e9:7.3f} GB  {nb / n_elem:5.2f} B/param  "
            f"x{nb / rb:6.4f} of {ref['name']}"
        )
    lines.append(
        f"device restore from the shared-memory segment (state_dict, plus the "
        f"bf16 weights where there is no master), {args.ckpt_reps} repetitions "
        "after a warm-up; ms"
    )
    for v in variants.values():
        d = v["restore_ms"]
        ref = variants[v["base"]] if v["base"] else v
        lines.append(
            f"  {v['name']:<13}" + " ".join(f"{x:8.1f}" for x in d)
            + f"   median {med(d):8.1f}  spread {spread(d):5.1f}%"
            + f"  x{med(d) / med(ref['restore_ms']):5.3f} of {ref['name']}"
            + f"  payload {v['payload'] / 1e9:.3f} GB"
        )
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
