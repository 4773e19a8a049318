"""Blocking-save and device-restore time of a flash-checkpoint snapshot, with
checkpoint checksums on or off.

Builds a synthetic training state with the tensor shapes of
LlamaConfig.small_1b (bf16 params plus fp32 master, exp_avg and exp_avg_sq,
about 15 GB), saves it to a shared-memory segment with block=False (the time
the training loop is stalled: the device snapshot) and restores it to the
device, several times each, and prints one JSON line with the medians and the
min-max spread.

    python scripts/bench_ckpt_integrity.py --checksum off
    python scripts/bench_ckpt_integrity.py --checksum on

With --checksum off the handler is built without the keyword, so the same
script measures a tree from before the option existed.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build_state(layers: int, odd_offset: bool = False):
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig.small_1b()
    n_layers = layers if layers > 0 else cfg.n_layers
    # only the shapes are needed: build ONE layer on the host and repeat it
    cfg.n_layers = 1
    cfg.max_seq_len = 64
    one = LlamaForCausalLM(cfg)
    shapes = []
    for name, p in one.named_parameters():
        if ".0." in name:
            shapes += [(name.replace(".0.", f".{k}.", 1), p.shape)
                       for k in range(n_layers)]
        else:
            shapes.append((name, p.shape))
    del one
    g = torch.Generator(device="cuda").manual_seed(0)
    params, opt = {}, {}
    for i, (name, shape) in enumerate(shapes):
        p = torch.empty(shape, device="meta")
        master = torch.randn(p.shape, device="cuda", generator=g) * 0.02
        params[name] = master.bfloat16()
        if odd_offset:
            # a view one element into its storage: 2-byte aligned, so the
            # pack kernel takes its word-wise path for the whole tensor
            flat = torch.empty(p.numel() + 1, dtype=torch.bfloat16, device="cuda")
            flat[1:].copy_(params[name].reshape(-1))
            params[name] = flat[1:].view(shape)
        opt[i] = {
            "master_param": master,
            "exp_avg": torch.randn(p.shape, device="cuda", generator=g) * 1e-3,
            "exp_avg_sq": torch.rand(p.shape, device="cuda", generator=g) * 1e-6,
            "step": 100,
        }
    return {"model": params, "optimizer": {"state": opt}, "step": 100}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checksum", choices=("on", "off"), default="off")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0,
                    help="override n_layers (0: the 22 of small_1b)")
    ap.add_argument("--odd-offset", action="store_true",
                    help="make every bf16 param a view at an odd element "
                         "offset (not 16-byte aligned)")
    ap.add_argument("--threads", type=int, default=16,
                    help="upper bound on CPU threads")
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(args.threads, 16, torch.get_num_threads())))
    if not torch.cuda.is_available():
        raise SystemExit("bench_ckpt_integrity needs a GPU; nothing was measured")

    from dlrover_amd.trainer.flash_checkpoint.shm_handler import SharedMemoryHandler

    name = f"ckpt_integrity_bench_{os.getpid()}"
    if args.checksum == "on":
        handler = SharedMemoryHandler(name, checksum=True)
    else:
        handler = SharedMemoryHandler(name)
    state = build_state(args.layers, args.odd_offset)
    torch.cuda.synchronize()
    dev = torch.device("cuda")
    saves, restores = [], []
    try:
        # warm-up: sizes and pins the segment, allocates the staging buffer,
        # loads the kernels
        handler.save_state_dict(1, state, block=False)
        handler.wait_drained()
        payload = handler.read_meta().payload_bytes
        n_tensors = len(handler.read_meta().tensors)
        for r in range(args.repeats):
            torch.cuda.synchronize()
            saves.append(handler.save_state_dict(2 + r, state, block=False))
            handler.wait_drained()
        out = handler.load_state_dict(device=dev)  # warm-up
        del out
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = handler.load_state_dict(device=dev)
            torch.cuda.synchronize()
            restores.append(time.perf_counter() - t0)
            del out
        chunked = bool(handler._stager._chunked)
    finally:
        handler.unlink()

    def stats(xs):
        return {
            "median_ms": round(statistics.median(xs) * 1e3, 3),
            "min_ms": round(min(xs) * 1e3, 3),
            "max_ms": round(max(xs) * 1e3, 3),
        }

    print(json.dumps({
        "bench": "ckpt_integrity",
        "checksum": args.checksum,
        "odd_offset_bf16": args.odd_offset,
        "payload_gb": round(payload / 1e9, 3),
        "tensors": n_tensors,
        "chunked_staging": chunked,
        "repeats": args.repeats,
        "blocking_save": stats(saves),
        "device_restore": stats(restores),
    }))


if __name__ == "__main__":
    main()
