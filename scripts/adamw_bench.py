"""Optimizer-step microbenchmark: per-parameter vs multi-tensor FusedAdamW.

GPU only — there is no CPU fallback; without a device this script fails.

Allocates optimizer state for the parameter shapes of LlamaConfig.small_1b()
(no model forward), bf16 params and bf16 gradients, and times opt.step() with
device events for three variants, alternating in one process:

  (a) per_param     today's default path, one launch per parameter
  (b) multi_tensor  FusedAdamW(multi_tensor=True)
  (c) clip          FusedAdamW(max_grad_norm=1.0): norm kernels + update

The whole alternation runs --reps times (default 3) and the spread over the
repetitions is reported. Expectation, from traffic alone: (c) reads the bf16
gradients twice, 30 B/param against 28, so (c) <= ~1.07x (a), 1.10x allowed
for noise (or the measured spread when that is larger); (b) <= (a). These
are reported, not enforced. After the timed runs (a) and (b), which saw the
same seeded inputs and the same number of steps, are compared with
assert_close(rtol=1e-4, atol=1e-5).

    python scripts/adamw_bench.py --out profiles/adamw_multi_tensor.txt
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def param_shapes():
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    # every block has the same shapes: build one layer, repeat it n_layers
    # times (building all 1.1 G parameters on the host just to read their
    # shapes takes minutes)
    cfg = LlamaConfig.small_1b(max_seq_len=64)
    n_layers, cfg.n_layers = cfg.n_layers, 1
    model = LlamaForCausalLM(cfg)
    shapes = []
    for name, p in model.named_parameters():
        reps = n_layers if name.startswith("blocks.0.") else 1
        shapes += [tuple(p.shape)] * reps
    return shapes


def make_variant(name, shapes, grads, dev, **opt_kw):
    from dlrover_amd.ops import FusedAdamW

    span = opt_kw.pop("span_elems", 0)
    gen = torch.Generator(device=dev).manual_seed(0)  # same init per variant
    params = []
    for shape, g in zip(shapes, grads):
        p = torch.nn.Parameter(
            (torch.randn(shape, device=dev, generator=gen) * 0.02).bfloat16()
        )
        p.grad = g  # gradients are only read: shared by every variant
        params.append(p)
    opt = FusedAdamW(params, lr=1e-4, weight_decay=0.1, **opt_kw)
    opt._span_elems = span
    return dict(name=name, params=params, opt=opt, dev_ms=[], host_ms=[])


def time_steps(variant, steps):
    opt = variant["opt"]
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(steps):
        opt.step()
    end.record()
    host = time.perf_counter() - t0  # enqueue only: no sync inside
    torch.cuda.synchronize()
    variant["dev_ms"].append(start.elapsed_time(end) / steps)
    variant["host_ms"].append(host * 1e3 / steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spans", default="",
                    help="comma-separated span_elems: extra multi_tensor "
                         "variants at forced spans (diagnostic)")
    ap.add_argument("--out", default="profiles/adamw_multi_tensor.txt")
    args = ap.parse_args()
    if args.steps < 50:
        ap.error("--steps must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("adamw_bench: needs a GPU (no CPU fallback)")
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
        make_variant("per_param", shapes, grads, dev),
        make_variant("multi_tensor", shapes, grads, dev, multi_tensor=True),
        make_variant("clip", shapes, grads, dev, max_grad_norm=1.0),
    ]
    for s in filter(None, args.spans.split(",")):
        variants.append(make_variant(
            f"multi_tensor@span{s}", shapes, grads, dev, multi_tensor=True,
            span_elems=int(s)))
        variants.append(make_variant(
            f"clip@span{s}", shapes, grads, dev, max_grad_norm=1.0,
            span_elems=int(s)))

    for v in variants:
        for _ in range(args.warmup):
            v["opt"].step()
    for _ in range(args.reps):
        for v in variants:
            time_steps(v, args.steps)

    lines = [
        f"adamw_bench: {torch.cuda.get_device_name(0)}, small_1b shapes, "
        f"{len(shapes)} tensors, {n_elem / 1e9:.3f} G params, bf16 grads",
        f"{args.steps} steps per window, {args.reps} alternating repetitions, "
        f"{args.warmup} warm-up steps; device-event ms per step "
        "(host enqueue ms per step in brackets)",
    ]
    base = variants[0]
    for v in variants:
        d = v["dev_ms"]
        med = sorted(d)[len(d) // 2]
        base_med = sorted(base["dev_ms"])[len(d) // 2]
        gbs = n_elem * (30 if v["opt"].max_grad_norm else 28) / med / 1e6
        lines.append(
            f"{v['name']:<28} "
            + " ".join(f"{x:8.3f}" for x in d)
            + f"   median {med:8.3f}  spread {(max(d) - min(d)) / med * 100:5.1f}%"
            + f"  x{med / base_med:5.3f} of per_param  {gbs:7.0f} GB/s  ["
            + " ".join(f"{x:.3f}" for x in v["host_ms"]) + "]"
        )
    lines.append(f"clip: last_grad_norm = {float(variants[2]['opt'].last_grad_norm):.6f}")

    # same seeded inputs, same number of steps: (a) and (b) must agree
    oa, ob = variants[0]["opt"], variants[1]["opt"]
    for pa, pb in zip(variants[0]["params"], variants[1]["params"]):
        for k in ("master_param", "exp_avg", "exp_avg_sq"):
            torch.testing.assert_close(
                ob.state[pb][k], oa.state[pa][k], rtol=1e-4, atol=1e-5
            )
    lines.append("per_param vs multi_tensor after the timed runs: "
                 "assert_close(rtol=1e-4, atol=1e-5) passed")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
