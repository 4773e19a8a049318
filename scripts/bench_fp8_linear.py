"""FP8 linear layers: the fused cast path against the torch composite it
replaces, and one Fp8Linear forward + backward against nn.Linear in bf16.

GPU only — without a device this script fails.

cast: for a bf16 [R, C] tensor, (a) fused = ops.fp8_quantize(rowwise and
colwise): the two-stage absmax and the cast + transpose kernel, 6 bytes per
element by construction (2 read for the absmax, 2 read and 1 + 1 written for
the cast); (b) composite = abs().amax(), divide, .to(float8_e4m3fn),
.t().contiguous(). The absmax and the cast are also timed alone.

layer: forward + backward (dx and dw) of one linear at the four llama3_8b
projection shapes with M tokens, (a) nn.Linear bf16, (b) ops.Fp8Linear.

The variants alternate in one process; every window is timed with device
events; medians over the repetitions, the base's own spread next to them.
Nothing here is enforced; the numbers are reported.

    python scripts/bench_fp8_linear.py --out profiles/fp8_linear.txt
    # kernel split of the fp8 layer, in a run of its own:
    rocprofv3 --kernel-trace --stats -- \\
        python scripts/bench_fp8_linear.py --part layer --variants fp8 --reps 1
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CAST_SHAPES = [(8192, 4096), (8192, 14336), (14336, 4096)]
# (name, N, K) of llama3_8b: hidden 4096, 32 + 2 x 8 heads of 128, mlp 14336
LAYER_SHAPES = [
    ("qkv_proj", 6144, 4096),
    ("o_proj", 4096, 4096),
    ("gate_up_proj", 28672, 4096),
    ("down_proj", 4096, 14336),
]


def window_ms(fn, steps):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def alternate(variants, steps, warmup, reps):
    """{name: [ms per call, one per repetition]}, the variants interleaved."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    out = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            out[name].append(window_ms(fn, steps))
    return out


def med(xs):
    return statistics.median(xs)


def spread(xs):
    return (max(xs) - min(xs)) / med(xs) * 100


def bench_cast(args, dev, lines):
    from dlrover_amd.ops import fp8_quantize

    lines.append(
        f"cast: bf16 [R, C] -> e4m3 codes [R, C] and [C, R]; {args.steps} calls "
        f"per window, {args.reps} alternating repetitions, {args.warmup} warm-up "
        "calls; device-event ms per call (measured); GB/s = bytes the variant "
        "must move / time (derived: fused 6 B/elem, absmax 2, cast 4)"
    )
    for R, C in CAST_SHAPES:
        x = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
        _, _, scale = fp8_quantize(x)

        def fused():
            return fp8_quantize(x, "e4m3", True, True)

        # a device divisor: dividing by a Python number multiplies by its
        # reciprocal on the device, which is not the format's fp32 division
        fmax = torch.full((), 448.0, device=dev)

        def composite():
            s = x.abs().amax().float() / fmax
            y = (x.float() / s).to(torch.float8_e4m3fn)
            return y, y.view(torch.uint8).t().contiguous(), s

        def absmax_only():
            return fp8_quantize(x, "e4m3", False, False)

        def cast_only():
            return fp8_quantize(x, "e4m3", True, True, scale=scale)

        a, at, s = fused()
        b, bt, sb = composite()
        same = (torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                and torch.equal(at.view(torch.uint8), bt) and bool(s[0] == sb))
        res = alternate(
            {"composite": composite, "fused": fused, "absmax": absmax_only,
             "cast": cast_only}, args.steps, args.warmup, args.reps)
        n = R * C
        lines.append(f"  [{R}, {C}]  ({n * 2 / 1e6:.0f} MB bf16; fused codes "
                     f"{'equal' if same else 'DIFFER FROM'} the composite's)")
        base = med(res["composite"])
        for name, bpe in (("composite", None), ("fused", 6), ("absmax", 2),
                          ("cast", 4)):
            d = res[name]
            gbs = f"{n * bpe / med(d) / 1e6:7.0f} GB/s" if bpe else " " * 12
            lines.append(
                f"    {name:<10}" + " ".join(f"{v:8.4f}" for v in d)
                + f"   median {med(d):8.4f}  spread {spread(d):5.1f}%  {gbs}"
                + f"  x{med(d) / base:5.3f} of composite"
            )
        del x


def bench_layer(args, dev, lines):
    from dlrover_amd.ops import Fp8Linear

    M = args.tokens
    lines.append(
        f"layer: forward + backward (dx, dw) at M = {M} tokens, bf16 "
        f"parameters; {args.layer_steps} calls per window, {args.reps} "
        f"alternating repetitions, {args.warmup} warm-up calls; device-event ms "
        "per call (measured); TFLOP/s = 6 M N K / time (derived)"
    )
    for name, N, K in LAYER_SHAPES:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
        torch.manual_seed(0)
        mods = {}
        if "bf16" in args.variants:
            mods["bf16"] = torch.nn.Linear(K, N, bias=False, device=dev,
                                           dtype=torch.bfloat16)
        if "fp8" in args.variants:
            mods["fp8"] = Fp8Linear(K, N, bias=False, device=dev,
                                    dtype=torch.bfloat16)

        def run(mod):
            def fn():
                x.grad = None
                mod.weight.grad = None
                mod(x).backward(dy)
            return fn

        res = alternate({k: run(m) for k, m in mods.items()},
                        args.layer_steps, args.warmup, args.reps)
        lines.append(f"  {name}  N = {N}, K = {K}")
        base = med(next(iter(res.values())))
        for k, d in res.items():
            lines.append(
                f"    {k:<6}" + " ".join(f"{v:8.3f}" for v in d)
                + f"   median {med(d):8.3f}  spread {spread(d):5.1f}%"
                + f"  {6 * M * N * K / med(d) / 1e9:6.0f} TFLOP/s"
                + f"  x{med(d) / base:5.3f} of {next(iter(res))}"
            )
        del x, dy, mods


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=("all", "cast", "layer"), default="all")
    ap.add_argument("--variants", default="bf16,fp8",
                    help="layer variants to run, the first is the base")
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--layer-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.variants = [v for v in args.variants.split(",") if v]
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_linear: needs a GPU (no CPU fallback)")
    from dlrover_amd.ops import fp8_linear_supported
    from dlrover_amd.ops.api import hip_ops

    hip_ops()
    dev = torch.device("cuda:0")
    lines = [f"bench_fp8_linear: {torch.cuda.get_device_name(0)}, "
             f"torch {torch.__version__}"]
    if args.part in ("all", "cast"):
        bench_cast(args, dev, lines)
    if args.part in ("all", "layer"):
        if "fp8" in args.variants and not fp8_linear_supported():
            raise SystemExit("bench_fp8_linear: torch._scaled_mm rejects FP8 here")
        bench_layer(args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
