"""Expert GEMMs of one MoEMLP: the library's grouped_mm behind moe_dispatch
against ops/csrc/moe_gemm.hip with the dispatch fused in.

GPU only — without a device this script fails.

One call is the pair of grouped GEMMs of an MoEMLP, gate_up [E, H, 2I] then
down [E, I, H] with the SwiGLU between them, forward and backward (dx and both
dw): (a) library = moe_dispatch + moe_grouped_mm(impl="library"),
(b) hip = moe_grouped_mm(impl="hip", gather=...). Mixtral-like shapes, R rows
over E experts, once split evenly and once with half of all rows in expert 0,
which shows what the unsplit weight gradient costs.

The variants alternate in one process; forward and backward are timed with
device events inside every call; medians over the repetitions with their
spread. TFLOP/s = 2 R K N per GEMM, 3 GEMMs per layer and direction pair.
Nothing here is enforced; the numbers are reported.

    python scripts/bench_moe_gemm.py --out profiles/moe_gemm.txt
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def routing(T, k, E, skewed, dev):
    """topk_idx [T, k]: even counts, or slot 0 of every token on expert 0."""
    t = torch.arange(T, device=dev).unsqueeze(1)
    j = torch.arange(k, device=dev).unsqueeze(0)
    idx = (t * k + j) % E
    if skewed:
        idx = 1 + (t * (k - 1) + j - 1) % (E - 1)
        idx[:, 0] = 0
    return idx.int()


def timed_calls(fn, steps):
    """(forward ms, backward ms) per call over `steps` calls."""
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
             for _ in range(steps)]
    for m in marks:
        fn(m)
    marks[-1][2].synchronize()
    fwd = sum(m[0].elapsed_time(m[1]) for m in marks) / steps
    bwd = sum(m[1].elapsed_time(m[2]) for m in marks) / steps
    return fwd, bwd


def med(xs):
    return statistics.median(xs)


def spread(xs):
    return (max(xs) - min(xs)) / med(xs) * 100


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inner", type=int, default=14336)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_gemm: needs a GPU (no CPU fallback)")
    from dlrover_amd.ops import api, moe_dispatch, moe_grouped_mm, moe_sort, swiglu

    api.hip_ops()
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    R, E, k, H, I = args.rows, args.experts, args.topk, args.hidden, args.inner
    T = R // k
    torch.manual_seed(0)
    x = torch.randn(T, H, device=dev, dtype=bf, requires_grad=True)
    w1 = (torch.randn(E, H, 2 * I, device=dev, dtype=bf) * 0.02).requires_grad_()
    w2 = (torch.randn(E, I, H, device=dev, dtype=bf) * 0.02).requires_grad_()
    dy = torch.randn(R, H, device=dev, dtype=bf)
    flops = 2 * R * (H * 2 * I + I * H)
    xp_mb = R * H * 2 / 1e6
    lines = [
        f"bench_moe_gemm: {torch.cuda.get_device_name(0)}, torch "
        f"{torch.__version__}",
        f"R = {R} rows (T = {T}, k = {k}), E = {E}, H = {H}, I = {I}, bf16; "
        f"{args.steps} calls per window, {args.reps} alternating repetitions, "
        f"{args.warmup} warm-up calls; device-event ms per call (measured); "
        "TFLOP/s = 2 R K N per GEMM / time (derived)",
        f"xp [R, H]: {xp_mb:.0f} MB that impl='hip' neither writes in the "
        "forward nor keeps for the backward (derived from the shapes)",
    ]
    for split in ("even", "half of the rows in expert 0"):
        offs, row_of_slot, slot_of_row = moe_sort(
            routing(T, k, E, split != "even", dev), E)

        def call(impl):
            def fn(marks):
                x.grad = w1.grad = w2.grad = None
                marks[0].record()
                if impl == "hip":
                    h = moe_grouped_mm(x, w1, offs, impl="hip",
                                       gather=(slot_of_row, row_of_slot, k))
                else:
                    h = moe_grouped_mm(
                        moe_dispatch(x, slot_of_row, row_of_slot, k), w1, offs)
                y = moe_grouped_mm(swiglu(h), w2, offs, impl=impl)
                marks[1].record()
                y.backward(dy)
                marks[2].record()
            return fn

        variants = {"library": call("library"), "hip": call("hip")}
        grads = {}
        for name, fn in variants.items():
            timed_calls(fn, args.warmup)
            grads[name] = [t.grad.float() for t in (x, w1, w2)]
        worst = max(
            ((a - b).abs().max() / b.abs().max()).item()
            for a, b in zip(grads["hip"], grads["library"]))
        del grads
        res = {name: ([], []) for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                f, b = timed_calls(fn, args.steps)
                res[name][0].append(f)
                res[name][1].append(b)
        counts = torch.diff(offs, prepend=offs.new_zeros(1)).tolist()
        lines.append(
            f"  split: {split}; rows per expert {counts}; dx, dw1, dw2 of hip "
            f"against library: worst max|diff| / max|ref| = {worst:.2e}")
        for d, what, mult in ((0, "forward", 1), (1, "backward", 2)):
            base = med(res["library"][d])
            for name in variants:
                v = res[name][d]
                lines.append(
                    f"    {what:<9}{name:<8}"
                    + " ".join(f"{t:8.3f}" for t in v)
                    + f"   median {med(v):8.3f}  spread {spread(v):5.1f}%"
                    + f"  {mult * flops / med(v) / 1e9:6.0f} TFLOP/s"
                    + f"  x{med(v) / base:5.3f} of library")
    lines.append(f"library fallbacks to the per-expert loop: "
                 f"{api.moe_grouped_mm_fallbacks}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
