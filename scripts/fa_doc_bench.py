"""Time document-masked flash attention against the causal path at the
flagship attention shape (B1 H32 HKV8 S4096 D128), forward and backward.

  (a) the causal path                      flash_attn_fwd / flash_attn_bwd
  (b) the doc path, one document of S      (what the DOC variant itself costs)
  (c) the doc path, S/512 documents of 512 and S/128 documents of 128

Every figure is the median over --reps timed windows of --iters calls each,
every window ended by a device synchronise; the cases alternate inside one
repetition so drift hits them alike. min/max over the repetitions is the
spread. "ideal" is the FLOP ratio sum(len_i^2) / S^2 a document layout allows;
"of ideal" is ideal / (measured time ratio to (a)).

Run on a GPU box:  python3 scripts/fa_doc_bench.py
--causal-only times (a) alone and needs no doc bindings, so the same script
measures an older checkout for an A/B of the causal kernels.
"""

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dlrover_amd.ops.api import hip_ops  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=1)
    p.add_argument("--H", type=int, default=32)
    p.add_argument("--HKV", type=int, default=8)
    p.add_argument("--S", type=int, default=4096)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--causal-only", action="store_true")
    p.add_argument("--json", default="", help="also write the figures here")
    args = p.parse_args()
    if args.reps < 5:
        p.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("fa_doc_bench: needs a GPU (no CPU fallback for a timing)")
    B, H, HKV, S, D = args.B, args.H, args.HKV, args.S, 128
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, HKV, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    ext = hip_ops()

    cases = {}  # name -> (fwd fn, bwd fn, ideal ratio)
    out, lse = ext.flash_attn_fwd(q, k, v, scale)
    dout = torch.randn_like(out)
    cases["a causal"] = (
        lambda: ext.flash_attn_fwd(q, k, v, scale),
        lambda o=out, l=lse: ext.flash_attn_bwd(q, k, v, o, dout, l, scale),
        1.0,
    )
    if not args.causal_only:
        from dlrover_amd.ops.api import doc_end_from_start

        for tag, n in (("b doc 1x%d" % S, S), ("c doc %dx512" % (S // 512), 512),
                       ("c doc %dx128" % (S // 128), 128)):
            idx = torch.arange(S, device="cuda", dtype=torch.int32)
            ds = (idx - idx % n).expand(B, S).contiguous()
            de = doc_end_from_start(ds)
            o, l = ext.flash_attn_doc_fwd(q, k, v, scale, ds)
            cases[tag] = (
                lambda ds=ds: ext.flash_attn_doc_fwd(q, k, v, scale, ds),
                lambda o=o, l=l, ds=ds, de=de: ext.flash_attn_doc_bwd(
                    q, k, v, o, dout, l, scale, ds, de),
                (S // n) * n * n / (S * S),
            )

    times = {name: {"fwd": [], "bwd": []} for name in cases}
    for name, (f, b, _) in cases.items():
        for _ in range(args.warmup):
            f()
            b()
    for _ in range(args.reps):
        for name, (f, b, _) in cases.items():
            times[name]["fwd"].append(window(f, args.iters))
            times[name]["bwd"].append(window(b, args.iters))

    result = {"shape": dict(B=B, H=H, HKV=HKV, S=S, D=D), "reps": args.reps,
              "iters": args.iters, "cases": {}}
    base = {d: statistics.median(times["a causal"][d]) for d in ("fwd", "bwd")}
    print(f"B{B} H{H} HKV{HKV} S{S} D{D}; median of {args.reps} windows x "
          f"{args.iters} calls, ms [min..max]")
    for name, (_, _, ideal) in cases.items():
        row = {"ideal_ratio": ideal}
        line = f"{name:14s}"
        for d in ("fwd", "bwd"):
            ts = times[name][d]
            med = statistics.median(ts)
            ratio = med / base[d]
            row[d] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3,
                          max_ms=max(ts) * 1e3, ratio_to_causal=ratio,
                          fraction_of_ideal=ideal / ratio)
            line += (f"  {d} {med * 1e3:7.3f} [{min(ts) * 1e3:.3f}..{max(ts) * 1e3:.3f}]"
                     f" x{ratio:.3f} of (a)")
            if ideal < 1.0:
                line += f" ({ideal / ratio * 100:.0f}% of ideal {ideal:.4f})"
        result["cases"][name] = row
        print(line)
    print("RESULT " + json.dumps(result))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    if not args.causal_only:
        slow = [(n, d) for n, r in result["cases"].items() if n.startswith("c ")
                for d in ("fwd", "bwd") if r[d]["ratio_to_causal"] >= 1.0]
        if slow:
            sys.exit(f"fa_doc_bench: doc path not faster than causal: {slow}")


if __name__ == "__main__":
    main()
