"""Extending a KV cache by T tokens on the MI355X: one JSON line per shape.

Shapes: bf16, d = 128, [B][N][H][d], B = 8, H = 32, Hkv in {8, 32}; a cached prefix of 4096 or 8192 tokens and T = 256, 512, 2048 new
ones.  Three ways to the same result, on the same data:
  extend   device_ops.flash_attn_extend(..., k_new=, v_new=): one fused append + the extend kernels (128 rows per workgroup)
  loop     what a caller had before: ceil(T / 128) fused decode calls (flash_attn_decode(..., k_new=, v_new=)) of 128 tokens each over
           the same cache, the lengths advanced from slice to slice
  square   the other thing a caller had: throw the cache away and run the square causal forward (flash_attn_fwd_gqa) over all
           prefix + T tokens (it also recomputes the prefix's own rows: that is its price)
``--section empty``: T = len from an empty cache (prefix 0) against the square forward over the same T tokens: the price of this
kernel's simpler pipeline where the slot kernels are at home.  ``--section crossover``: T = 32 .. 256 after a prefix of 4096, extend
against the loop (one call up to 128 tokens, two above).
Per path: milliseconds per call (device events around ``--reps`` calls after ``--warmup``; ``--repeats`` such windows, median and
min .. max reported).  The workspaces are allocated once, outside the windows, as KVCache does.
A kernel trace is a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python tools/bench_extend.py --trace-workload HKV,PREFIX,T
    python tools/bench_extend.py --kernel-stats DIR/.../t_kernel_stats.csv
prints per kernel family the calls and the fastest / average time of one launch.

    python tools/bench_extend.py [--reps 10] [--warmup 3] [--repeats 5] > profiles/extend_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

B, H, D = 8, 32, 128
HKVS = (8, 32)
PREFIXES = (4096, 8192)
TS = (256, 512, 2048)
CROSSOVER_TS = (32, 64, 96, 128, 160, 192, 256)
STEP = 128   # the decode call's largest Nq


def window_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def spread(fn, reps, warmup, repeats):
    """median, min, max over ``repeats`` timed windows (the first one carries the warm-up)."""
    xs = [window_ms(fn, reps, warmup if i == 0 else 1) for i in range(repeats)]
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


class Case:
    """The tensors of one (Hkv, prefix, T): caches of capacity prefix + T holding the prefix, the T new tokens' q, k and v, and the
    three paths as callables.  Every path leaves the caches as it found them in rows 0 .. prefix-1, so the paths can alternate."""

    def __init__(self, hkv, prefix, T, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.hkv, self.prefix, self.T, self.N = hkv, prefix, T, prefix + T
        self.q_all, self.k_all, self.v_all = rnd(B, self.N, H, D), rnd(B, self.N, hkv, D), rnd(B, self.N, hkv, D)
        self.kc, self.vc = self.k_all.clone(), self.v_all.clone()   # (rows prefix .. N-1 are what the appends write again)
        self.q, self.k, self.v = (t[:, prefix:].contiguous() for t in (self.q_all, self.k_all, self.v_all))
        self.len_all = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.ws_extend = device_ops.extend_workspace(self.q, self.kc)
        self.slices = []
        for a in range(0, T, STEP):
            e = min(a + STEP, T)
            qs, ks, vs = (t[:, a:e].contiguous() for t in (self.q, self.k, self.v))
            lens = torch.full((B,), prefix + e, dtype=torch.int32, device="cuda")
            self.slices.append((qs, ks, vs, lens, device_ops.decode_workspace(qs, self.kc)))

    def extend(self):
        return device_ops.flash_attn_extend(self.q, self.kc, self.vc, self.len_all, causal=True, workspace=self.ws_extend, k_new=self.k,
                                            v_new=self.v)[0]

    def loop(self):
        return [device_ops.flash_attn_decode(qs, self.kc, self.vc, lens, causal=True, workspace=ws, k_new=ks, v_new=vs)[0]
                for qs, ks, vs, lens, ws in self.slices]

    def square(self):
        return device_ops.flash_attn_fwd_gqa(self.q_all, self.k_all, self.v_all, True, _lib.FA_VARIANT_FA2)[0]

    def max_diff(self):
        """max-abs difference of the three paths' outputs for the new tokens (they compute one function)."""
        e = self.extend()
        lp = torch.cat(self.loop(), dim=1)
        sq = self.square()[:, self.prefix:]
        torch.cuda.synchronize()
        return {"extend_vs_loop": float((e - lp).abs().max()), "extend_vs_square": float((e - sq).abs().max())}


def measure(case, paths, args):
    row = {"Hkv": case.hkv, "G": H // case.hkv, "prefix": case.prefix, "T": case.T,
           "extend_splits": _lib.decode().fa_mi355x_extend_splits(B, H, case.hkv, case.T, case.N, D, 1), "max_abs_diff": case.max_diff()}
    for name in paths:
        row[name] = spread(getattr(case, name), args.reps, args.warmup, args.repeats)
    for name in paths[1:]:
        row[f"{name}_over_extend"] = round(row[name]["median_ms"] / row["extend"]["median_ms"], 3)
    if "loop" in row:   # is the difference to the loop beyond the loop's own window-to-window spread?
        row["loop_spread_ms"] = round(row["loop"]["max_ms"] - row["loop"]["min_ms"], 4)
        row["extend_faster_than_loop_beyond_spread"] = row["loop"]["median_ms"] - row["extend"]["median_ms"] > row["loop_spread_ms"]
    return row


def trace_workload(hkv, prefix, T, reps):
    """``reps`` calls of the extend path and of the decode loop on one shape and nothing else: the program of a kernel trace."""
    case = Case(hkv, prefix, T)
    for _ in range(reps):
        case.extend()
        case.loop()
    torch.cuda.synchronize()


FAMILIES = ("extend_split_kernel", "decode_split_kernel", "decode_combine_kernel", "decode_append_kernel")


def kernel_stats(path):
    import csv
    rows = {}
    for r in csv.DictReader(open(path)):
        for fam in FAMILIES:
            if fam in r["Name"]:
                e = rows.setdefault(fam, {"calls": 0, "total_us": 0.0, "min_us": None})
                e["calls"] += int(r["Calls"])
                e["total_us"] += float(r["AverageNs"]) * int(r["Calls"]) / 1e3
                mn = float(r["MinNs"]) / 1e3
                e["min_us"] = mn if e["min_us"] is None else min(e["min_us"], mn)
                break
    for e in rows.values():
        e["avg_us"] = round(e["total_us"] / e["calls"], 2)
        e["total_us"], e["min_us"] = round(e["total_us"], 1), round(e["min_us"], 2)
    return {"kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--section", choices=("prefix", "empty", "crossover", "all"), default="all")
    ap.add_argument("--hkv", type=int, nargs="+", default=list(HKVS), help="kv head counts to measure")
    ap.add_argument("--prefix", type=int, nargs="+", default=list(PREFIXES), help="prefix lengths of the prefix section")
    ap.add_argument("--t", type=int, nargs="+", default=None, help="new-token counts (default: each section's own list)")
    ap.add_argument("--trace-workload", metavar="HKV,PREFIX,T", help="run only extend + loop calls of this shape (for a kernel trace)")
    ap.add_argument("--kernel-stats", metavar="CSV", help="summarise the kernel_stats.csv of a trace of --trace-workload")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats)))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_extend.py measures on the GPU; there is none here")
    if args.trace_workload:
        trace_workload(*(int(x) for x in args.trace_workload.split(",")), args.reps)
        return
    print(json.dumps({"device": torch.cuda.get_device_name(0), "B": B, "H": H, "d": D, "dtype": "bf16", "layout": "bnhd", "causal": True,
                      "reps": args.reps, "repeats": args.repeats}), flush=True)
    if args.section in ("prefix", "all"):
        for hkv in args.hkv:
            for prefix in args.prefix:
                for T in args.t or TS:
                    print(json.dumps(dict(section="prefix", **measure(Case(hkv, prefix, T), ("extend", "loop", "square"), args))), flush=True)
    if args.section in ("empty", "all"):
        for hkv in args.hkv:
            for T in args.t or TS:
                print(json.dumps(dict(section="empty", **measure(Case(hkv, 0, T), ("extend", "square"), args))), flush=True)
    if args.section in ("crossover", "all"):
        for hkv in args.hkv:
            for T in args.t or CROSSOVER_TS:
                print(json.dumps(dict(section="crossover", **measure(Case(hkv, 4096, T), ("extend", "loop"), args))), flush=True)


if __name__ == "__main__":
    main()
