"""Grouped-query (GQA / MQA) heads in the training / prefill path on the MI355X: one JSON line per (Hkv, causal) shape.

Shapes: bf16, d = 64, [B][N][H][d], B = 8, H = 32, N = 4096, Hkv in {32, 8, 1}, causal and not.  Two paths on the same data:
  grouped    device_ops.flash_attn_gqa on the (B, N, Hkv, d) k and v: the kernels read the Hkv heads in place, the backward stores a
             dK / dV per query head into its workspace and group_sum_kernel adds each group's heads
  expanded   what a grouped model did before: k and v expanded to H heads (one copy each), the ungrouped operator
             (_FlashAttnFn on [B][N][H][d]), autograd's sum over the group in the backward of the expansion
Per path: milliseconds of the forward and of forward + backward (device events around ``--reps`` calls after ``--warmup``; ``--repeats``
such windows, median and min .. max reported), and torch.cuda.max_memory_allocated of ONE forward + backward above what the inputs
hold, and the copy rate of this box measured in the same process (a 512 MiB tensor copy: read + write).
The group-sum launch by itself comes from a kernel trace, a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python tools/bench_gqa.py --trace-workload 8
    python tools/bench_gqa.py --kernel-stats DIR/.../t_kernel_stats.csv --hkv 8 --copy-tbs <the main run's copy rate>
prints its time, the bytes it must move (2*B*H*N*d floats read, 2*B*Hkv*N*d written) over that time beside the copy rate, and its
share of the backward's kernel time.
Hkv = H runs the grouped entry points with no group: the ungrouped kernels, no scratch, no group sum.
The two paths do not run the same builds at this shape: the expanded path is an ungrouped call of B*H = 256 heads, whose dQ and dK/dV
stages take the tiled slot builds (several heads per workgroup); a grouped call takes the same kernels' one-head-per-workgroup builds
("Grouped-query heads": exclusions).  The comparison is between what a user gets either way.

    python tools/bench_gqa.py [--reps 20] [--warmup 5] [--repeats 5] > profiles/gqa_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops, modules_transformer as mt  # noqa: E402

B, H, N, D = 8, 32, 4096, 64
HKVS = (32, 8, 1)


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


def copy_rate_tbs(repeats):
    """read + write bytes per second of a device-to-device copy of 512 MiB (larger than the 256 MiB Infinity Cache)."""
    src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ms = min(window_ms(lambda: dst.copy_(src), 10, 3) for _ in range(repeats))
    return 2 * src.numel() / (ms * 1e-3) / 1e12


def expanded_attention(q, k, v, causal):
    # (.contiguous(): with Hkv = 1, _expand_kv's reshape of (B, N, 1, G, d) to (B, N, G, d) merges no dimensions and stays a stride-0 view,
    # which the ungrouped operator rejects; for Hkv > 1 the reshape has already copied and this is a no-op)
    ke, ve = mt._expand_kv(k, H).contiguous(), mt._expand_kv(v, H).contiguous()
    return device_ops._FlashAttnFn.apply(q, ke, ve, causal, _lib.FA_VARIANT_FA2, _lib.FA_LAYOUT_BNHD, None)


def grouped_attention(q, k, v, causal):
    return device_ops.flash_attn_gqa(q, k, v, causal=causal, layout="bnhd")


def peak_extra_bytes(attn, q, k, v, do, causal):
    for t in (q, k, v):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    attn(q, k, v, causal).backward(do)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    for t in (q, k, v):
        t.grad = None
    return peak


def trace_workload(hkv, causal, reps):
    """``reps`` grouped forward + backward calls of one shape and nothing else: the program of a kernel trace
    (rocprofv3 --kernel-trace --stats -f csv -- python tools/bench_gqa.py --trace-workload HKV), which times every kernel by itself."""
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
    q, k, v = rnd(B, N, H, D).requires_grad_(), rnd(B, N, hkv, D).requires_grad_(), rnd(B, N, hkv, D).requires_grad_()
    do = rnd(B, N, H, D).float()
    for _ in range(reps):
        grouped_attention(q, k, v, causal).backward(do)
        q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()


def kernel_stats(path, hkv, copy_tbs):
    """The group-sum launch by itself, from the *kernel_stats.csv of a trace of trace_workload(hkv): its time (the fastest call: the
    average includes the first, cold launches), the bytes it must move over that time, and its share of the backward's kernels."""
    import csv
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].split("(")[0]
        for fam in ("group_sum_kernel", "bwd_dkdv_slot_kernel", "bwd_dkdv_kernel", "bwd_dq_slot_kernel", "bwd_dq_kernel", "bwd_prep_kernel",
                    "fwd_slot_kernel", "fwd_kernel"):
            if fam in name:
                e = rows.setdefault(fam, {"calls": 0, "min_us": 0.0, "avg_us": 0.0})
                e["calls"] += int(r["Calls"])
                e["min_us"] += float(r["MinNs"]) / 1e3      # (a family's builds run once per call each: their times add up)
                e["avg_us"] += float(r["AverageNs"]) / 1e3
                break
    gs = rows["group_sum_kernel"]["min_us"]
    bwd = sum(e["min_us"] for fam, e in rows.items() if fam.startswith(("bwd_", "group_sum")))
    nbytes = 2 * B * (H + hkv) * N * D * 4
    tbs = nbytes / (gs * 1e-6) / 1e12
    return {"Hkv": hkv, "kernels_us": {f: {k: round(x, 2) if k != "calls" else x for k, x in e.items()} for f, e in rows.items()},
            "group_sum_us": round(gs, 2), "group_sum_bytes": nbytes, "group_sum_TBps": round(tbs, 3),
            "share_of_copy_rate": round(tbs / copy_tbs, 3) if copy_tbs else None, "share_of_backward_kernels": round(gs / bwd, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-workload", type=int, metavar="HKV", default=0, help="run only grouped fwd + bwd calls at this Hkv (for a kernel trace)")
    ap.add_argument("--causal", action="store_true", help="with --trace-workload")
    ap.add_argument("--kernel-stats", metavar="CSV", help="summarise the kernel_stats.csv of a trace of --trace-workload HKV (needs --hkv)")
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--copy-tbs", type=float, default=0.0, help="with --kernel-stats: the copy rate the main run measured")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats, args.hkv, args.copy_tbs)))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_gqa.py measures on the GPU; there is none here")
    if args.trace_workload:
        trace_workload(args.trace_workload, args.causal, args.reps)
        return
    copy_tbs = copy_rate_tbs(args.repeats)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.core().fa_mi355x_version().decode(),
                      "copy_rate_TBps_read_plus_write": round(copy_tbs, 3), "B": B, "H": H, "N": N, "d": D, "dtype": "bf16",
                      "layout": "bnhd", "reps": args.reps, "repeats": args.repeats}))
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
    for causal in (False, True):
        for hkv in HKVS:
            q, k, v = rnd(B, N, H, D).requires_grad_(), rnd(B, N, hkv, D).requires_grad_(), rnd(B, N, hkv, D).requires_grad_()
            do = rnd(B, N, H, D).float()
            row = {"Hkv": hkv, "G": H // hkv, "causal": causal}
            for name, attn in (("grouped", grouped_attention), ("expanded", expanded_attention)):
                def fwd():
                    with torch.no_grad():
                        attn(q, k, v, causal)

                def fwd_bwd():
                    attn(q, k, v, causal).backward(do)
                    q.grad = k.grad = v.grad = None
                row[name] = {"fwd": spread(fwd, args.reps, args.warmup, args.repeats),
                             "fwd_bwd": spread(fwd_bwd, args.reps, args.warmup, args.repeats),
                             "peak_extra_MiB": round(peak_extra_bytes(attn, q, k, v, do, causal) / 2 ** 20, 1)}
            row["fwd_speedup"] = round(row["expanded"]["fwd"]["median_ms"] / row["grouped"]["fwd"]["median_ms"], 3)
            row["fwd_bwd_speedup"] = round(row["expanded"]["fwd_bwd"]["median_ms"] / row["grouped"]["fwd_bwd"]["median_ms"], 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
