"""The ragged-batch call against today's uniform calls on the MI355X: one JSON line per workload.

All sides are the fused calls (append + attention) on ONE paged cache (page_size 256, a randomly permuted table), d = 128,
H = 32, Hkv = 8, causal, in one process:
  mixed    31 sequences decode one token at length 4096 and one adds 512 tokens after an 8192-token prefix (B = 32, 543 packed rows).
           ragged: one flash_attn_ragged call.  (a) padded: flash_attn_extend with Nq = 512 for all 32 (16384 rows).  (b) two calls on
           sub-batches: flash_attn_decode on the 31 and flash_attn_extend on the one.
  uniform  B = 8, every count 512, after an 8192-token prefix: flash_attn_ragged against flash_attn_extend (the same tile loop; the
           difference is the schedule launch, the map reads and the policy's bound on the row blocks).
  decode   B = 32, every count 1, length 4096: flash_attn_ragged against flash_attn_decode, bf16 and fp32.
Per side: milliseconds per call from device events around a window of calls (at least ``--reps``, and enough to fill ``--window-ms``
of device time); ``--repeats`` windows per side after warm-up, the sides ALTERNATING window by window, median and min .. max
reported.  EVERY baseline is measured twice per round (an A/A repeat): next to each ``ragged_over_X`` stand ``aa_X``, the ratio of
that baseline's two series' medians, and ``spread_X``, its (max - min) / median: the noise the ratio is read against.
A kernel trace (the schedule kernel's own time) is a run of its own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python tools/bench_ragged.py --trace-workload uniform

    python tools/bench_ragged.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/ragged_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

D, H, HKV, PAGE = 128, 32, 8, 256
# name -> (counts, lengths counting the new tokens, dtype)
WORKLOADS = {
    "mixed": ([1] * 31 + [512], [4096] * 31 + [8192 + 512], torch.bfloat16),
    "uniform": ([512] * 8, [8192 + 512] * 8, torch.bfloat16),
    "decode": ([1] * 32, [4096] * 32, torch.bfloat16),
    "decode-f32": ([1] * 32, [4096] * 32, torch.float32),
}


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


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


class Case:
    """One workload: the pools and the table, the packed new tokens of the ragged call, and the same tokens in the shapes the
    uniform calls take."""

    def __init__(self, name, seed=0):
        self.name = name
        self.counts, lens, self.dtype = WORKLOADS[name]
        self.B, self.T, top = len(self.counts), sum(self.counts), max(self.counts)
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(self.dtype)
        mp = -(-max(l - c + top for l, c in zip(lens, self.counts)) // PAGE)   # (room for the padded call's lengths)
        ids = torch.randperm(self.B * mp, generator=torch.Generator().manual_seed(seed + 1))
        self.table = ids.view(self.B, mp).to(torch.int32).cuda()
        self.kp, self.vp = rnd(self.B * mp, PAGE, HKV, D), rnd(self.B * mp, PAGE, HKV, D)
        self.lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
        self.cu = torch.tensor([0] + torch.tensor(self.counts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
        self.q, self.kn, self.vn = rnd(self.T, H, D), rnd(self.T, HKV, D), rnd(self.T, HKV, D)
        self.ws = device_ops.ragged_workspace(self.q, self.kp, self.cu, block_table=self.table)
        self.ncap = mp * PAGE
        # the padded uniform call: every sequence brings `top` tokens (its own at the end)
        self.pq, self.pkn, self.pvn = rnd(self.B, top, H, D), rnd(self.B, top, HKV, D), rnd(self.B, top, HKV, D)
        self.plens = torch.tensor([l - c + top for l, c in zip(lens, self.counts)], dtype=torch.int32, device="cuda")
        self.uniform_fn = device_ops.flash_attn_decode if top == 1 else device_ops.flash_attn_extend
        new_ws = device_ops.decode_workspace if top == 1 else device_ops.extend_workspace
        self.pws = new_ws(self.pq, self.kp, block_table=self.table)
        if name == "mixed":   # the two sub-batches: the 31 that decode, the one that extends
            n = self.B - 1
            self.dq, self.dkn, self.dvn = rnd(n, 1, H, D), rnd(n, 1, HKV, D), rnd(n, 1, HKV, D)
            self.eq, self.ekn, self.evn = rnd(1, top, H, D), rnd(1, top, HKV, D), rnd(1, top, HKV, D)
            self.dtable, self.etable = self.table[:n].contiguous(), self.table[n:].contiguous()
            self.dlens, self.elens = self.lens[:n].contiguous(), self.lens[n:].contiguous()
            self.dws = device_ops.decode_workspace(self.dq, self.kp, block_table=self.dtable)
            self.ews = device_ops.extend_workspace(self.eq, self.kp, block_table=self.etable)

    def ragged(self):
        return device_ops.flash_attn_ragged(self.q, self.kp, self.vp, self.cu, self.lens, causal=True, workspace=self.ws, k_new=self.kn,
                                            v_new=self.vn, block_table=self.table)

    def uniform(self):   # (mixed: the padded call)
        return self.uniform_fn(self.pq, self.kp, self.vp, self.plens, causal=True, workspace=self.pws, k_new=self.pkn, v_new=self.pvn,
                               block_table=self.table)

    def two_calls(self):
        device_ops.flash_attn_decode(self.dq, self.kp, self.vp, self.dlens, causal=True, workspace=self.dws, k_new=self.dkn, v_new=self.dvn,
                                     block_table=self.dtable)
        return device_ops.flash_attn_extend(self.eq, self.kp, self.vp, self.elens, causal=True, workspace=self.ews, k_new=self.ekn,
                                            v_new=self.evn, block_table=self.etable)


def measure(case, args):
    sides = ["ragged", "uniform"] + (["two_calls"] if case.name == "mixed" else [])
    reps = max(args.reps, int(args.window_ms / window_ms(case.ragged, 5, args.warmup)) + 1)
    order = sides + ["aa:" + s for s in sides[1:]]
    xs = {s: [] for s in order}
    for i in range(args.repeats):   # the sides alternate, window by window; every baseline once more at the end of every round
        for side in order:
            xs[side].append(window_ms(getattr(case, side.split(":")[-1]), reps, args.warmup if i == 0 else 1))
    lib, code = _lib.decode(), 1 if case.dtype == torch.bfloat16 else 0
    row = {"workload": case.name, "dtype": str(case.dtype).split(".")[1], "B": case.B, "T": case.T, "Ncap": case.ncap,
           "ragged_splits": lib.fa_mi355x_ragged_splits(case.B, H, HKV, case.T, case.ncap, D, code), "calls_per_window": reps}
    for s in sides:
        row[s] = stats(xs[s])
    names = {"uniform": "padded_extend" if case.name == "mixed" else case.uniform_fn.__name__, "two_calls": "decode_plus_extend"}
    for s in sides[1:]:
        b = row[s]
        row["ragged_over_" + names[s]] = round(row["ragged"]["median_ms"] / b["median_ms"], 3)
        row["aa_" + names[s]] = round(statistics.median(xs["aa:" + s]) / b["median_ms"], 3)
        row["spread_" + names[s]] = round((b["max_ms"] - b["min_ms"]) / b["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--workload", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--trace-workload", choices=list(WORKLOADS), help="run only the ragged and the uniform call of this workload (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on the GPU; there is none here")
    if args.trace_workload:
        case = Case(args.trace_workload)
        for _ in range(args.reps):
            case.ragged()
            case.uniform()
        torch.cuda.synchronize()
        return
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "H": H, "Hkv": HKV, "page_size": PAGE, "layout": "bnhd", "causal": True,
                      "fused_append": True, "reps": args.reps, "repeats": args.repeats}), flush=True)
    for name in args.workload:
        print(json.dumps(measure(Case(name), args)), flush=True)


if __name__ == "__main__":
    main()
