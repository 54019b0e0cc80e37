"""A paged KV cache against the contiguous one on the MI355X: one JSON line per (shape, page_size, table).

Both sides run the same call on the same cache contents in one process: the contiguous call on a slab per sequence, the paged call
(block_table=) on a pool of pages.  The contiguous kernels are the yardstick (the PAGED = false builds, unchanged); the paged call
reads the same bytes plus one table entry per 128-key tile, and at G = 1 it runs the grouped build of the decode kernel.
Shapes (bf16, d = 128, [B][N][H][d], causal):
  decode   Nq = 1, B = 32, H = 32, Hkv = 8 and 32, 4096 cached tokens; and B = 1, H = Hkv = 8, 65536 cached tokens
  extend   T = 512 new tokens after a prefix of 8192, B = 8, H = 32, Hkv = 8 (the fused append + attention, as tools/bench_extend.py)
each with page_size 128 and 256, and with the identity table (sequence b owns pages b * max_pages ...) and a randomly permuted one.
Per side: milliseconds per call, device events around a window of calls (at least ``--reps``, and enough of them to fill
``--window-ms`` of device time: a 20 us call is not timed over a handful of launches); ``--repeats`` windows per side, ALTERNATING
the two sides, median and min .. max reported.  ``paged_over_contiguous`` is the ratio of the medians; ``contiguous_spread`` the contiguous side's
(max - min) / median, the noise the ratio is read against.  ``bitwise_equal``: the two sides' out and lse are the same bits.
A kernel trace is a run of its own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python tools/bench_paged.py --trace-workload NAME,PAGE_SIZE

    python tools/bench_paged.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/paged_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

D = 128
# name -> (extend, B, H, Hkv, prefix, T)
SHAPES = {
    "decode-B32-H32-Hkv8-len4096": (False, 32, 32, 8, 4095, 1),
    "decode-B32-H32-Hkv32-len4096": (False, 32, 32, 32, 4095, 1),
    "decode-B1-H8-Hkv8-len65536": (False, 1, 8, 8, 65535, 1),
    "extend-B8-H32-Hkv8-prefix8192-T512": (True, 8, 32, 8, 8192, 512),
}
PAGE_SIZES = (128, 256)


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
    """One shape: the slabs (B, N, Hkv, D) with N = prefix + T, the T new tokens' q (and k, v for the extend shapes), and per
    (page_size, table) the pools that hold the same rows."""

    def __init__(self, name, seed=0):
        self.name = name
        self.extend, self.B, self.H, self.Hkv, self.prefix, self.T = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.N = self.prefix + self.T
        self.kc, self.vc = rnd(self.B, self.N, self.Hkv, D), rnd(self.B, self.N, self.Hkv, D)
        self.q = rnd(self.B, self.T, self.H, D)
        self.new = dict(k_new=self.kc[:, self.prefix:].contiguous(), v_new=self.vc[:, self.prefix:].contiguous()) if self.extend else {}
        self.lens = torch.full((self.B,), self.N, dtype=torch.int32, device="cuda")
        self.fn = device_ops.flash_attn_extend if self.extend else device_ops.flash_attn_decode
        self.new_ws = device_ops.extend_workspace if self.extend else device_ops.decode_workspace
        self.ws = self.new_ws(self.q, self.kc)

    def contiguous(self):
        return self.fn(self.q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, **self.new)

    def paginate(self, page_size, permuted, seed=1):
        assert self.N % page_size == 0
        mp = self.N // page_size
        ids = torch.arange(self.B * mp)
        if permuted:
            ids = ids[torch.randperm(self.B * mp, generator=torch.Generator().manual_seed(seed))]
        self.table = ids.view(self.B, mp).to(torch.int32).cuda()
        self.kp, self.vp = (torch.empty((self.B * mp, page_size, self.Hkv, D), dtype=torch.bfloat16, device="cuda") for _ in range(2))
        for pool, slab in ((self.kp, self.kc), (self.vp, self.vc)):
            pool[self.table.long().view(-1)] = slab.view(self.B * mp, page_size, self.Hkv, D)
        self.ws_paged = self.new_ws(self.q, self.kp, block_table=self.table)

    def paged(self):
        return self.fn(self.q, self.kp, self.vp, self.lens, causal=True, workspace=self.ws_paged, block_table=self.table, **self.new)


def measure(case, page_size, permuted, args):
    case.paginate(page_size, permuted)
    a, b = case.contiguous(), case.paged()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    reps = max(args.reps, int(args.window_ms / window_ms(case.contiguous, 5, args.warmup)) + 1)
    xs = {"contiguous": [], "paged": []}
    for i in range(args.repeats):   # the two sides alternate, window by window
        for side in ("contiguous", "paged"):
            xs[side].append(window_ms(getattr(case, side), reps, args.warmup if i == 0 else 1))
    splits = _lib.decode().fa_mi355x_extend_splits if case.extend else _lib.decode().fa_mi355x_decode_splits_gqa
    row = {"shape": case.name, "page_size": page_size, "table": "permuted" if permuted else "identity",
           "splits": splits(case.B, case.H, case.Hkv, case.T, case.N, D, 1), "calls_per_window": reps, "bitwise_equal": same,
           "contiguous": stats(xs["contiguous"]), "paged": stats(xs["paged"])}
    c = row["contiguous"]
    row["paged_over_contiguous"] = round(row["paged"]["median_ms"] / c["median_ms"], 3)
    row["contiguous_spread"] = round((c["max_ms"] - c["min_ms"]) / c["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--shape", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--trace-workload", metavar="NAME,PAGE_SIZE", help="run only contiguous + paged calls of this shape (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged.py measures on the GPU; there is none here")
    if args.trace_workload:
        name, ps = args.trace_workload.split(",")
        case = Case(name)
        case.paginate(int(ps), True)
        for _ in range(args.reps):
            case.contiguous()
            case.paged()
        torch.cuda.synchronize()
        return
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "causal": True,
                      "reps": args.reps, "repeats": args.repeats}), flush=True)
    for name in args.shape:
        case = Case(name)
        for ps in PAGE_SIZES:
            for permuted in (False, True):
                print(json.dumps(measure(case, ps, permuted, args)), flush=True)


if __name__ == "__main__":
    main()
