"""Logit soft-capping against the same call without it on the MI355X: one JSON line per (shape, slab or paged).

Both sides run the same call on the same caches in one process: the uncapped call (the yardstick: the builds that were there,
unchanged) and the call with ``softcap=`` (the SOFTCAP builds of the split kernels, which spend one v_exp_f32 and one v_rcp_f32 more
per score, and the existing combine kernel).  The uncapped side is measured twice, interleaved with the capped side (A, capped, A'),
so every row carries its own A/A figure: ``aa`` is median(A') / median(A) and ``plain_spread`` the (max - min) / median over both.
Shapes (bf16, d = 128, [B][N][H][d], B = 32, H = 32, Hkv = 8, causal; the shapes of tools/bench_window.py):
  decode   Nq = 1 at 4096 cached tokens, on slabs and on a pool of 128-row pages under a randomly permuted table
  extend   512 new tokens (fused append) after a prefix of 8192, on slabs
There is no pass mark.  The expectation: the one-token step is bound by HBM, so its ratio should sit inside the A/A spread; the
512-token call does two transcendentals more for each of its B * H * 512 * ~8450 scores and will show it.
Per side: milliseconds per call, device events around a window of calls (at least ``--reps``, and enough of them to fill
``--window-ms`` of device time); ``--repeats`` windows per side, median and min .. max reported.

    python tools/bench_softcap.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/softcap_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

D, PAGE, B, H, HKV = 128, 128, 32, 32, 8
SOFTCAP = 50.0   # Gemma-2's attn_logit_softcapping
# name -> (extend, prefix, T, paged)
SHAPES = {
    "decode-len4096-slab": (False, 4095, 1, False),
    "decode-len4096-paged": (False, 4095, 1, True),
    "extend-prefix8192-T512-slab": (True, 8192, 512, False),
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
    """One shape: bf16 caches (B, N, Hkv, D) with N = prefix + T (or the pool that holds them), the T new tokens' q, and their k, v
    for the fused extend call."""

    def __init__(self, extend, prefix, T, paged, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.T, self.N, self.extend = T, prefix + T, extend
        kc, vc = rnd(B, self.N, HKV, D), rnd(B, self.N, HKV, D)
        self.q = rnd(B, T, H, D)
        self.new = dict(k_new=kc[:, prefix:].contiguous(), v_new=vc[:, prefix:].contiguous()) if extend else {}
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.where = {}
        if paged:
            mp = self.N // PAGE
            assert mp * PAGE == self.N
            table = torch.randperm(B * mp, generator=torch.Generator().manual_seed(1)).view(B, mp).to(torch.int32).cuda()
            pools = []
            for t in (kc, vc):
                pool = torch.empty((B * mp, PAGE, HKV, D), dtype=t.dtype, device="cuda")
                pool[table.long().view(-1)] = t.reshape(B * mp, PAGE, HKV, D)
                pools.append(pool)
            kc, vc = pools
            self.where = dict(block_table=table)
        self.caches = (kc, vc)
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        self.ws = (device_ops.extend_workspace if extend else device_ops.decode_workspace)(self.q, kc, **self.where)

    def plain(self):
        return self.fn(self.q, *self.caches, self.lens, causal=True, workspace=self.ws, **self.new, **self.where)

    def capped(self):
        return self.fn(self.q, *self.caches, self.lens, causal=True, workspace=self.ws, softcap=SOFTCAP, **self.new, **self.where)


def measure(name, case, args):
    a, b = case.plain, case.capped
    a(), b()
    torch.cuda.synchronize()
    reps = max(args.reps, int(args.window_ms / window_ms(a, 5, args.warmup)) + 1)
    xs = {"plain": [], "softcap": [], "plain_again": []}
    for i in range(args.repeats):   # A, capped, A': window by window
        for side, fn in (("plain", a), ("softcap", b), ("plain_again", a)):
            xs[side].append(window_ms(fn, reps, args.warmup if i == 0 else 1))
    row = {"shape": name, "calls_per_window": reps}
    row.update({s: stats(x) for s, x in xs.items()})
    base = row["plain"]["median_ms"]
    both = xs["plain"] + xs["plain_again"]
    row["aa"] = round(row["plain_again"]["median_ms"] / base, 3)
    row["plain_spread"] = round((max(both) - min(both)) / statistics.median(both), 3)
    row["softcap_over_plain"] = round(row["softcap"]["median_ms"] / base, 3)
    row["plain_tbps"] = round(2 * B * HKV * case.N * D * 2 / base / 1e9, 2)   # the K and V cache bytes the call reads
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--shape", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_softcap.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "B": B, "H": H, "Hkv": HKV, "layout": "bnhd",
                      "causal": True, "page_size": PAGE, "softcap": SOFTCAP, "reps": args.reps, "repeats": args.repeats}), flush=True)
    for name in args.shape:
        extend, prefix, T, paged = SHAPES[name]
        case = Case(extend, prefix, T, paged)
        row = measure(name, case, args)
        splits = _lib.decode().fa_mi355x_extend_splits if extend else _lib.decode().fa_mi355x_decode_splits_gqa
        row["splits"] = splits(B, H, HKV, T, case.N, D, 1)
        print(json.dumps(row), flush=True)
        del case
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
