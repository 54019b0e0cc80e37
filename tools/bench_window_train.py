"""The sliding-window training call against the causal one on the MI355X: one JSON line per (N, W, S).

Setup: bf16, d = 128, H = 32, Hkv = 8, [B][N][H][d], B = 2.  Grid: N in {4096, 8192, 16384, 32768} x W in {1024, 4096} x S in {0, 4}.
Measured per row: the forward alone and forward + backward of flash_attn_gqa(causal=True, window=W, sink=S) (the kernels of
libflash_attn_mi355x_window.so), and for the forward also flash_attn_extend(window=W, sink=S) with all N tokens as queries
against a cache that holds exactly their keys (the cache kernels under the same mask).  Baseline: flash_attn_gqa(causal=True) in
the same process.  The conventions are those of tools/bench_window.py: all sides of one N run window by window in turn, the
median of ``--repeats`` windows is reported, and every baseline is measured twice (``*_again``): its A/A ratio is the noise the
ratios are read against.  ``pairs`` is the number of admitted (query, key) pairs, windowed over causal: the share of the work
the mask leaves, to read the time ratios against.
The last line checks the one condition the design fixes in advance: at W = 1024, forward + backward from N = 8192 to N = 16384
grows by a factor below 3 (linear work gives 2, the causal call 4); the exit status is 1 when it does not.

    python tools/bench_window_train.py [--repeats 5] [--window-ms 60] > profiles/window_train_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import device_ops  # noqa: E402

D, B, H, HKV = 128, 2, 32, 8
NS, WS, SS = (4096, 8192, 16384, 32768), (1024, 4096), (0, 4)


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


def rnd(g, *shape):
    return torch.rand(shape, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)


def pairs(N, W, S):
    """Admitted (query, key) pairs: row i admits j <= i with j > i - W or j < S."""
    i = torch.arange(N, dtype=torch.int64)
    return int((torch.clamp(i + 1, max=W) + torch.clamp(torch.clamp(i - W + 1, min=0), max=S)).sum())


def sides_of(g, N):
    """name -> callable for one N: the causal baselines (twice each) and the three windowed calls of every (W, S)."""
    q, do = (rnd(g, B, N, H, D) for _ in range(2))
    k, v = (rnd(g, B, N, HKV, D) for _ in range(2))
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    dof = do.float()
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")

    def fwd(**kw):
        def call():
            with torch.no_grad():
                device_ops.flash_attn_gqa(q, k, v, True, None, "bnhd", **kw)
        return call

    def fwd_bwd(**kw):
        def call():
            qg.grad = kg.grad = vg.grad = None
            device_ops.flash_attn_gqa(qg, kg, vg, True, None, "bnhd", **kw).backward(dof)
        return call
    sides = {"causal_fwd": fwd(), "causal_fwd_bwd": fwd_bwd()}
    for W in WS:
        for S in SS:
            if W >= N:
                continue
            ws = device_ops.extend_workspace(q, k, window=W, sink=S or None)
            sides[f"fwd W{W} S{S}"] = fwd(window=W, sink=S)
            sides[f"fwd_bwd W{W} S{S}"] = fwd_bwd(window=W, sink=S)
            sides[f"extend W{W} S{S}"] = (lambda W=W, S=S, ws=ws: device_ops.flash_attn_extend(q, k, v, lens, causal=True, workspace=ws,
                                                                                              window=W, sink=S or None))
    sides["causal_fwd_again"], sides["causal_fwd_bwd_again"] = sides["causal_fwd"], sides["causal_fwd_bwd"]
    return sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="least device time of one timed window")
    ap.add_argument("--n", type=int, nargs="*", default=list(NS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_train.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "B": B, "H": H, "Hkv": HKV,
                      "repeats": args.repeats, "window_ms": args.window_ms}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    fb = {}
    for N in args.n:
        sides = sides_of(g, N)
        reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
        xs = {n: [] for n in sides}
        for _ in range(args.repeats):
            for n, c in sides.items():
                xs[n].append(window_ms(c, reps[n], 1))
        med = {n: statistics.median(v) for n, v in xs.items()}
        r3 = lambda x: round(x, 3)
        base = {"N": N, "causal_fwd_ms": r3(med["causal_fwd"]), "causal_fwd_bwd_ms": r3(med["causal_fwd_bwd"]),
                "aa_fwd": r3(med["causal_fwd_again"] / med["causal_fwd"]), "aa_fwd_bwd": r3(med["causal_fwd_bwd_again"] / med["causal_fwd_bwd"])}
        for W in WS:
            for S in SS:
                if f"fwd W{W} S{S}" not in med:
                    continue
                f, t, e = med[f"fwd W{W} S{S}"], med[f"fwd_bwd W{W} S{S}"], med[f"extend W{W} S{S}"]
                fb[(N, W, S)] = t
                print(json.dumps({**base, "W": W, "S": S, "pairs": r3(pairs(N, W, S) / pairs(N, N, 0)), "fwd_ms": r3(f), "fwd_bwd_ms": r3(t),
                                  "extend_fwd_ms": r3(e), "fwd_over_causal": r3(f / med["causal_fwd"]),
                                  "fwd_bwd_over_causal": r3(t / med["causal_fwd_bwd"]), "fwd_over_extend": r3(f / e),
                                  "min_max_fwd_bwd_ms": [r3(min(xs[f"fwd_bwd W{W} S{S}"])), r3(max(xs[f"fwd_bwd W{W} S{S}"]))]}), flush=True)
        del sides
        torch.cuda.empty_cache()
    ok = True
    for S in SS:
        if (8192, 1024, S) in fb and (16384, 1024, S) in fb:
            growth = fb[(16384, 1024, S)] / fb[(8192, 1024, S)]
            ok = ok and growth < 3
            print(json.dumps({"check": "fwd_bwd time at W = 1024, N = 16384 over N = 8192", "S": S, "growth": round(growth, 3), "required": "< 3"}),
                  flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
