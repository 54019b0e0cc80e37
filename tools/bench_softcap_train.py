"""Logit soft-capping in the training call on the MI355X: the capped call over the uncapped one, one JSON line per (N, W).

Setup: bf16, d = 128, B = 2, H = 32, Hkv = 8, [B][N][H][d], softcap = 50.  Rows: W = 1024 at N = 4096 / 8192 / 16384, and no window
at N = 4096 (W = N).  Measured per row: the forward alone and forward + backward of flash_attn_gqa(causal=True, window=W,
softcap=50) (the cap builds of libflash_attn_mi355x_window.so) over the same call without the cap through the same library's
uncapped kernels (for W = N: those kernels at window = N, which flash_attn_gqa itself never picks).  The row without a window also
gives the capped call over flash_attn_gqa(causal=True), the core library's kernels: what the uncapped model runs.
All sides of one row run window by window in turn in one process, the median of ``--repeats`` windows is reported, and the baseline
is measured twice (``aa_*``: second over first, the noise the ratios are read against), as tools/bench_window_train.py does.
No ratio is a pass condition.

    python tools/bench_softcap_train.py [--repeats 5] [--window-ms 60] > profiles/softcap_train_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import device_ops  # noqa: E402
from bench_window_train import rnd, window_ms  # noqa: E402

D, B, H, HKV, CAP = 128, 2, 32, 8, 50.0
ROWS = ((4096, 1024), (8192, 1024), (16384, 1024), (4096, 0))   # (N, W); W = 0: no window


def sides_of(g, N, W):
    """name -> callable: the uncapped window kernels (twice) and the cap builds, forward and forward + backward; without a window
    also the core library's causal call."""
    q, do = (rnd(g, B, N, H, D) for _ in range(2))
    k, v = (rnd(g, B, N, HKV, D) for _ in range(2))
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    dof = do.float()
    Wc = W or N

    def attend(tq, tk, tv, cap):   # (the autograd path flash_attn_gqa routes a windowed or capped call to)
        return device_ops._window_fn(tq, tk, tv, None, "bnhd", Wc, 0, cap)

    def fwd(op):
        def call():
            with torch.no_grad():
                op(q, k, v)
        return call

    def fwd_bwd(op):
        def call():
            qg.grad = kg.grad = vg.grad = None
            op(qg, kg, vg).backward(dof)
        return call
    plain = lambda tq, tk, tv: attend(tq, tk, tv, None)
    capped = lambda tq, tk, tv: device_ops.flash_attn_gqa(tq, tk, tv, True, None, "bnhd", window=W or None, softcap=CAP)
    sides = {"plain_fwd": fwd(plain), "plain_fwd_bwd": fwd_bwd(plain), "cap_fwd": fwd(capped), "cap_fwd_bwd": fwd_bwd(capped)}
    if not W:
        core = lambda tq, tk, tv: device_ops.flash_attn_gqa(tq, tk, tv, True, None, "bnhd")
        sides["core_fwd"], sides["core_fwd_bwd"] = fwd(core), fwd_bwd(core)
    sides["plain_fwd_again"], sides["plain_fwd_bwd_again"] = sides["plain_fwd"], sides["plain_fwd_bwd"]
    return sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="least device time of one timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_softcap_train.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "B": B, "H": H, "Hkv": HKV,
                      "softcap": CAP, "repeats": args.repeats, "window_ms": args.window_ms}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    r3 = lambda x: round(x, 3)
    for N, W in ROWS:
        sides = sides_of(g, N, W)
        reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
        xs = {n: [] for n in sides}
        for _ in range(args.repeats):
            for n, c in sides.items():
                xs[n].append(window_ms(c, reps[n], 1))
        med = {n: statistics.median(v) for n, v in xs.items()}
        row = {"N": N, "W": W or "none", "plain_fwd_ms": r3(med["plain_fwd"]), "cap_fwd_ms": r3(med["cap_fwd"]),
               "plain_fwd_bwd_ms": r3(med["plain_fwd_bwd"]), "cap_fwd_bwd_ms": r3(med["cap_fwd_bwd"]),
               "cap_over_plain_fwd": r3(med["cap_fwd"] / med["plain_fwd"]), "aa_fwd": r3(med["plain_fwd_again"] / med["plain_fwd"]),
               "cap_over_plain_fwd_bwd": r3(med["cap_fwd_bwd"] / med["plain_fwd_bwd"]),
               "aa_fwd_bwd": r3(med["plain_fwd_bwd_again"] / med["plain_fwd_bwd"]),
               "min_max_cap_fwd_bwd_ms": [r3(min(xs["cap_fwd_bwd"])), r3(max(xs["cap_fwd_bwd"]))]}
        if not W:
            row.update({"core_fwd_ms": r3(med["core_fwd"]), "core_fwd_bwd_ms": r3(med["core_fwd_bwd"]),
                        "cap_over_core_fwd": r3(med["cap_fwd"] / med["core_fwd"]),
                        "cap_over_core_fwd_bwd": r3(med["cap_fwd_bwd"] / med["core_fwd_bwd"])})
        print(json.dumps(row), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
