"""The two-sided sliding-window packed call against the bidirectional packed call on the same tensors, on the MI355X: one JSON line
per (head configuration, length mix), one per head configuration for the growth with the sequence length, one for the encoder stack.

Setup: bf16, one cu_seqlens for queries and keys (encoder self-attention), packed q (T, H, d) and k, v (T, Hkv, d), at
  d = 64, H = Hkv = 12      an encoder of the BERT-base shape
  d = 128, H = 32, Hkv = 8  the project's grouped-query shape
Measured per mix, forward alone (``fwd``) and forward + backward (``fwd_bwd``):
  local 64    flash_attn_varlen_local(q, k, v, cu_seqlens, window=(64, 64))
  local 512   the same with window=(512, 512)
  bidir       flash_attn_varlen_bidir(q, k, v, cu_seqlens): what such a layer costs without the band, every pair of a sequence
Mixes: uniform 8 x 1024, 8 x 4096 and 2 x 16384; long-tailed, one sequence of 16384 and seven of 512 .. 2048.
``pairs``: the share of the bidirectional call's (query, key) pairs that the band leaves.  ``growth``: the time at 2 x 16384 over the
time at 8 x 4096, the same 32768 tokens in sequences four times as long: 1 for work that is linear in the length, 4 for quadratic.
The stack: modules_transformer.encoder_stack_packed with 4 layers, E = 768, 12 heads, on the 8 x 4096 mix, windows alternating
(64, 64) and None against all None, forward + backward.

The conventions are those of tools/bench_bidir.py (its helpers are used): all sides of one mix run window by window in turn, the
median of ``--repeats`` windows is reported, and the baseline is measured twice (``bidir again``): its A/A ratio (``aa``) is the
noise the ratios are read against.  A ratio above 1: the local call is faster.

    python tools/bench_local.py [--repeats 5] [--window-ms 40] > profiles/local_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_bidir import both, cu_of, leaf, rnd, window_ms  # noqa: E402
from flash_attention_minitorch_amd import device_ops  # noqa: E402
from flash_attention_minitorch_amd import modules_transformer as mt  # noqa: E402

CONFIGS = [(64, 12, 12), (128, 32, 8)]   # (d, H, Hkv)
WINDOWS = [(64, 64), (512, 512)]
MIXES = {
    "uniform 8 x 1024": [1024] * 8,
    "uniform 8 x 4096": [4096] * 8,
    "uniform 2 x 16384": [16384] * 2,
    "long tail 16384 + 7 of 512..2048": [16384, 512, 768, 1024, 1280, 1536, 1792, 2048],
}


def band_pairs(n, left, right):
    """(query, key) pairs of a sequence of n tokens under the band: row i admits the keys max(0, i - left) .. min(n - 1, i + right)."""
    return sum(min(n - 1, i + right) - max(0, i - left) + 1 for i in range(n))


def sides_of(g, lens, d, H, Hkv):
    T = sum(lens)
    q, do = (rnd(g, T, H, d) for _ in range(2))
    k, v = (rnd(g, T, Hkv, d) for _ in range(2))
    dof = do.float()
    _, cu = cu_of(lens)
    sides = {}
    for w in WINDOWS:
        def local(grad, w=w):
            qq, kk, vv = (leaf(t, grad) for t in (q, k, v))
            return (lambda: [(device_ops.flash_attn_varlen_local(qq, kk, vv, cu, None, w), dof)]), [qq, kk, vv]
        sides.update(both(f"local {w[0]}", local))

    def bidir(grad):
        qq, kk, vv = (leaf(t, grad) for t in (q, k, v))
        return (lambda: [(device_ops.flash_attn_varlen_bidir(qq, kk, vv, cu), dof)]), [qq, kk, vv]
    sides.update(both("bidir", bidir))
    for n in [n for n in sides if n.startswith("bidir")]:
        sides[n + " again"] = sides[n]
    return sides


def measure(sides, args):
    """name -> (median, min, max) ms over ``--repeats`` windows, the sides taking turns."""
    reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
    xs = {n: [] for n in sides}
    for _ in range(args.repeats):
        for n, c in sides.items():
            xs[n].append(window_ms(c, reps[n], 1))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in xs.items()}


def stack_sides(g, lens):
    E, heads, layers_n = 768, 12, 4
    T = sum(lens)
    x = rnd(g, T, E)
    dy = rnd(g, T, E)
    layers = [tuple(rnd(g, E, E) / 28 for _ in range(4)) for _ in range(layers_n)]
    _, cu = cu_of(lens)
    windows = [(64, 64), None] * (layers_n // 2)

    def side(window):
        def run():
            xg = x.clone().requires_grad_()
            mt.encoder_stack_packed(xg, cu, layers, heads, window=window).backward(dy)
        return run
    return {"alternating": side(windows), "global": side(None), "global again": side(None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0, help="least device time of one timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "dtype": "bf16", "repeats": args.repeats, "window_ms": args.window_ms,
                      "ratios": "bidir time over local time: above 1, the local call is faster"}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    r3 = lambda x: round(x, 3)
    for d, H, Hkv in CONFIGS:
        kept = {}
        for name, lens in MIXES.items():
            sides = sides_of(g, lens, d, H, Hkv)
            med = measure(sides, args)
            row = {"d": d, "H": H, "Hkv": Hkv, "mix": name, "T": sum(lens), "nseq": len(lens)}
            full = sum(n * n for n in lens)
            for kind in ("fwd", "fwd_bwd"):
                b, again = med[f"bidir {kind}"][0], med[f"bidir {kind} again"][0]
                row[f"bidir {kind}"] = {"ms": r3(b), "aa": r3(again / b)}
                for w in WINDOWS:
                    m, lo, hi = med[f"local {w[0]} {kind}"]
                    row[f"local {w[0]} {kind}"] = {"ms": r3(m), "min_max_ms": [r3(lo), r3(hi)],
                                                  "pairs": round(sum(band_pairs(n, *w) for n in lens) / full, 4), "bidir_over_local": r3(b / m)}
            kept[name] = med
            print(json.dumps(row), flush=True)
            del sides
            torch.cuda.empty_cache()
        a, b = kept["uniform 8 x 4096"], kept["uniform 2 x 16384"]
        names = [f"{s} {kind}" for kind in ("fwd", "fwd_bwd") for s in ("local 64", "local 512", "bidir")]
        print(json.dumps({"d": d, "H": H, "Hkv": Hkv, "growth 8 x 4096 -> 2 x 16384": {n: r3(b[n][0] / a[n][0]) for n in names}}), flush=True)
    med = measure(stack_sides(g, MIXES["uniform 8 x 4096"]), args)
    print(json.dumps({"stack": "encoder_stack_packed, 4 layers, E 768, 12 heads, 8 x 4096, fwd_bwd", "alternating (64, 64) / None ms": r3(med["alternating"][0]),
                      "all None": {"ms": r3(med["global"][0]), "aa": r3(med["global again"][0] / med["global"][0]),
                                   "over_alternating": r3(med["global"][0] / med["alternating"][0])}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
