"""The causal two-array packed call (a cached prefix) against what a caller can do without it, on the MI355X: one JSON line per mix.

Setup: bf16, d = 128, H = 32, Hkv = 8, packed q (Tq, H, d) and k, v (Tk, Hkv, d); sequence b has n_q new tokens behind a prefix of
n_k - n_q rows.  Measured per mix, forward alone (``fwd``) and forward + backward (``fwd_bwd``):

  a  8 x 512 behind 8192
      packed  flash_attn_varlen_prefix(q, k, v, cu_seqlens_q, cu_seqlens_k)
      full    flash_attn_varlen over the full 8704-token sequences: what a user runs today to get gradients through this shape; it
              recomputes every prefix row
      extend  flash_attn_extend on a slab cache (8, 8704, Hkv, d) that holds the same keys: forward only, not differentiable
  b  long tail: 2048 behind 16384, seven of 64 .. 512 behind 512 .. 4096
      packed, full   as above
  c  8 x 4096, no prefix (one array for both sides)
      packed  flash_attn_varlen_prefix(q, k, v, cu_seqlens)
      full    flash_attn_varlen(q, k, v, cu_seqlens): the same work on the packed causal library's kernels
      batched flash_attn_gqa(causal=True) on (8, 4096, heads, d): the MFMA-slot pipelines; expect the packed call to LOSE here

The conventions are those of tools/bench_bidir.py (its helpers are used): all sides of one mix run window by window in turn, the
median of ``--repeats`` windows is reported, and every baseline is measured twice (``* again``): its A/A ratio (``aa``) is the noise
the ratios are read against.  ``pairs`` is the number of (query, key) pairs a side computes over the pairs the packed call computes.
A ratio above 1: the packed call is faster.

    python tools/bench_prefix.py [--repeats 5] [--window-ms 40] > profiles/prefix_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_bidir import D, H, HKV, both, cu_of, leaf, rnd, window_ms  # noqa: E402
from flash_attention_minitorch_amd import device_ops  # noqa: E402

# name -> (new tokens per sequence, prefix rows per sequence)
MIXES = {
    "a: 8 x 512 behind 8192": ([512] * 8, [8192] * 8),
    "b: long tail, 2048 behind 16384 + 7 of 64..512 behind 512..4096": ([2048, 64, 128, 192, 256, 320, 384, 512],
                                                                        [16384, 512, 1024, 1536, 2048, 2560, 3072, 4096]),
    "c: 8 x 4096, no prefix": ([4096] * 8, [0] * 8),
}


def sides_of(g, nq, npre):
    nk = [a + b for a, b in zip(nq, npre)]
    Tq, Tk, nseq = sum(nq), sum(nk), len(nq)
    q, do = (rnd(g, Tq, H, D) for _ in range(2))
    k, v = (rnd(g, Tk, HKV, D) for _ in range(2))
    dof = do.float()
    (_, cuq), (_, cuk) = cu_of(nq), cu_of(nk)
    one_array = not any(npre)

    def packed(grad):
        qq, kk, vv = (leaf(t, grad) for t in (q, k, v))
        return (lambda: [(device_ops.flash_attn_varlen_prefix(qq, kk, vv, cuq, None if one_array else cuk), dof)]), [qq, kk, vv]
    sides = both("packed", packed)

    def full(grad):   # queries for every key row: the prefix rows are recomputed
        fq, fdo = (q, dof) if one_array else (rnd(g, Tk, H, D), rnd(g, Tk, H, D).float())
        qq, kk, vv = (leaf(t, grad) for t in (fq, k, v))
        return (lambda: [(device_ops.flash_attn_varlen(qq, kk, vv, cuk), fdo)]), [qq, kk, vv]
    sides.update(both("full", full))
    if len(set(nq)) == 1 and len(set(npre)) == 1 and not one_array:
        cq, ck, cv = q.view(nseq, nq[0], H, D), k.view(nseq, nk[0], HKV, D), v.view(nseq, nk[0], HKV, D)

        def extend_fwd():   # (it allocates out, lse and its workspace per call, as the autograd sides allocate theirs)
            device_ops.flash_attn_extend(cq, ck, cv, None, causal=True)
        sides["extend fwd"] = extend_fwd
    if one_array:
        def batched(grad):
            pq, pdo = (rnd(g, nseq, nq[0], H, D) for _ in range(2))
            pk, pv = (rnd(g, nseq, nq[0], HKV, D) for _ in range(2))
            pq, pk, pv = (leaf(t, grad) for t in (pq, pk, pv))
            pdo = pdo.float()
            return (lambda: [(device_ops.flash_attn_gqa(pq, pk, pv, True), pdo)]), [pq, pk, pv]
        sides.update(both("batched", batched))
    for n in [n for n in sides if not n.startswith("packed")]:
        sides[n + " again"] = sides[n]
    return sides


def causal_pairs(n_q, n_k):
    """(query, key) pairs under the bottom-right aligned mask: row i admits i + n_k - n_q + 1 keys."""
    return n_q * (n_k - n_q) + n_q * (n_q + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0, help="least device time of one timed window")
    ap.add_argument("--mix", type=int, nargs="*", default=list(range(len(MIXES))))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "H": H, "Hkv": HKV, "repeats": args.repeats,
                      "window_ms": args.window_ms,
                      "ratios": "baseline time over packed time: above 1, the packed call is faster"}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    r3 = lambda x: round(x, 3)
    for i, (name, (nq, npre)) in enumerate(MIXES.items()):
        if i not in args.mix:
            continue
        sides = sides_of(g, nq, npre)
        reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
        xs = {n: [] for n in sides}
        for _ in range(args.repeats):
            for n, c in sides.items():
                xs[n].append(window_ms(c, reps[n], 1))
        med = {n: statistics.median(v) for n, v in xs.items()}
        nk = [a + b for a, b in zip(nq, npre)]
        work = sum(causal_pairs(a, b) for a, b in zip(nq, nk))
        row = {"mix": name, "Tq": sum(nq), "Tk": sum(nk), "nseq": len(nq)}
        for kind in ("fwd", "fwd_bwd"):
            row[f"packed {kind}_ms"] = r3(med[f"packed {kind}"])
            row[f"packed {kind}_min_max_ms"] = [r3(min(xs[f"packed {kind}"])), r3(max(xs[f"packed {kind}"]))]
        full_pairs = sum(causal_pairs(b, b) for b in nk) / work
        for base, share in (("full", full_pairs), ("extend", 1.0), ("batched", 1.0)):
            for kind in ("fwd", "fwd_bwd"):
                if f"{base} {kind}" not in med:
                    continue
                b, again = med[f"{base} {kind}"], med[f"{base} {kind} again"]
                row[f"{base} {kind}"] = {"ms": r3(b), "aa": r3(again / b), "pairs": r3(share), "over_packed": r3(b / med[f"packed {kind}"])}
        print(json.dumps(row), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
