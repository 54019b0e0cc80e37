"""The bidirectional packed call against what a caller can do without it, on the MI355X: one JSON line per length mix.

Setup: bf16, d = 128, H = 32, Hkv = 8, packed q (Tq, H, d) and k, v (Tk, Hkv, d).  Measured per mix, forward alone (``fwd``) and
forward + backward (``fwd_bwd``):

  long tail   self-attention on one sequence of 16384 and seven of 512 .. 2048
      packed  flash_attn_varlen_bidir(q, k, v, cu_seqlens)
      padded  the batched non-causal call on the batch padded to the longest sequence.  The padding lies behind every sequence and
              the mask is not causal, so the padded keys must be masked: flash_attn_fwd_masked / flash_attn_bwd_masked, the entry
              points that take the (B, N) key-padding mask.  They take (B, H, N, d) tensors with H key heads, so k and v are expanded
              to the 32 query heads and head-split BEFORE the timed window (the baseline is not charged for those copies).
      loop    one flash_attn_gqa(causal=False) call per sequence
  cross       nq of 64 .. 512 against memories of 512 .. 8192
      packed  flash_attn_varlen_bidir(q, k, v, cu_seqlens_q, cu_seqlens_k)
      sdpa    torch.nn.functional.scaled_dot_product_attention on the batch padded on both sides, (B, H, 512, d) against
              (B, H, 8192, d) with a boolean (B, 1, 1, 8192) key mask: the only alternative a user has today (Nq != Nk exists nowhere
              else in training).  k and v are expanded to 32 heads before the timed window.
  uniform     8 x 4096, self-attention
      packed  flash_attn_varlen_bidir
      batched flash_attn_gqa(causal=False) on (8, 4096, heads, d): the MFMA-slot pipelines; expect the packed call to LOSE here

The conventions are those of tools/bench_varlen.py: all sides of one mix run window by window in turn, the median of ``--repeats``
windows is reported, and every baseline is measured twice (``* again``): its A/A ratio (``aa``) is the noise the ratios are read
against.  ``pairs`` is the number of (query, key) pairs a side computes over the pairs the packed call computes: the share of the
work that is wasted, to read the time ratios against.  A ratio above 1: the packed call is faster.

    python tools/bench_bidir.py [--repeats 5] [--window-ms 40] > profiles/bidir_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import device_ops  # noqa: E402

D, H, HKV = 128, 32, 8
# name -> (nq per sequence, nk per sequence or None for self-attention)
MIXES = {
    "long tail self 16384 + 7 of 512..2048": ([16384, 512, 768, 1024, 1280, 1536, 1792, 2048], None),
    "cross nq 64..512 on nk 512..8192": ([64, 128, 192, 256, 320, 384, 448, 512], [512, 1024, 2048, 3072, 4096, 6144, 8192, 8192]),
    "uniform self 8 x 4096": ([4096] * 8, None),
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


def rnd(g, *shape):
    return torch.rand(shape, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)


def both(name, make):
    """fwd and fwd_bwd callables of one autograd side: make(grad) -> (a function that returns [(output, its cotangent)], the leaves)."""
    (f, _), (t, leaves) = make(False), make(True)

    def fwd():
        with torch.no_grad():
            f()

    def fwd_bwd():
        for leaf in leaves:
            leaf.grad = None
        outs = t()
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    return {f"{name} fwd": fwd, f"{name} fwd_bwd": fwd_bwd}


def leaf(t, grad):
    return t.clone().requires_grad_() if grad else t


def cu_of(lengths):
    starts = [0] + list(torch.tensor(lengths).cumsum(0).tolist())
    return starts, torch.tensor(starts, dtype=torch.int32, device="cuda")


def sides_of(g, nq, nk):
    self_attn = nk is None
    nk = nq if self_attn else nk
    Tq, Tk, nseq = sum(nq), sum(nk), len(nq)
    q, do = (rnd(g, Tq, H, D) for _ in range(2))
    k, v = (rnd(g, Tk, HKV, D) for _ in range(2))
    dof = do.float()
    (sq, cuq), (sk, cuk) = cu_of(nq), cu_of(nk)

    def packed(grad):
        qq, kk, vv = (leaf(t, grad) for t in (q, k, v))
        return (lambda: [(device_ops.flash_attn_varlen_bidir(qq, kk, vv, cuq, None if self_attn else cuk), dof)]), [qq, kk, vv]
    sides = both("packed", packed)
    if self_attn and len(set(nq)) > 1:
        longest = max(nq)
        # the padded, key-masked batch: (B, H, N, d) with all H heads; the mask is 0 on a sequence's keys and -inf behind them
        pq, pk, pv, pdo = (rnd(g, nseq, H, longest, D) for _ in range(4))
        mask = torch.full((nseq, longest), float("-inf"), device="cuda")
        for b, n in enumerate(nq):
            mask[b, :n] = 0.0

        def padded_fwd():
            return device_ops.flash_attn_fwd_masked(pq, pk, pv, mask)

        def padded_fwd_bwd():
            o, l, m = device_ops.flash_attn_fwd_masked(pq, pk, pv, mask)
            device_ops.flash_attn_bwd_masked(pq, pk, pv, o, pdo, l, m, mask)
        sides.update({"padded fwd": padded_fwd, "padded fwd_bwd": padded_fwd_bwd})

        def loop(grad):
            seqs = [tuple(leaf(t[s:e][None].contiguous(), grad) for t in (q, k, v)) + (dof[s:e][None],) for s, e in zip(sq, sq[1:])]
            return (lambda: [(device_ops.flash_attn_gqa(a, b, c, False), go) for a, b, c, go in seqs]), [t for s in seqs for t in s[:3]]
        sides.update(both("loop", loop))
    if self_attn and len(set(nq)) == 1:
        def batched(grad):
            pq, pdo = (rnd(g, nseq, nq[0], H, D) for _ in range(2))
            pk, pv = (rnd(g, nseq, nq[0], HKV, D) for _ in range(2))
            pq, pk, pv = (leaf(t, grad) for t in (pq, pk, pv))
            pdo = pdo.float()
            return (lambda: [(device_ops.flash_attn_gqa(pq, pk, pv, False), pdo)]), [pq, pk, pv]
        sides.update(both("batched", batched))
    if not self_attn:
        Nq, Nk = max(nq), max(nk)
        keep = torch.zeros((nseq, 1, 1, Nk), dtype=torch.bool, device="cuda")
        for b, n in enumerate(nk):
            keep[b, :, :, :n] = True

        def sdpa(grad):
            pq, pk, pv, pdo = (rnd(g, nseq, H, n, D) for n in (Nq, Nk, Nk, Nq))
            pq, pk, pv = (leaf(t, grad) for t in (pq, pk, pv))
            return (lambda: [(torch.nn.functional.scaled_dot_product_attention(pq, pk, pv, attn_mask=keep), pdo)]), [pq, pk, pv]
        sides.update(both("sdpa", sdpa))
    for n in [n for n in sides if not n.startswith("packed")]:
        sides[n + " again"] = sides[n]
    return sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0, help="least device time of one timed window")
    ap.add_argument("--mix", type=int, nargs="*", default=list(range(len(MIXES))))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bidir.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "H": H, "Hkv": HKV, "repeats": args.repeats,
                      "window_ms": args.window_ms,
                      "ratios": "baseline time over packed time: above 1, the packed call is faster"}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    r3 = lambda x: round(x, 3)
    for i, (name, (nq, nk)) in enumerate(MIXES.items()):
        if i not in args.mix:
            continue
        sides = sides_of(g, nq, nk)
        reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
        xs = {n: [] for n in sides}
        for _ in range(args.repeats):
            for n, c in sides.items():
                xs[n].append(window_ms(c, reps[n], 1))
        med = {n: statistics.median(v) for n, v in xs.items()}
        nkk = nq if nk is None else nk
        work = sum(a * b for a, b in zip(nq, nkk))
        row = {"mix": name, "Tq": sum(nq), "Tk": sum(nkk), "nseq": len(nq)}
        for kind in ("fwd", "fwd_bwd"):
            row[f"packed {kind}_ms"] = r3(med[f"packed {kind}"])
            row[f"packed {kind}_min_max_ms"] = [r3(min(xs[f"packed {kind}"])), r3(max(xs[f"packed {kind}"]))]
        padded_pairs = len(nq) * max(nq) * max(nkk) / work
        for base, share in (("padded", padded_pairs), ("loop", 1.0), ("batched", 1.0), ("sdpa", padded_pairs)):
            if f"{base} fwd" not in med:
                continue
            for kind in ("fwd", "fwd_bwd"):
                b, again = med[f"{base} {kind}"], med[f"{base} {kind} again"]
                row[f"{base} {kind}"] = {"ms": r3(b), "aa": r3(again / b), "pairs": r3(share), "over_packed": r3(b / med[f"packed {kind}"])}
        print(json.dumps(row), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
