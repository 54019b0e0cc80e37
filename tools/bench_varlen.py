"""The packed variable-length call against what a caller can do without it, on the MI355X: one JSON line per length mix.

Setup: bf16, d = 128, H = 32, Hkv = 8, packed (T, H, d).  Length mixes: uniform (8 x 4096), long-tailed (one 16384 and seven of
512 .. 2048), many short (256 x 128).  Measured per mix, forward alone (``fwd``) and forward + backward (``fwd_bwd``):

  packed     flash_attn_varlen(q, k, v, cu_seqlens), without a window and with window = 1024
  (a) padded flash_attn_gqa(causal=True) on the batch padded to the longest sequence: the one thing a caller can do today without a
             window.  Its padded rows are wasted; the real rows are right without a key mask only because the padding lies BEHIND
             every sequence and the mask is causal (a padded key is never admitted by a real query); the padded rows' outputs and
             gradients are garbage the caller drops.
  (b) loop   one flash_attn_gqa(causal=True[, window=1024]) call per sequence, with and without the window
  (c) batch  uniform lengths only: the batched flash_attn_gqa(causal=True[, window=1024]); against the windowed one the packed call
             runs the same kernel bodies on the same blocks, so the difference is the cost of the map and the schedule launch
  schedule   the forward call at H = Hkv = 1, d = 32 with nseq one-token sequences in T rows: the schedule launch (maps of the same
             size, T - nseq rows of 32 floats zeroed) and a forward launch whose blocks hold one row each: an upper bound on the
             schedule launch alone

The conventions are those of tools/bench_window_train.py: all sides of one mix run window by window in turn, the median of
``--repeats`` windows is reported, and every baseline is measured twice (``*_again``): its A/A ratio (``aa``) is the noise the ratios
are read against.  ``pairs`` is the number of (query, key) pairs a side computes over the pairs the packed call computes under the
same mask: the share of the work that is wasted, to read the time ratios against.  A ratio above 1: the packed call is faster.

    python tools/bench_varlen.py [--repeats 5] [--window-ms 40] > profiles/varlen_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import device_ops  # noqa: E402

D, H, HKV, W = 128, 32, 8, 1024
MIXES = {
    "uniform 8 x 4096": [4096] * 8,
    "long tail 16384 + 7 of 512..2048": [16384, 512, 768, 1024, 1280, 1536, 1792, 2048],
    "many short 256 x 128": [128] * 256,
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


def pairs(n, w=None):
    """Admitted (query, key) pairs of one causal sequence of n tokens under a window of w (None: none)."""
    w = n if w is None else min(w, n)
    return w * (w + 1) // 2 + (n - w) * w


def both(name, make):
    """fwd and fwd_bwd callables of one side: make(grad) -> (a function that returns [(output, its cotangent)], the leaves)."""
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


def sides_of(g, lengths):
    T, nseq, longest = sum(lengths), len(lengths), max(lengths)
    q, do = (rnd(g, T, H, D) for _ in range(2))
    k, v = (rnd(g, T, HKV, D) for _ in range(2))
    dof = do.float()
    starts = [0] + list(torch.tensor(lengths).cumsum(0).tolist())
    cu = torch.tensor(starts, dtype=torch.int32, device="cuda")

    def leaf(t, grad):
        return t.clone().requires_grad_() if grad else t

    def packed(window):
        def make(grad):
            qq, kk, vv = (leaf(t, grad) for t in (q, k, v))
            return (lambda: [(device_ops.flash_attn_varlen(qq, kk, vv, cu, window=window), dof)]), [qq, kk, vv]
        return make

    def loop(window):
        def make(grad):
            seqs = [tuple(leaf(t[s:e][None].contiguous(), grad) for t in (q, k, v)) + (dof[s:e][None],) for s, e in zip(starts, starts[1:])]
            return (lambda: [(device_ops.flash_attn_gqa(a, b, c, True, None, "bnhd", window), go) for a, b, c, go in seqs],
                    [t for sq in seqs for t in sq[:3]])
        return make

    def batched(shape_n, window):
        def make(grad):
            pq, pdo = (rnd(g, nseq, shape_n, H, D) for _ in range(2))
            pk, pv = (rnd(g, nseq, shape_n, HKV, D) for _ in range(2))
            pq, pk, pv = (leaf(t, grad) for t in (pq, pk, pv))
            pdo = pdo.float()
            return (lambda: [(device_ops.flash_attn_gqa(pq, pk, pv, True, None, "bnhd", window), pdo)]), [pq, pk, pv]
        return make
    sides = {}
    sides.update(both("packed", packed(None)))
    sides.update(both(f"packed W{W}", packed(W)))
    sides.update(both("padded", batched(longest, None)))
    sides.update(both("loop", loop(None)))
    sides.update(both(f"loop W{W}", loop(W)))
    if len(set(lengths)) == 1 and longest > W:
        sides.update(both(f"batched W{W}", batched(longest, W)))
    for n in [n for n in sides if not n.startswith("packed")]:
        sides[n + " again"] = sides[n]
    # the schedule launch, with next to nothing behind it
    sq, sk = (rnd(g, T, 1, 32) for _ in range(2))
    scu = torch.arange(nseq + 1, dtype=torch.int32, device="cuda")
    sws = device_ops.varlen_workspace(sq, sk, scu, backward=False)
    so, sl = torch.empty((T, 1, 32), device="cuda"), torch.empty((1, T), device="cuda")
    sides["schedule"] = lambda: device_ops.flash_attn_varlen_fwd(sq, sk, sk, scu, out=so, workspace=sws, lse=sl)
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
        raise SystemExit("bench_varlen.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "H": H, "Hkv": HKV, "window": W,
                      "repeats": args.repeats, "window_ms": args.window_ms,
                      "ratios": "baseline time over packed time under the same mask: above 1, the packed call is faster"}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    r3 = lambda x: round(x, 3)
    for i, (name, lengths) in enumerate(MIXES.items()):
        if i not in args.mix:
            continue
        sides = sides_of(g, lengths)
        reps = {n: max(args.reps, int(args.window_ms / window_ms(c, 2, args.warmup)) + 1) for n, c in sides.items()}
        xs = {n: [] for n in sides}
        for _ in range(args.repeats):
            for n, c in sides.items():
                xs[n].append(window_ms(c, reps[n], 1))
        med = {n: statistics.median(v) for n, v in xs.items()}
        nseq, longest = len(lengths), max(lengths)
        work = {None: sum(pairs(n) for n in lengths), W: sum(pairs(n, W) for n in lengths)}
        row = {"mix": name, "T": sum(lengths), "nseq": nseq, "schedule_and_one_row_blocks_fwd_ms": r3(med["schedule"])}
        for w, tag in ((None, "packed"), (W, f"packed W{W}")):
            for kind in ("fwd", "fwd_bwd"):
                row[f"{tag} {kind}_ms"] = r3(med[f"{tag} {kind}"])
                row[f"{tag} {kind}_min_max_ms"] = [r3(min(xs[f"{tag} {kind}"])), r3(max(xs[f"{tag} {kind}"]))]
        for base, w, share in (("padded", None, nseq * pairs(longest) / work[None]), ("loop", None, 1.0), (f"loop W{W}", W, 1.0),
                               (f"batched W{W}", W, 1.0)):
            if f"{base} fwd" not in med:
                continue
            tag = "packed" if w is None else f"packed W{W}"
            for kind in ("fwd", "fwd_bwd"):
                b, again = med[f"{base} {kind}"], med[f"{base} {kind} again"]
                row[f"{base} {kind}"] = {"ms": r3(b), "aa": r3(again / b), "pairs": r3(share), "over_packed": r3(b / med[f"{tag} {kind}"])}
        print(json.dumps(row), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
