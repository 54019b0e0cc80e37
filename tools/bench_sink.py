"""Attention-sink tokens against the windowed calls on the MI355X: one JSON line per measurement.

The question: what do S sink tokens cost beside a window of W?  From tile counts alone a block reads ceil(S / 128) more 128-key
tiles beside the W + 255 keys of its window range at the most, about 128 / (W + 255) = 3 % at W = 4096 for one sink tile; that is
a count of tiles, not a time.  Shapes (bf16, d = 128, [B][N][H][d], B = 32, H = 32, Hkv = 8):
  decode   Nq = 1 at length 32768, W = 4096:  sink = 4 and sink = 128   against   the windowed call (no sinks), slab caches
  paged    the same decode calls through a block table (pages of 256 rows, the identity table on the same memory)
  extend   512 new tokens (fused append) after a prefix of 32768, W = 4096:  sink = 4 and sink = 128   against   the windowed call
All sides of a measurement run in one process on the same caches, window by window in turn (``--repeats`` windows per side, each of
at least ``--reps`` calls and ``--window-ms`` of device time); the windowed baseline is measured TWICE (``window`` /
``window_again``): the A/A ratio of the two is the noise the ratios are read against.

    python tools/bench_sink.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/sink_bench.txt
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402
from bench_window import B, D, H, HKV, LONG, W, rnd, run  # noqa: E402

SINKS = (4, 128)
PAGE = 256


class Call:
    """One side: T new tokens against caches of ``prefix`` + T rows under a window of W, with ``sink`` sink tokens (None: the
    windowed call); ``paged``: through a block table over the same memory."""

    def __init__(self, q, kc, vc, extend, prefix, T, sink, paged):
        self.extend, self.T, self.N, self.sink = extend, T, prefix + T, sink
        self.q = q
        self.new = dict(k_new=kc[:, prefix:].contiguous(), v_new=vc[:, prefix:].contiguous()) if extend else {}
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.kw = dict(window=W) if sink is None else dict(window=W, sink=sink)
        self.kc, self.vc = kc, vc
        if paged:   # (the slab's memory as a pool: sequence b owns the pages b * mp .. b * mp + mp - 1)
            mp = self.N // PAGE
            assert mp * PAGE == self.N
            self.kc, self.vc = (c.view(B * mp, PAGE, HKV, D) for c in (kc, vc))
            self.kw["block_table"] = torch.arange(B * mp, dtype=torch.int32, device="cuda").view(B, mp)
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        new_ws = device_ops.extend_workspace if extend else device_ops.decode_workspace
        self.ws = new_ws(self.q, self.kc, **self.kw)

    def __call__(self):
        return self.fn(self.q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, **self.kw, **self.new)

    def splits(self):
        lib = _lib.decode()
        fn = lib.fa_mi355x_extend_sink_splits if self.extend else lib.fa_mi355x_decode_sink_splits
        return fn(B, H, HKV, self.T, self.N, D, 1, W, self.sink or 0)


def measure(extend, T, paged, args):
    g = torch.Generator(device="cuda").manual_seed(0)
    prefix = LONG - (0 if extend else T)
    kc, vc, q = rnd(g, B, prefix + T, HKV, D), rnd(g, B, prefix + T, HKV, D), rnd(g, B, T, H, D)
    sides = {"window": Call(q, kc, vc, extend, prefix, T, None, paged)}
    for S in SINKS:
        sides[f"sink{S}"] = Call(q, kc, vc, extend, prefix, T, S, paged)
    sides["window_again"] = sides["window"]
    res, reps = run(sides, args)
    m = lambda n: res[n]["median_ms"]
    row = {"call": ("extend" if extend else "decode") + ("-paged" if paged else ""), "B": B, "H": H, "Hkv": HKV, "T": T, "window": W,
           "len": prefix + T, "splits": {n: sides[n].splits() for n in sides if n != "window_again"}, "calls_per_window": reps, **res,
           "aa_window": round(m("window_again") / m("window"), 3),
           "tile_count_estimate": {f"sink{S}": round(1 + -(-S // 128) * 128 / (W + 255), 3) for S in SINKS}}
    for S in SINKS:
        row[f"sink{S}_over_window"] = round(m(f"sink{S}") / m("window"), 3)
    a, b = sides["window"](), sides["sink4"]()
    torch.cuda.synchronize()
    row["max_abs_diff_sink4_vs_window"] = float((a[0] - b[0]).abs().max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sink.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "causal": True,
                      "reps": args.reps, "repeats": args.repeats, "page_size": PAGE}), flush=True)
    print(json.dumps(measure(False, 1, False, args)), flush=True)
    print(json.dumps(measure(False, 1, True, args)), flush=True)
    print(json.dumps(measure(True, 512, False, args)), flush=True)


if __name__ == "__main__":
    main()
