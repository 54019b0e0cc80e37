"""An fp8 (e4m3) KV cache against the bf16 one on the MI355X: one JSON line per (shape, slab or paged).

Both sides run the same call on a cache of the same shape in one process: the bf16 call on bf16 caches (the yardstick: the
FP8 = false builds, unchanged) and the fp8 call on caches of e4m3 bytes with per-head scales, which reads half the cache bytes and
widens every staged tile to bf16 on its way to LDS.  The bf16 side is measured twice, interleaved with the fp8 side (A, fp8, A'),
so every row carries its own A/A figure: ``aa`` is median(A') / median(A) and ``bf16_spread`` the (max - min) / median over both.
Shapes (d = 128, [B][N][H][d], causal):
  decode   Nq = 1, B = 32, H = 32, Hkv = 32 and 8, 4096 cached tokens; and B = 1, H = Hkv = 8, 65536 cached tokens
  extend   T = 512 new tokens after a prefix of 8192, B = 8, H = 32, Hkv = 8 (the fused append + attention, as tools/bench_extend.py)
  append   the append launch alone: the extend shape's 512 tokens, and one token for B = 32, Hkv = 8
each on slabs and on a pool of 128-row pages under a randomly permuted table.
``tbps``: terabytes per second counted on the K and V cache bytes the call reads (2 * B * Hkv * N * d elements of 2 bytes or of 1);
q, the output and the partials are not counted.  The ideal at the bandwidth-bound shapes is fp8_over_bf16 = 0.5.
Per side: milliseconds per call, device events around a window of calls (at least ``--reps``, and enough of them to fill
``--window-ms`` of device time); ``--repeats`` windows per side, median and min .. max reported.

    python tools/bench_fp8.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/fp8_bench.txt
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
PAGE = 128
# name -> (extend, B, H, Hkv, prefix, T)
SHAPES = {
    "decode-B32-H32-Hkv32-len4096": (False, 32, 32, 32, 4095, 1),
    "decode-B32-H32-Hkv8-len4096": (False, 32, 32, 8, 4095, 1),
    "decode-B1-H8-Hkv8-len65536": (False, 1, 8, 8, 65535, 1),
    "extend-B8-H32-Hkv8-prefix8192-T512": (True, 8, 32, 8, 8192, 512),
}
# name -> (B, Hkv, prefix, T): the append launch alone
APPENDS = {
    "append-B8-Hkv8-T512": (8, 8, 8192, 512),
    "append-B32-Hkv8-T1": (32, 8, 4095, 1),
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


def quantise(t, scale):
    """(B, N, Hkv, D) bf16 -> e4m3 bytes of t / scale[h] (torch's cast: round to nearest even)."""
    return (t.float() / scale[None, None, :, None]).clamp(-448, 448).to(torch.float8_e4m3fn)


def paginate(slab, table):
    """The pool (pages of PAGE rows) that holds ``slab`` (B, N, Hkv, D) under ``table``."""
    B, N, Hkv, _ = slab.shape
    pool = torch.empty((table.numel(), PAGE, Hkv, D), dtype=slab.dtype, device="cuda")
    pool.view(torch.uint8)[table.long().view(-1)] = slab.reshape(table.numel(), PAGE, Hkv, D).view(torch.uint8)
    return pool


class Case:
    """One shape: bf16 caches (B, N, Hkv, D) with N = prefix + T, their e4m3 quantisation with per-head scales amax / 448, the T new
    tokens' q (and k, v for the fused and append shapes), and with ``paged`` the pools that hold the same rows."""

    def __init__(self, B, H, Hkv, prefix, T, extend, paged, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.B, self.H, self.Hkv, self.T, self.N, self.extend = B, H, Hkv, T, prefix + T, extend
        kc, vc = rnd(B, self.N, Hkv, D), rnd(B, self.N, Hkv, D)
        self.q = rnd(B, T, H, D)
        self.new = dict(k_new=kc[:, prefix:].contiguous(), v_new=vc[:, prefix:].contiguous())
        self.ks, self.vs = (t.float().abs().amax(dim=(0, 1, 3)).div(448).contiguous() for t in (kc, vc))
        k8, v8 = quantise(kc, self.ks), quantise(vc, self.vs)
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.where = {}
        if paged:
            mp = self.N // PAGE
            assert mp * PAGE == self.N
            ids = torch.randperm(B * mp, generator=torch.Generator().manual_seed(1))
            self.where = dict(block_table=ids.view(B, mp).to(torch.int32).cuda())
            kc, vc, k8, v8 = (paginate(t, self.where["block_table"]) for t in (kc, vc, k8, v8))
        self.bf16_caches, self.fp8_caches = (kc, vc), (k8, v8)
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        self.ws = (device_ops.extend_workspace if extend else device_ops.decode_workspace)(self.q, kc, **self.where)

    def bf16(self):
        return self.fn(self.q, *self.bf16_caches, self.lens, causal=True, workspace=self.ws, **(self.new if self.extend else {}), **self.where)

    def fp8(self):
        return self.fn(self.q, *self.fp8_caches, self.lens, causal=True, workspace=self.ws, k_scale=self.ks, v_scale=self.vs,
                       **(self.new if self.extend else {}), **self.where)

    def append_bf16(self):
        device_ops.extend_append(self.new["k_new"], self.new["v_new"], *self.bf16_caches, self.lens, **self.where)

    def append_fp8(self):
        device_ops.extend_append(self.new["k_new"], self.new["v_new"], *self.fp8_caches, self.lens, k_scale=self.ks, v_scale=self.vs, **self.where)


def measure(name, case, sides, args, cache_bytes):
    a, b = sides
    a(), b()
    torch.cuda.synchronize()
    reps = max(args.reps, int(args.window_ms / window_ms(a, 5, args.warmup)) + 1)
    xs = {"bf16": [], "fp8": [], "bf16_again": []}
    for i in range(args.repeats):   # A, fp8, A': window by window
        for side, fn in (("bf16", a), ("fp8", b), ("bf16_again", a)):
            xs[side].append(window_ms(fn, reps, args.warmup if i == 0 else 1))
    row = {"shape": name, "cache": "paged" if case.where else "slab", "calls_per_window": reps}
    row.update({s: stats(x) for s, x in xs.items()})
    base = row["bf16"]["median_ms"]
    both = xs["bf16"] + xs["bf16_again"]
    row["aa"] = round(row["bf16_again"]["median_ms"] / base, 3)
    row["bf16_spread"] = round((max(both) - min(both)) / statistics.median(both), 3)
    row["fp8_over_bf16"] = round(row["fp8"]["median_ms"] / base, 3)
    if cache_bytes:
        row["bf16_tbps"] = round(2 * cache_bytes / base / 1e9, 2)
        row["fp8_tbps"] = round(cache_bytes / row["fp8"]["median_ms"] / 1e9, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--shape", nargs="+", default=list(SHAPES) + list(APPENDS), choices=list(SHAPES) + list(APPENDS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "queries": "bf16", "layout": "bnhd", "causal": True, "page_size": PAGE,
                      "reps": args.reps, "repeats": args.repeats}), flush=True)
    for name in args.shape:
        for paged in (False, True):
            if name in SHAPES:
                extend, B, H, Hkv, prefix, T = SHAPES[name]
                case = Case(B, H, Hkv, prefix, T, extend, paged)
                row = measure(name, case, (case.bf16, case.fp8), args, B * Hkv * case.N * D * 2)   # K and V, one byte per element
                splits = _lib.decode().fa_mi355x_extend_splits if extend else _lib.decode().fa_mi355x_decode_splits_gqa
                row["splits"] = splits(B, H, Hkv, T, case.N, D, 1)
            else:
                B, Hkv, prefix, T = APPENDS[name]
                case = Case(B, Hkv, Hkv, prefix, T, True, paged)
                row = measure(name, case, (case.append_bf16, case.append_fp8), args, 0)
            print(json.dumps(row), flush=True)
            del case
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
