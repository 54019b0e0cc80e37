"""Sliding-window attention against the unwindowed calls on the MI355X: one JSON line per measurement.

The claim under test: a windowed call at length L costs about what the unwindowed call costs at length W (the kernels start every
row block's key range at its window and the splits follow the window span), and far less than the unwindowed call at length L.
Shapes (bf16, d = 128, [B][N][H][d], B = 32, H = 32, Hkv = 8, slab caches):
  decode   Nq = 1:  window W = 4096 at length 32768   against   no window at length 4096   and   no window at length 32768
  extend   512 new tokens (fused append) after a prefix of 32768 with W = 4096   against   no window after a prefix of 4096   and
           no window after the prefix of 32768
The short baseline runs on a cache of its own capacity (its split policy is that of a 4096-token cache, as in the README's rows).
All sides of a measurement run in one process, window by window in turn (``--repeats`` windows per side, each of at least ``--reps``
calls and ``--window-ms`` of device time); every baseline is measured TWICE (``short`` / ``short_again``, ``long`` / ``long_again``):
the A/A ratio of the two is the noise the ratios are read against.  decode also reports the largest difference between the
windowed result and the short call on the last W rows of the long cache (one query: the same keys).
``--unwindowed-rows``: only the README's existing decode and extend rows through the unwindowed entry points (window=None), for
an A/B of two builds of the library with tools/ab_dirs.sh.

    python tools/bench_window.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/window_bench.txt
    tools/ab_dirs.sh "python tools/bench_window.py --unwindowed-rows" 2
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

D, B, H, HKV = 128, 32, 32, 8
W, LONG = 4096, 32768


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


def rnd(g, *shape):
    return torch.rand(shape, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)


class Call:
    """One side: T new tokens against a slab cache of ``prefix`` + T rows, with or without a window."""

    def __init__(self, g, extend, prefix, T, window, B=B, Hkv=HKV, caches=None):
        self.extend, self.B, self.Hkv, self.T, self.N, self.window = extend, B, Hkv, T, prefix + T, window
        self.kc, self.vc = caches if caches is not None else (rnd(g, B, self.N, Hkv, D), rnd(g, B, self.N, Hkv, D))
        self.q = rnd(g, B, T, H, D)
        self.new = dict(k_new=self.kc[:, prefix:].contiguous(), v_new=self.vc[:, prefix:].contiguous()) if extend else {}
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        new_ws = device_ops.extend_workspace if extend else device_ops.decode_workspace
        self.ws = new_ws(self.q, self.kc, window=window)

    def __call__(self):
        return self.fn(self.q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, window=self.window, **self.new)

    def splits(self):
        lib = _lib.decode()
        if self.window is None:
            fn = lib.fa_mi355x_extend_splits if self.extend else lib.fa_mi355x_decode_splits_gqa
            return fn(self.B, H, self.Hkv, self.T, self.N, D, 1)
        fn = lib.fa_mi355x_extend_window_splits if self.extend else lib.fa_mi355x_decode_window_splits
        return fn(self.B, H, self.Hkv, self.T, self.N, D, 1, self.window)


def run(sides, args):
    """sides: name -> Call.  The windows of all sides in turn; name -> stats."""
    first = next(iter(sides.values()))
    reps = max(args.reps, int(args.window_ms / window_ms(first, 5, args.warmup)) + 1)
    xs = {name: [] for name in sides}
    for i in range(args.repeats):
        for name, call in sides.items():
            xs[name].append(window_ms(call, reps, args.warmup if i == 0 else 1))
    return {name: stats(v) for name, v in xs.items()}, reps


def measure(extend, T, args):
    g = torch.Generator(device="cuda").manual_seed(0)
    long_ = Call(g, extend, LONG - (0 if extend else T), T, None)
    windowed = Call(g, extend, long_.N - T, T, W, caches=(long_.kc, long_.vc))
    windowed.q, windowed.new = long_.q, long_.new
    prefix = W if extend else W - T
    # the short baseline: its own slab, holding the last rows of the long cache (decode: exactly the windowed call's keys)
    short = Call(g, extend, prefix, T, None, caches=tuple(c[:, long_.N - prefix - T:].contiguous() for c in (long_.kc, long_.vc)))
    short.q, short.new = long_.q, long_.new
    sides = {"window": windowed, "short": short, "long": long_, "short_again": short, "long_again": long_}
    res, reps = run(sides, args)
    m = lambda n: res[n]["median_ms"]
    row = {"call": "extend" if extend else "decode", "B": B, "H": H, "Hkv": HKV, "T": T, "window": W, "long_len": long_.N, "short_len": short.N,
           "splits": {n: sides[n].splits() for n in ("window", "short", "long")}, "calls_per_window": reps, **res,
           "window_over_short": round(m("window") / m("short"), 3), "window_over_long": round(m("window") / m("long"), 3),
           "aa_short": round(m("short_again") / m("short"), 3), "aa_long": round(m("long_again") / m("long"), 3)}
    if not extend:
        a, b = windowed(), short()
        torch.cuda.synchronize()
        row["max_abs_diff_window_vs_short"] = float((a[0] - b[0]).abs().max())
        keys = 2 * B * HKV * W * D * 2
        row["window_TBps_on_W_keys"] = round(keys / (m("window") * 1e-3) / 1e12, 2)
    return row


# the README's existing rows, through the unwindowed entry points: (name, extend, B, Hkv, prefix, T)
ROWS = [("decode-B32-H32-Hkv32-len4096", False, 32, 32, 4095, 1), ("decode-B32-H32-Hkv8-len4096", False, 32, 8, 4095, 1),
        ("extend-B8-H32-Hkv8-prefix8192-T512", True, 8, 8, 8192, 512)]


def unwindowed_rows(args):
    """The library's own unwindowed entry points through ctypes, binding only the symbols a build from before the window has too
    (device_ops binds every symbol of the headers, which such a build lacks)."""
    lib = _lib.load(_lib.DECODE_NAME)
    for sym in ("fa_mi355x_decode_workspace_bytes_gqa", "fa_mi355x_fwd_decode_gqa", "fa_mi355x_extend_workspace_bytes",
                "fa_mi355x_fwd_extend_append"):
        getattr(lib, sym).restype, getattr(lib, sym).argtypes = _lib.DECODE_ABI[sym]
    g = torch.Generator(device="cuda").manual_seed(0)
    stream = device_ops._stream_ptr()
    for name, extend, b, hkv, prefix, T in ROWS:
        N = prefix + T
        kc, vc, q = rnd(g, b, N, hkv, D), rnd(g, b, N, hkv, D), rnd(g, b, T, H, D)
        kn, vn = kc[:, prefix:].contiguous(), vc[:, prefix:].contiguous()
        out, lse = torch.empty(q.shape, dtype=torch.float32, device="cuda"), torch.empty((b, H, T), dtype=torch.float32, device="cuda")
        lens = torch.full((b,), N, dtype=torch.int32, device="cuda")
        nbytes = (lib.fa_mi355x_extend_workspace_bytes if extend else lib.fa_mi355x_decode_workspace_bytes_gqa)(b, H, hkv, T, N, D)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device="cuda")
        p = lambda t: t.data_ptr()
        if extend:
            call = lambda: lib.fa_mi355x_fwd_extend_append(p(q), p(kn), p(vn), p(kc), p(vc), p(out), p(lse), p(lens), p(ws), b, H, hkv, T, N, D, D,
                                                           _lib.FA_LAYOUT_BNHD, 0.0, 1, _lib.FA_DTYPE_BF16, stream)
        else:
            call = lambda: lib.fa_mi355x_fwd_decode_gqa(p(q), p(kc), p(vc), p(out), p(lse), p(lens), p(ws), b, H, hkv, T, N, D,
                                                        _lib.FA_LAYOUT_BNHD, 0.0, 1, _lib.FA_DTYPE_BF16, stream)
        assert call() == _lib.FA_OK
        res, reps = run({"first": call, "again": call}, args)
        print(json.dumps({"row": name, "build": "alternate" if "FA_MI355X_KERNEL_DIR" in os.environ else "in-tree", "calls_per_window": reps, **res,
                          "aa": round(res["again"]["median_ms"] / res["first"]["median_ms"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--unwindowed-rows", action="store_true", help="only the README's existing rows, window=None (for tools/ab_dirs.sh)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py measures on the GPU; there is none here")
    if args.unwindowed_rows:
        return unwindowed_rows(args)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "causal": True,
                      "reps": args.reps, "repeats": args.repeats}), flush=True)
    print(json.dumps(measure(False, 1, args)), flush=True)
    print(json.dumps(measure(True, 512, args)), flush=True)


if __name__ == "__main__":
    main()
