"""Learned sink logits against the same call without them on the MI355X (KV-cache calls, training, the logit gradient): one JSON
line per shape.

Both sides run the same call on the same caches in one process: the call without ``sink_logits`` (the yardstick: the builds that
were there, unchanged) and the call with it (the LSINK builds of the split kernels and of the combine kernel: one load and a few
scalar operations per row where its 1 / l is formed, and as many launches).  The plain side is measured twice, interleaved with the
other (A, lsink, A'), so every row carries its own A/A figure: ``aa`` is median(A') / median(A) and ``plain_spread`` the
(max - min) / median over both.  ``exceeds_spread`` says plainly whether |lsink / plain - 1| is larger than that spread.
Shapes (gpt-oss's attention: bf16, d = 64, [B][N][H][d], B = 32, H = 64, Hkv = 8, causal):
  decode   Nq = 1 at 4096 and at 32768 cached tokens, with a window of 128 and with none, on slabs and on a pool of 128-row pages
           under a randomly permuted table
  extend   512 new tokens (fused append) after a prefix of 8192, with the window and without, on slabs
  train    the training forward (flash_attn_fwd_window_lsink against flash_attn_fwd_window, at W = N with window = N: one kernel
           text with and without the term) and forward + backward (flash_attn_gqa under autograd, with and without
           ``sink_logits=``, the logits requiring grad) at B = 2, N = 4096 and 8192, W = 128 and W = N.  At W = N the plain
           flash_attn_gqa call is what a user makes and runs the CORE library's kernels, another kernel family: that row
           (``plain_family`` "core") compares two paths, and its ratio is not the cost of the sink term
  grad     the two sink_logits_grad launches alone at B = 2, H = 32, N = 8192: GB/s of the bytes they read (out fp32, out_grad bf16,
           lse) beside the rate of a device-to-device copy of as many bytes on the same box
There is no pass mark and no ratio fixed in advance.
Per side: milliseconds per call, device events around a window of calls (at least ``--reps``, and enough of them to fill
``--window-ms`` of device time); ``--repeats`` windows per side, median and min .. max reported.

    python tools/bench_lsink.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/lsink_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops  # noqa: E402

D, PAGE, B, H, HKV, W = 64, 128, 32, 64, 8, 128
TB = 2   # the training rows' batch
# name -> (extend, prefix, T, paged, window)
SHAPES = {}
for _n in (4096, 32768):
    for _w in (W, None):
        for _paged in (False, True):
            SHAPES[f"decode-len{_n}-{'W128' if _w else 'full'}-{'paged' if _paged else 'slab'}"] = (False, _n - 1, 1, _paged, _w)
for _w in (W, None):
    SHAPES[f"extend-prefix8192-T512-{'W128' if _w else 'full'}-slab"] = (True, 8192, 512, False, _w)


TRAIN = {f"train-{'fwd+bwd' if _b else 'fwd'}-N{_n}-{'W128' if _w else 'full'}": (_n, _w, _b)
         for _n in (4096, 8192) for _w in (W, None) for _b in (False, True)}


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
    """One shape: bf16 caches (B, N, Hkv, D) with N = prefix + T (or the pool that holds them), the T new tokens' q, their k, v for
    the fused extend call, and one logit per query head in U(-1, 3)."""

    def __init__(self, extend, prefix, T, paged, window, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.T, self.N, self.extend = T, prefix + T, extend
        kc, vc = rnd(B, self.N, HKV, D), rnd(B, self.N, HKV, D)
        self.q = rnd(B, T, H, D)
        self.logits = torch.rand(H, generator=g, device="cuda").mul_(4).sub_(1)
        self.new = dict(k_new=kc[:, prefix:].contiguous(), v_new=vc[:, prefix:].contiguous()) if extend else {}
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.where = {} if window is None else dict(window=window)
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
            self.where["block_table"] = table
        self.caches = (kc, vc)
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        self.ws = (device_ops.extend_workspace if extend else device_ops.decode_workspace)(self.q, kc, **self.where)

    def plain(self):
        return self.fn(self.q, *self.caches, self.lens, causal=True, workspace=self.ws, **self.new, **self.where)

    def lsink(self):
        return self.fn(self.q, *self.caches, self.lens, causal=True, workspace=self.ws, sink_logits=self.logits, **self.new, **self.where)


class TrainCase:
    """The training forward (``backward`` False) or forward + backward at B = 2, N tokens, a window of W (None: W = N)."""

    def __init__(self, N, window, backward, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(s, generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.q, self.k, self.v, self.do = rnd(TB, N, H, D), rnd(TB, N, HKV, D), rnd(TB, N, HKV, D), rnd(TB, N, H, D).float()
        self.logits = torch.rand(H, generator=g, device="cuda").mul_(4).sub_(1)
        self.N, self.window, self.backward = N, window, backward
        if backward:
            for t in (self.q, self.k, self.v, self.logits):
                t.requires_grad_()

    def _run(self, logits):
        if not self.backward:
            if logits is not None:
                return device_ops.flash_attn_fwd_window_lsink(self.q, self.k, self.v, self.window or self.N, logits)
            return device_ops.flash_attn_fwd_window(self.q, self.k, self.v, self.window or self.N)
        for t in (self.q, self.k, self.v, self.logits):
            t.grad = None
        device_ops.flash_attn_gqa(self.q, self.k, self.v, True, None, "bnhd", self.window, sink_logits=logits).backward(self.do)

    def plain(self):
        return self._run(None)

    def lsink(self):
        return self._run(self.logits)


def grad_row(args):
    """The sink_logits_grad launches alone, and a copy of as many bytes as they read."""
    Bg, Hg, Ng = 2, 32, 8192
    g = torch.Generator(device="cuda").manual_seed(0)
    out = torch.rand((Bg, Ng, Hg, D), generator=g, device="cuda")
    dout = torch.rand((Bg, Ng, Hg, D), generator=g, device="cuda").to(torch.bfloat16)
    lse = torch.rand((Bg, Hg, Ng), generator=g, device="cuda")
    logits = torch.rand(Hg, generator=g, device="cuda")
    ws = device_ops.lsink_workspace(dout)
    nbytes = out.numel() * 4 + dout.numel() * 2 + lse.numel() * 4
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    fn, cp = (lambda: device_ops.sink_logits_grad(out, dout, lse, logits, workspace=ws)), (lambda: dst.copy_(src))
    reps = max(args.reps, int(args.window_ms / window_ms(fn, 5, args.warmup)) + 1)
    xs = {"grad": [], "copy": []}
    for i in range(args.repeats):
        for side, f in (("grad", fn), ("copy", cp)):
            xs[side].append(window_ms(f, reps, args.warmup if i == 0 else 1))
    row = {"shape": f"sink_logits_grad-B{Bg}-H{Hg}-N{Ng}-d{D}", "calls_per_window": reps, "bytes_read": nbytes,
           "workgroups": Hg * ((Bg * Ng + 511) // 512)}
    row.update({s: stats(x) for s, x in xs.items()})
    row["grad_gbps"] = round(nbytes / row["grad"]["median_ms"] / 1e6, 1)
    row["copy_gbps_read"] = round(nbytes / row["copy"]["median_ms"] / 1e6, 1)   # (the copy also WRITES as many bytes)
    return row


def measure(name, case, args):
    a, b = case.plain, case.lsink
    a(), b()
    torch.cuda.synchronize()
    reps = max(args.reps, int(args.window_ms / window_ms(a, 5, args.warmup)) + 1)
    xs = {"plain": [], "lsink": [], "plain_again": []}
    for i in range(args.repeats):   # A, lsink, A': window by window
        for side, fn in (("plain", a), ("lsink", b), ("plain_again", a)):
            xs[side].append(window_ms(fn, reps, args.warmup if i == 0 else 1))
    row = {"shape": name, "calls_per_window": reps}
    row.update({s: stats(x) for s, x in xs.items()})
    base = row["plain"]["median_ms"]
    both = xs["plain"] + xs["plain_again"]
    row["aa"] = round(row["plain_again"]["median_ms"] / base, 3)
    row["plain_spread"] = round((max(both) - min(both)) / statistics.median(both), 3)
    row["lsink_over_plain"] = round(row["lsink"]["median_ms"] / base, 3)
    row["exceeds_spread"] = abs(row["lsink_over_plain"] - 1.0) > row["plain_spread"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    ap.add_argument("--shape", nargs="+", default=list(SHAPES) + list(TRAIN) + ["grad"], choices=list(SHAPES) + list(TRAIN) + ["grad"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsink.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "B": B, "H": H, "Hkv": HKV, "layout": "bnhd",
                      "causal": True, "page_size": PAGE, "window": W, "reps": args.reps, "repeats": args.repeats}), flush=True)
    for name in args.shape:
        if name == "grad":
            print(json.dumps(grad_row(args)), flush=True)
            continue
        if name in TRAIN:
            case = TrainCase(*TRAIN[name])
            row = measure(name, case, args)
            row["plain_family"] = "core" if case.backward and not case.window else "window"
            print(json.dumps(row), flush=True)
            del case
            torch.cuda.empty_cache()
            continue
        extend, prefix, T, paged, window = SHAPES[name]
        case = Case(extend, prefix, T, paged, window)
        row = measure(name, case, args)
        splits = _lib.decode().fa_mi355x_extend_window_splits if extend else _lib.decode().fa_mi355x_decode_window_splits
        row["splits"] = splits(B, H, HKV, T, case.N, D, 1, window or 0)
        print(json.dumps(row), flush=True)
        del case
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
