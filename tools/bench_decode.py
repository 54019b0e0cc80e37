"""KV-cache decode (fa_mi355x_fwd_decode / fa_mi355x_fwd_decode_gqa) on the MI355X: one JSON line per shape.

Per shape: microseconds per decode call (device events around `--reps` calls after `--warmup`), the K+V bytes one call must read
(B * Hkv * len * d * 2 * element size, Hkv = the cache's heads), GB/s and the share of the 6.3 TB/s measured copy rate and of the 8 TB/s spec.  The calls rotate
over enough distinct caches that the bytes touched exceed 512 MB, so the 256 MB Infinity Cache does not serve repeated calls.
Beside it, on the same data:
  (a) what a user does without decode: the existing causal forward on [B][N][H][d] (device_ops.flash_attn_fwd_bnhd, the library's
      default guarded call) over all len tokens, of which the caller keeps the last Nq rows;
  (b) torch.nn.functional.scaled_dot_product_attention on the cache slice ([B][H][len][d]); no mask (for Nq = 1 the same function).
A grouped shape (Hkv < H: G = H / Hkv query heads share a cache head) is also timed against the two calls that bracket it:
  (x) the same q on the cache expanded to H heads (repeat_interleave: all a user can do without grouped decode; G x the bytes);
  (y) an ungrouped call with H = Hkv heads: the same K / V stream with 1/G of the queries (the floor the bytes set).
Then the in-model numbers: one attention_stack_step of a 4-layer stack, the same step with the append inside the library
(attention_stack_step_fused), eager and captured in a graph (GraphedStep), against re-running attention_stack over the whole prefix, and the step of a 32-head stack with 8 kv heads against the same stack with 32; and the
append launch alone (decode_append: the new token's k and v into the caches, the launch the step's fused call starts with).

    python tools/bench_decode.py [--reps 50] [--warmup 5] [--only decode|grouped|model] > decode.txt
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops, modules_transformer as mt  # noqa: E402

COPY_TBS, SPEC_TBS = 6.3, 8.0
ROTATE_BYTES = 512 << 20

# (dtype, B, H, Nq, len, d[, Hkv = H])
SHAPES = [
    ("bf16", 1, 8, 1, 4096, 128), ("bf16", 1, 8, 1, 16384, 128), ("bf16", 1, 8, 1, 65536, 128), ("bf16", 32, 32, 1, 4096, 128),
    ("f32", 8, 8, 1, 4096, 64),
    ("f32", 8, 8, 1, 1024, 32), ("bf16", 8, 8, 1, 1024, 32),
    ("bf16", 8, 8, 4, 4096, 128), ("bf16", 8, 8, 64, 4096, 128),
]
GROUPED_SHAPES = [
    ("bf16", 32, 32, 1, 4096, 128, 8), ("bf16", 32, 32, 1, 4096, 128, 1), ("bf16", 1, 32, 1, 4096, 128, 8),
    ("f32", 8, 8, 1, 4096, 64, 2), ("bf16", 8, 32, 4, 4096, 128, 8),
]
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def timed_us(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _rotation(kv_bytes):
    return max(1, math.ceil(ROTATE_BYTES / kv_bytes) + 1) if kv_bytes < ROTATE_BYTES else 1


def _decode_us(q, caches, n, reps, warmup):
    """us per flash_attn_decode call of q against the caches in rotation (caller-owned out, lse, workspace: no allocation timed)."""
    B, Nq, H, _ = q.shape
    lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
    out = torch.empty(q.shape, dtype=torch.float32, device="cuda")
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device="cuda")
    ws = device_ops.decode_workspace(q, caches[0][0])

    def dec(i):
        k, v = caches[i % len(caches)]
        device_ops.flash_attn_decode(q, k, v, lens, causal=True, out=out, lse=lse, workspace=ws)

    return timed_us(dec, reps, warmup)


def bench_shape(dtype, B, H, Nq, n, d, Hkv=None, reps=50, warmup=5, only="all"):
    dt = DT[dtype]
    Hkv = Hkv or H
    G = H // Hkv
    esz = torch.tensor([], dtype=dt).element_size()
    kv_bytes = B * Hkv * n * d * 2 * esz
    ncache = _rotation(kv_bytes)
    gen = torch.Generator(device="cuda").manual_seed(0)
    u = lambda *s: (torch.rand(*s, device="cuda", generator=gen) * 2 - 1).to(dt)
    caches = [(u(B, n, Hkv, d), u(B, n, Hkv, d)) for _ in range(ncache)]
    q = u(B, Nq, H, d)
    code = 1 if dtype == "bf16" else 0
    lib = _lib.decode()
    splits = lib.fa_mi355x_decode_splits(B, H, Nq, n, d, code) if G == 1 else lib.fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, n, d, code)
    us = _decode_us(q, caches, n, reps, warmup)
    rec = {"shape": f"B={B} H={H} Nq={Nq} len={n} d={d} {dtype}", "dtype": dtype, "B": B, "H": H, "Nq": Nq, "len": n, "d": d,
           "splits": splits, "caches_rotated": ncache, "decode_us": round(us, 2), "kv_bytes": kv_bytes,
           "GB_s": round(kv_bytes / us / 1e3, 1), "of_copy_6.3TBs": round(kv_bytes / us / 1e6 / COPY_TBS, 3),
           "of_spec_8TBs": round(kv_bytes / us / 1e6 / SPEC_TBS, 3)}
    if G > 1:
        rec["shape"] = f"B={B} H={H} Hkv={Hkv} Nq={Nq} len={n} d={d} {dtype}"
        rec["Hkv"] = Hkv
        # (y) first, on the same caches; then (x) on expanded copies, as many as its own bytes need to get past the Infinity Cache
        y_us = _decode_us(q[:, :, ::G].contiguous(), caches, n, reps, warmup)
        nx = min(ncache, _rotation(kv_bytes * G))
        expanded = [tuple(t.repeat_interleave(G, dim=2) for t in caches[i]) for i in range(nx)]
        x_us = _decode_us(q, expanded, n, reps, warmup)
        del expanded
        rec.update(x_expanded_cache_us=round(x_us, 2), x_splits=lib.fa_mi355x_decode_splits(B, H, Nq, n, d, code),
                   x_caches_rotated=nx, y_ungrouped_hkv_heads_us=round(y_us, 2),
                   y_splits=lib.fa_mi355x_decode_splits(B, Hkv, Nq, n, d, code),
                   speedup_vs_x=round(x_us / us, 2), over_y=round(us / y_us, 3))
    if only != "decode" and G == 1:
        k, v = caches[0]
        qfull = u(B, n, H, d)
        qfull[:, n - Nq:] = q

        def prefill(i):
            device_ops.flash_attn_fwd_bnhd(qfull, k, v, True, _lib.FA_VARIANT_FA2)

        r = max(3, reps // 10)
        rec["a_full_causal_fwd_us"] = round(timed_us(prefill, r, 2), 2)
        qs, ks, vs = (t.transpose(1, 2).contiguous() for t in (q, k, v))
        sdpa = lambda i: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs)
        rec["b_torch_sdpa_us"] = round(timed_us(sdpa, r, 2), 2)
        rec["speedup_vs_a"] = round(rec["a_full_causal_fwd_us"] / us, 2)
        rec["speedup_vs_b"] = round(rec["b_torch_sdpa_us"] / us, 2)
    del caches
    torch.cuda.empty_cache()
    return rec


def bench_append(dtype, B, Hkv, Nq, Ncap, d, reps, warmup):
    """us per decode_append call: Nq new tokens of B * Hkv heads into caches of Ncap rows, at lengths that differ per batch element."""
    dt = DT[dtype]
    gen = torch.Generator(device="cuda").manual_seed(2)
    u = lambda *s: (torch.rand(*s, device="cuda", generator=gen) * 2 - 1).to(dt)
    kc, vc, kn, vn = u(B, Ncap, Hkv, d), u(B, Ncap, Hkv, d), u(B, Nq, Hkv, d), u(B, Nq, Hkv, d)
    lens = (torch.arange(B, dtype=torch.int32, device="cuda") * 97) % (Ncap - Nq) + Nq
    us = timed_us(lambda i: device_ops.decode_append(kn, vn, kc, vc, lens), reps, warmup)
    return {"append": f"B={B} Hkv={Hkv} Nq={Nq} Ncap={Ncap} d={d} {dtype}", "append_us": round(us, 2),
            "bytes_written": 2 * kn.numel() * kn.element_size()}


def bench_stack(dtype, B, E, H, prefix, reps, warmup, layers_n=4, Hkv=None, full=True, graphed=False):
    dt = DT[dtype]
    Hkv = Hkv or H
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = lambda *s: (torch.rand(*s, device="cuda", generator=gen) * 2 - 1)
    kv_cols = Hkv * (E // H)
    layers = [tuple((u(E, c) / math.sqrt(E)).to(dt) for c in (E, kv_cols, kv_cols, E)) for _ in range(layers_n)]
    x = u(B, prefix + 1, E).to(dt)
    cache = mt.KVCache(layers_n, B, prefix + (3 if graphed else 1) * (warmup + reps) + 8, H, E // H, dt, "cuda", n_kv_head=Hkv)
    mt.attention_stack_prefill(x[:, :prefix].contiguous(), layers, H, cache)
    xs = x[:, prefix:].contiguous()
    step = timed_us(lambda i: mt.attention_stack_step(xs, layers, H, cache), reps, warmup)
    rec = {"stack": f"{layers_n}-layer B={B} E={E} H={H} Hkv={Hkv} prefix={prefix} {dtype}", "step_us": round(step, 1)}
    if graphed:   # the fused step, eager and replayed from a graph, on the same cache (each goes on from where the last one stopped)
        fus = timed_us(lambda i: mt.attention_stack_step_fused(xs, layers, H, cache), reps, warmup)
        g = mt.GraphedStep(layers, H, cache, 1)
        gus = timed_us(lambda i: g.step(xs), reps, warmup)
        rec.update(fused_step_us=round(fus, 1), graphed_step_us=round(gus, 1), fused_vs_step=round(step / fus, 2),
                   graphed_vs_fused=round(fus / gus, 2))
    if full:
        full_us = timed_us(lambda i: mt.attention_stack(x, layers, H, causal=True), max(3, reps // 5), 2)
        rec.update(full_prefix_us=round(full_us, 1), speedup=round(full_us / step, 2))
        if graphed:
            rec.update(fused_speedup=round(full_us / fus, 2), graphed_speedup=round(full_us / gus, 2))
    del cache
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["all", "decode", "ungrouped", "grouped", "model"], default="all",
                    help="decode: the decode timings alone, without the comparisons (a) and (b) (for a trace run); ungrouped: the nine "
                         "Hkv = H shapes alone (build-against-build comparisons); grouped: the Hkv < H shapes and the grouped stack; "
                         "model: the model steps (plain, fused and graphed) and the append launch alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py needs a GPU")
    only = "decode" if args.only in ("ungrouped", "grouped") else args.only
    shapes = [] if args.only == "model" else (SHAPES if args.only != "grouped" else []) + (GROUPED_SHAPES if args.only != "ungrouped" else [])
    for s in shapes:
        print(json.dumps(bench_shape(*s, reps=args.reps, warmup=args.warmup, only=only)), flush=True)
    if args.only in ("all", "grouped", "model"):
        for hkv in (8, 32):
            print(json.dumps(bench_stack("bf16", 8, 4096, 32, 8192, args.reps, args.warmup, Hkv=hkv, full=False, graphed=True)), flush=True)
    if args.only in ("all", "model"):
        for dtype, B, E, H, prefix in (("bf16", 8, 256, 8, 1024), ("f32", 8, 256, 8, 1024), ("bf16", 1, 1024, 8, 8192)):
            print(json.dumps(bench_stack(dtype, B, E, H, prefix, args.reps, args.warmup, graphed=True)), flush=True)
        print(json.dumps(bench_append("bf16", 32, 8, 1, 4096, 128, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
