"""MLA decode on an fp8 latent cache beside the bf16 call it must equal (profiles/mla_fp8_bench.txt).

The rows of tools/bench_mla.py and tools/bench_mla_sparse.py at B = 32, H in {16, 128}, Nq in {1, 2}, every sequence of length 32768,
slab and 128-row pages; the sparse rows at topk = 2048 (distinct positions drawn at random, unsorted).  The fp8 cache holds random e4m3
codes (no NaN code) under power-of-two scales of 2^-8 .. 2^-10 and U(-1, 1) k_pe; the bf16 cache is that cache dequantised, so both
calls of a pair compute the same thing, and their outputs are compared bit for bit before anything is timed.  Every figure is the median
of WINDOWS timed windows of REPS calls each (HIP events), the candidates of a shape interleaved in one process, each with an A/A repeat
beside it (the same call timed again: the spread a ratio must exceed to mean anything).  TB/s counts the cache bytes a call reads once:
rows * 656 for fp8, rows * 1152 for bf16.  The floor on fp8 / bf16 where the stream is the limit is 656 / 1152 = 0.57."""
import statistics
import sys

import torch

from flash_attention_minitorch_amd import device_ops as ops

WINDOWS, REPS = 5, 10
B, N, TOPK, DQK, DV, ROW, PAGE, SCALE = 32, 32768, 2048, 576, 512, 656, 128, 192 ** -0.5


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPS   # ms per call


def compare(calls):
    """name -> median ms over the windows; every call twice (name, name + " (A/A)"), interleaved window by window."""
    calls = {n: f for name, fn in calls.items() for n, f in ((name, fn), (name + " (A/A)", fn))}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in calls}
    for _ in range(WINDOWS):
        for n, fn in calls.items():
            samples[n].append(timed(fn))
    return {n: statistics.median(s) for n, s in samples.items()}


def caches():
    """(fp8 cache (B, N, 656) uint8, the same cache dequantised to bf16 (B, N, 576)), made on the device."""
    codes = torch.randint(0, 0x7F, (B, N, DV), device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, (B, N, DV), device="cuda", dtype=torch.uint8) << 7)
    scales = torch.ldexp(torch.ones(B, N, 4, device="cuda"), -torch.randint(8, 11, (B, N, 4), device="cuda"))
    pe = (torch.rand(B, N, DQK - DV, device="cuda") * 2 - 1).to(torch.bfloat16)
    fp8 = torch.cat([codes, scales.view(torch.uint8), pe.view(torch.uint8)], -1).contiguous()
    lat = (codes.view(torch.float8_e4m3fn).float().view(B, N, 4, 128) * scales[..., None]).view(B, N, DV).to(torch.bfloat16)
    return fp8, torch.cat([lat, pe], -1).contiguous()


def mla_call(q, kv, lens, table=None, indices=None):
    Bq, Nq, H, _ = q.shape
    ws = ops.mla_workspace(q, kv, table, topk=None if indices is None else indices.shape[-1])
    out, lse = torch.empty(Bq, Nq, H, DV, dtype=torch.float32, device="cuda"), torch.empty(Bq, H, Nq, dtype=torch.float32, device="cuda")
    return lambda: ops.flash_attn_decode_mla(q, kv, lens, SCALE, block_table=table, out=out, lse=lse, workspace=ws, indices=indices)


def shape_calls(H, Nq, fp8, bf16):
    q = (torch.rand(B, Nq, H, DQK, device="cuda") * 2 - 1).to(torch.bfloat16)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    idx = torch.rand(B, Nq, N, device="cuda").argsort(-1)[..., :TOPK].int().contiguous()
    mp = N // PAGE
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    calls = {}
    for kind, indices in (("dense", None), ("sparse", idx)):
        for lay, tb in (("slab", None), ("pages", table)):
            for name, kv in (("bf16", bf16), ("fp8", fp8)):
                calls[f"{kind} {lay} {name}"] = mla_call(q, kv if tb is None else kv.view(B * mp, PAGE, kv.shape[-1]), lens, tb, indices)
            a, b = calls[f"{kind} {lay} bf16"](), calls[f"{kind} {lay} fp8"]()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"{kind} {lay}: the fp8 call differs from the bf16 call"
    return calls


def main():
    lines = []
    fp8, bf16 = caches()
    for H in (16, 128):
        for Nq in (1, 2):
            res = compare(shape_calls(H, Nq, fp8, bf16))
            lines.append(f"B={B} H={H} Nq={Nq} len={N} topk={TOPK}   (each fp8 result bit-equal to its bf16 twin)")
            for n, ms in res.items():
                rows = B * N if n.startswith("dense") else B * Nq * TOPK
                nbytes = rows * (ROW if "fp8" in n else DQK * 2)
                lines.append(f"  {n:28s} {ms:9.4f} ms   {nbytes / ms / 1e9:6.3f} TB/s of cache rows")
            for kind in ("dense slab", "dense pages", "sparse slab", "sparse pages"):
                f, b = res[kind + " fp8"], res[kind + " bf16"]
                lines.append(f"  {kind}: fp8 / bf16 time ratio {f / b:.3f}   (A/A of bf16: {res[kind + ' bf16 (A/A)'] / b:.3f}, of fp8: "
                             f"{res[kind + ' fp8 (A/A)'] / f:.3f})")
            print("\n".join(lines[-21:]), flush=True)
            torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
