"""MLA decode (flash_attn_decode_mla) against what a user has without it (profiles/mla_bench.txt).

B = 32, Nq in {1, 2}, H in {16, 128}, every sequence of the same length in {4096, 32768}, slab and 128-row pages.  Baselines:
A  scaled_dot_product_attention with the H * Nq (query, head) pairs as the rows of one problem per sequence, K = the cache and
   V = cache[..., :512] (nothing is expanded or copied; no causal mask, which only spares it work at Nq = 2);
B  a device copy of as many bytes as the cache rows the call reads: the box's copy rate;
C  flash_attn_decode at d = 128 with Hkv = 1 on K and V caches of the same bytes in all (a reference point, another function).
Every figure is the median of WINDOWS timed windows of REPS calls each (HIP events), all candidates of a shape interleaved in one
process, each with an A/A repeat beside it (the same call timed again: the spread a ratio must exceed to mean anything).  TB/s counts
the cache bytes once; TFLOP/s counts the two products, 2 * B * H * Nq * len * (576 + 512)."""
import statistics
import sys

import torch

from flash_attention_minitorch_amd import device_ops as ops

WINDOWS, REPS = 5, 10
B, DQK, DV, PAGE, SCALE = 32, 576, 512, 128, 192 ** -0.5


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


def u(*shape):
    return (torch.rand(*shape, device="cuda") * 2 - 1).to(torch.bfloat16)


def mla_call(q, kv, lens, table=None):
    Bq, Nq, H, _ = q.shape
    ws = ops.mla_workspace(q, kv, table)
    out, lse = torch.empty(Bq, Nq, H, DV, dtype=torch.float32, device="cuda"), torch.empty(Bq, H, Nq, dtype=torch.float32, device="cuda")
    return lambda: ops.flash_attn_decode_mla(q, kv, lens, SCALE, block_table=table, out=out, lse=lse, workspace=ws)


def shape_calls(H, Nq, N):
    q, kv = u(B, Nq, H, DQK), u(B, N, DQK)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    mp = N // PAGE
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    calls = {"mla slab": mla_call(q, kv, lens), "mla 128-row pages": mla_call(q, kv.view(B * mp, PAGE, DQK), lens, table)}
    qs, ks, vs = q.view(B, 1, Nq * H, DQK), kv.view(B, 1, N, DQK), kv.view(B, 1, N, DQK)[..., :DV]
    calls["A sdpa (heads as rows)"] = lambda: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, scale=SCALE)
    dst = torch.empty_like(kv)
    calls["B device copy"] = lambda: dst.copy_(kv)
    n128 = N * DQK // 256   # rows of a d = 128 K cache and V cache that hold the latent cache's bytes between them
    q128, k128, v128 = u(B, Nq, H, 128), u(B, n128, 1, 128), u(B, n128, 1, 128)
    lens128 = torch.full((B,), n128, dtype=torch.int32, device="cuda")
    ws = ops.decode_workspace(q128, k128)
    o128 = torch.empty(q128.shape, dtype=torch.float32, device="cuda")
    calls["C decode d=128 Hkv=1"] = lambda: ops.flash_attn_decode(q128, k128, v128, lens128, out=o128, workspace=ws)
    return calls, kv.numel() * 2, 2 * B * H * Nq * N * (DQK + DV)


def main():
    lines = []
    for N in (4096, 32768):
        for H in (16, 128):
            for Nq in (1, 2):
                calls, nbytes, flops = shape_calls(H, Nq, N)
                res = compare(calls)
                lines.append(f"B={B} H={H} Nq={Nq} len={N}: {nbytes / 1e6:.0f} MB of cache, {flops / 1e9:.1f} GFLOP")
                for n, ms in res.items():
                    rate = f"{flops / ms / 1e9:7.1f} TFLOP/s" if n[0] in "mA" else ""
                    lines.append(f"  {n:30s} {ms:9.4f} ms   {nbytes / ms / 1e9:6.2f} TB/s of cache   {rate}")
                for base in ("A sdpa (heads as rows)", "B device copy", "C decode d=128 Hkv=1"):
                    lines.append(f"  mla slab / {base[0]} time ratio {res['mla slab'] / res[base]:.3f}")
                print("\n".join(lines[-16:]), flush=True)
                del calls
                torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
