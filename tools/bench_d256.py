"""Head dim 256 against the d = 128 calls that stream the same cache bytes (profiles/d256_bench.txt).

Decode: Nq = 1, B = 32, H = 32, Hkv = 8; d = 256 at length 2048 against d = 128 at length 4096, slab and 256-row pages, and against
scaled_dot_product_attention on the gathered cache.  Extend: 512 tokens after an 8192 prefix against d = 128 after 16384.  Every figure
is the median of WINDOWS timed windows of REPS calls each (HIP events), all candidates interleaved in one process, each with an A/A
repeat beside it (the same call timed again: the spread a ratio must exceed to mean anything)."""
import statistics
import sys

import torch

from flash_attention_minitorch_amd import device_ops as ops

WINDOWS, REPS = 9, 20


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPS * 1e3   # us per call


def compare(calls):
    """name -> median us over the windows; every call twice (name, name + " (A/A)"), interleaved window by window."""
    calls = {n: f for name, fn in calls.items() for n, f in ((name, fn), (name + " (A/A)", fn))}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in calls}
    for _ in range(WINDOWS):
        for n, fn in calls.items():
            samples[n].append(timed(fn))
    return {n: statistics.median(s) for n, s in samples.items()}


def cache(B, N, Hkv, d, page=None):
    u = lambda *s: (torch.rand(*s, device="cuda") * 2 - 1).to(torch.bfloat16)
    if page is None:
        return u(B, N, Hkv, d), u(B, N, Hkv, d), None
    mp = N // page
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    return u(B * mp, page, Hkv, d), u(B * mp, page, Hkv, d), table


def decode_case(B, H, Hkv, N, d, page):
    k, v, table = cache(B, N, Hkv, d, page)
    q = (torch.rand(B, 1, H, d, device="cuda") * 2 - 1).to(torch.bfloat16)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    ws = ops.decode_workspace(q, k, block_table=table)
    out, lse = torch.empty(q.shape, dtype=torch.float32, device="cuda"), torch.empty(B, H, 1, dtype=torch.float32, device="cuda")
    return (lambda: ops.flash_attn_decode(q, k, v, lens, out=out, lse=lse, workspace=ws, block_table=table)), 2 * k.numel() * 2, (q, k, v)


def main():
    B, H, Hkv = 32, 32, 8
    lines = []
    for page in (None, 256):
        f256, bytes256, (q, k, v) = decode_case(B, H, Hkv, 2048, 256, page)
        f128, bytes128, _ = decode_case(B, H, Hkv, 4096, 128, page)
        calls = {"d=256 len 2048": f256, "d=128 len 4096": f128}
        if page is None:
            # (one query per head: the G heads of a kv head are the rows of one sdpa problem, so the cache is not expanded)
            qs, ks, vs = q.view(B, Hkv, H // Hkv, 256), k.transpose(1, 2), v.transpose(1, 2)
            calls["sdpa d=256 (gathered)"] = lambda: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs)
        res = compare(calls)
        lines.append(f"decode Nq=1 B={B} H={H} Hkv={Hkv} {'slab' if page is None else f'{page}-row pages'}")
        for n, us in res.items():
            nbytes = bytes128 if "128" in n else bytes256
            lines.append(f"  {n:28s} {us:9.1f} us   {nbytes / us / 1e6:6.2f} TB/s of cache")
        lines.append(f"  d=256 / d=128 time ratio {res['d=256 len 2048'] / res['d=128 len 4096']:.3f}")
    res = {}
    calls = {}
    for d, prefix in ((256, 8192), (128, 16384)):
        k, v, _ = cache(1, prefix + 512, Hkv, d)
        q = (torch.rand(1, 512, H, d, device="cuda") * 2 - 1).to(torch.bfloat16)
        ws = ops.extend_workspace(q, k)
        calls[f"extend d={d} 512 after {prefix}"] = (lambda q=q, k=k, v=v, ws=ws: ops.flash_attn_extend(q, k, v, workspace=ws))
    res = compare(calls)
    lines.append(f"extend B=1 H={H} Hkv={Hkv}, 512 tokens")
    for n, us in res.items():
        d, prefix = (256, 8192) if "256" in n else (128, 16384)
        units = 512 * H * (prefix + 256) * d   # (query, key, column) units under the causal mask
        lines.append(f"  {n:34s} {us:9.1f} us   {us * 1e6 / units:7.4f} ps per (query, key, column)")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
