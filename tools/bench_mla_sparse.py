"""Sparse MLA decode (flash_attn_decode_mla(indices=), DeepSeek-V3.2 DSA) against what a DSA model costs without it
(profiles/mla_sparse_bench.txt).

B = 32, H in {16, 128}, Nq in {1, 2}, every sequence of length 32768, topk = 2048, slab and 128-row pages; each query token's list
is 2048 distinct positions drawn at random from the whole sequence, unsorted.  Baselines, both the dense kernel:
a  flash_attn_decode_mla over the whole cache at length 32768: what a DSA model costs today, the number to beat;
b  flash_attn_decode_mla at length 2048: as many rows, but contiguous and shared by both query tokens: a floor a gather cannot beat.
Every figure is the median of WINDOWS timed windows of REPS calls each (HIP events), all candidates of a shape interleaved in one
process, each with an A/A repeat beside it (the same call timed again: the spread a ratio must exceed to mean anything).  GB/s counts
the rows the sparse call gathers, B * Nq * topk * 1152 bytes, over each candidate's time."""
import statistics
import sys

import torch

from flash_attention_minitorch_amd import device_ops as ops

WINDOWS, REPS = 5, 10
B, N, TOPK, DQK, DV, PAGE, SCALE = 32, 32768, 2048, 576, 512, 128, 192 ** -0.5


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


def mla_call(q, kv, lens, table=None, indices=None):
    Bq, Nq, H, _ = q.shape
    ws = ops.mla_workspace(q, kv, table, topk=None if indices is None else indices.shape[-1])
    out, lse = torch.empty(Bq, Nq, H, DV, dtype=torch.float32, device="cuda"), torch.empty(Bq, H, Nq, dtype=torch.float32, device="cuda")
    return lambda: ops.flash_attn_decode_mla(q, kv, lens, SCALE, block_table=table, out=out, lse=lse, workspace=ws, indices=indices)


def shape_calls(H, Nq):
    u = lambda *shape: (torch.rand(*shape, device="cuda") * 2 - 1).to(torch.bfloat16)
    q, kv = u(B, Nq, H, DQK), u(B, N, DQK)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    idx = torch.rand(B, Nq, N, device="cuda").argsort(-1)[..., :TOPK].int().contiguous()   # distinct positions, unsorted
    mp = N // PAGE
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    short = torch.full((B,), TOPK, dtype=torch.int32, device="cuda")
    return {"sparse slab": mla_call(q, kv, lens, indices=idx),
            "sparse 128-row pages": mla_call(q, kv.view(B * mp, PAGE, DQK), lens, table, idx),
            "a dense, length 32768": mla_call(q, kv, lens),
            "b dense, length 2048": mla_call(q, kv[:, :TOPK].contiguous(), short)}


def main():
    lines = []
    for H in (16, 128):
        for Nq in (1, 2):
            res = compare(shape_calls(H, Nq))
            nbytes = B * Nq * TOPK * DQK * 2
            lines.append(f"B={B} H={H} Nq={Nq} len={N} topk={TOPK}: {nbytes / 1e6:.0f} MB of gathered rows")
            for n, ms in res.items():
                lines.append(f"  {n:32s} {ms:9.4f} ms   {nbytes / ms / 1e6:8.1f} GB/s of gathered rows")
            for kind in ("sparse slab", "sparse 128-row pages"):
                for base in ("a dense, length 32768", "b dense, length 2048"):
                    lines.append(f"  {kind} / {base[0]} time ratio {res[kind] / res[base]:.3f}   (A/A of {base[0]}: "
                                 f"{res[base + ' (A/A)'] / res[base]:.3f})")
            print("\n".join(lines[-13:]), flush=True)
            torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
