"""The lightning indexer (device_ops.mla_indexer, DeepSeek-V3.2 DSA) against the torch ops a model would use without it, and the
indexer + sparse attention against the dense MLA call it replaces (profiles/mla_indexer_bench.txt).

B = 32, HI = 64, topk = 2048, every sequence of length 4096 or 32768, Nq in {1, 2}, slab and 128-row pages; attention at H = 128.
Candidates of a shape, interleaved in one process: the score launch, the top-k launch and the fused call (separate calls, so their
sum shows what the fused call saves); a device copy of the index-key bytes (the streaming rate the score launch is measured by);
the torch indexer on the same tensors (einsum -> relu -> weighted sum -> causal mask -> torch.topk); indexer + sparse attention
and the dense MLA call over the whole cache.  Every figure is the median of WINDOWS timed windows of REPS calls each (HIP events),
each with an A/A repeat beside it (the same call timed again: the spread a ratio must exceed to mean anything).

`--fp8 [file]`: the fp8 index keys (144-byte rows; profiles/mla_indexer_fp8_bench.txt) at the same shapes: the score launch slab and
paged, the append and the fused call, each beside the bf16 call on the same keys, interleaved in the same run."""
import sys

import torch

from bench_mla_sparse import B, DQK, PAGE, TOPK, compare, mla_call
from flash_attention_minitorch_amd import device_ops as ops

HI, DI, H = 64, 128, 128


def shape_calls(N, Nq):
    u = lambda *shape: (torch.rand(*shape, device="cuda") * 2 - 1).to(torch.bfloat16)
    q_idx, kidx, w = u(B, Nq, HI, DI), u(B, N, DI), torch.rand(B, Nq, HI, device="cuda") * 2 - 1
    q, kv = u(B, Nq, H, DQK), u(B, N, DQK)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    mp = N // PAGE
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    scores = torch.empty(B, Nq, N, dtype=torch.float32, device="cuda")
    idx = torch.empty(B, Nq, TOPK, dtype=torch.int32, device="cuda")
    copy_dst = torch.empty_like(kidx)
    pos = torch.arange(N, device="cuda")[None, None, :] > (N - Nq + torch.arange(Nq, device="cuda"))[None, :, None]
    ops.mla_index_scores(q_idx, w, kidx, lens, scores=scores)

    def torch_indexer():
        s = torch.einsum("bihc,bsc->bihs", q_idx, kidx).float().relu_()
        s = torch.einsum("bih,bihs->bis", w, s).masked_fill_(pos, float("-inf"))
        return s.topk(TOPK, -1).indices.int()

    sparse, dense = mla_call(q, kv, lens, indices=idx), mla_call(q, kv, lens)
    indexer = lambda: ops.mla_indexer(q_idx, w, kidx, lens, TOPK, scores=scores, indices=idx)
    return {"scores slab": lambda: ops.mla_index_scores(q_idx, w, kidx, lens, scores=scores),
            "scores 128-row pages": lambda: ops.mla_index_scores(q_idx, w, kidx.view(B * mp, PAGE, DI), lens, block_table=table, scores=scores),
            "copy of the index keys": lambda: copy_dst.copy_(kidx),
            "top-k": lambda: ops.mla_index_topk(scores, lens, TOPK, indices=idx),
            "indexer (fused call)": indexer,
            "torch indexer": torch_indexer,
            "indexer + sparse attention": lambda: (indexer(), sparse()),
            "dense MLA attention": dense}


def fp8_shape_calls(N, Nq):
    """name -> (bf16 call, fp8 call) on the same keys; the fp8 cache is filled by the quantising append, 128 rows a call."""
    u = lambda *shape: (torch.rand(*shape, device="cuda") * 2 - 1).to(torch.bfloat16)
    q_idx, kidx, w, new = u(B, Nq, HI, DI), u(B, N, DI), torch.rand(B, Nq, HI, device="cuda") * 2 - 1, u(B, Nq, DI)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    k8 = torch.zeros(B, N, ops._IDX_FP8_ROW, dtype=torch.uint8, device="cuda")
    for s in range(0, N, 128):
        ops.mla_index_append(kidx[:, s:s + 128].contiguous(), k8, torch.full_like(lens, s + 128))
    mp = N // PAGE
    table = torch.randperm(B * mp, device="cuda").reshape(B, mp).int()
    scores = torch.empty(B, Nq, N, dtype=torch.float32, device="cuda")
    idx = torch.empty(B, Nq, TOPK, dtype=torch.int32, device="cuda")
    both = lambda make: (make(kidx), make(k8))
    return {"scores slab": both(lambda k: lambda: ops.mla_index_scores(q_idx, w, k, lens, scores=scores)),
            "scores 128-row pages": both(lambda k: lambda: ops.mla_index_scores(q_idx, w, k.view(B * mp, PAGE, k.shape[-1]), lens,
                                                                                block_table=table, scores=scores)),
            "append": both(lambda k: lambda: ops.mla_index_append(new, k, lens)),
            "indexer (fused call)": both(lambda k: lambda: ops.mla_indexer(q_idx, w, k, lens, TOPK, kidx_new=new, scores=scores, indices=idx))}


def fp8_main(path):
    lines = []
    for N in (4096, 32768):
        for Nq in (1, 2):
            pairs = fp8_shape_calls(N, Nq)
            res = compare({f"{n} {kind}": fn for n, fns in pairs.items() for kind, fn in zip(("bf16", "fp8"), fns)})
            first = len(lines)
            lines.append(f"B={B} HI={HI} Nq={Nq} len={N} topk={TOPK}: index keys {B * N * DI * 2 / 1e6:.0f} MB bf16, {B * N * 144 / 1e6:.0f} MB fp8")
            for n in pairs:
                a, b = res[n + " bf16"], res[n + " fp8"]
                rate = f"   {B * N * 144 / b / 1e9:5.2f} TB/s of fp8 rows" if n.startswith("scores") else ""
                lines.append(f"  {n:22s} bf16 {a:8.4f} ms   fp8 {b:8.4f} ms   fp8 / bf16 {b / a:.3f}   (A/A: bf16 "
                             f"{res[n + ' bf16 (A/A)'] / a:.3f}, fp8 {res[n + ' fp8 (A/A)'] / b:.3f}){rate}")
            print("\n".join(lines[first:]), flush=True)
            torch.cuda.empty_cache()
    if path:
        open(path, "w").write("\n".join(lines) + "\n")


def main():
    if sys.argv[1:2] == ["--fp8"]:
        return fp8_main(sys.argv[2] if len(sys.argv) > 2 else None)
    lines = []
    for N in (4096, 32768):
        for Nq in (1, 2):
            res = compare(shape_calls(N, Nq))
            nbytes = B * N * DI * 2
            lines.append(f"B={B} HI={HI} Nq={Nq} len={N} topk={TOPK} H={H}: {nbytes / 1e6:.0f} MB of index keys")
            for n, ms in res.items():
                rate = f"   {nbytes / ms / 1e9:6.2f} TB/s of index keys" if n.startswith(("scores", "copy")) else ""
                lines.append(f"  {n:36s} {ms:9.4f} ms{rate}")
            first = len(lines)
            for a, b in (("scores slab", "copy of the index keys"), ("indexer (fused call)", "torch indexer"),
                         ("indexer + sparse attention", "dense MLA attention")):
                lines.append(f"  {a} / {b} time ratio {res[a] / res[b]:.3f}   (A/A of the latter: {res[b + ' (A/A)'] / res[b]:.3f})")
            print("\n".join(lines[first - len(res) - 1:]), flush=True)
            torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
