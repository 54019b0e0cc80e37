"""MLA prefill (flash_attn_mla_prefill) against what a user has without it (profiles/mla_prefill_bench.txt).

H in {16, 128}; B x P in {1 x 8192, 4 x 4096, 16 x 1024} as causal self-attention, and one chunk of 1024 queries behind 8192 keys.
k_nope and v are the two views of one (Tk, H, 256) buffer, as the model layer passes them.  Baselines:
A  scaled_dot_product_attention on a materialised K = [k_nope | k_pe copied to every head], timed without and with the concatenation
   (causal for the self-attention shapes; the chunk runs it unmasked, which costs it 1 / 0.94 of the admitted work);
B  flash_attn_extend at d = 256 on q, K and V zero-padded to 256 columns (the padding is not timed): what the project offered.
Every figure is the median of WINDOWS timed windows of REPS calls each (HIP events), all candidates of a shape interleaved in one
process, each with an A/A repeat beside it (the same call timed again: the spread a ratio must exceed to mean anything).  TFLOP/s
counts 2 * (192 + 128) flops per admitted (query, key, head) for every candidate, whatever it issues.
Usage: bench_mla_prefill.py [out.txt [H ...]]
       bench_mla_prefill.py backward out.txt     the backward rows (profiles/mla_prefill_bwd_bench.txt), see backward_calls"""
import statistics
import sys

import torch
import torch.nn.functional as F

from flash_attention_minitorch_amd import device_ops as ops

WINDOWS, REPS = 5, 3
SHAPES = [(1, 8192, 8192), (4, 4096, 4096), (16, 1024, 1024), (1, 1024, 8192)]   # (B, n_q, n_k) per sequence


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


def shape_calls(H, B, nq, nk):
    q, kv, k_pe = u(B * nq, H, 192), u(B * nk, H, 256), u(B * nk, 64)
    k_nope, v = kv[..., :128], kv[..., 128:]
    cu_q, cu_k = (torch.arange(B + 1, dtype=torch.int32, device="cuda") * n for n in (nq, nk))
    out, lse = torch.empty(B * nq, H, 128, dtype=torch.float32, device="cuda"), torch.empty(H, B * nq, dtype=torch.float32, device="cuda")
    ws = ops.mla_prefill_workspace(q, k_nope, cu_q)
    calls = {"mla prefill": lambda: ops.flash_attn_mla_prefill(q, k_nope, k_pe, v, cu_q, cu_k, out=out, lse=lse, workspace=ws)}
    cat = lambda: torch.cat([k_nope, k_pe[:, None, :].expand(-1, H, -1)], -1).view(B, nk, H, 192).transpose(1, 2)
    qs, ks, vs = q.view(B, nq, H, 192).transpose(1, 2), cat(), v.reshape(B, nk, H, 128).transpose(1, 2)
    calls["A sdpa"] = lambda: F.scaled_dot_product_attention(qs, ks, vs, is_causal=nq == nk)
    calls["A sdpa + concat"] = lambda: F.scaled_dot_product_attention(qs, cat(), vs, is_causal=nq == nk)
    q256, k256, v256 = F.pad(q, (0, 64)).view(B, nq, H, 256), F.pad(ks.transpose(1, 2), (0, 64)).contiguous(), F.pad(vs.transpose(1, 2), (0, 128)).contiguous()
    lens = torch.full((B,), nk, dtype=torch.int32, device="cuda")
    o256, ws256 = torch.empty(q256.shape, dtype=torch.float32, device="cuda"), ops.extend_workspace(q256, k256)
    calls["B extend d=256 (padded)"] = lambda: ops.flash_attn_extend(q256, k256, v256, lens, softmax_scale=192 ** -0.5, out=o256, workspace=ws256)
    admitted = B * sum(min(nk, i + nk - nq + 1) for i in range(nq))
    return calls, 2 * (192 + 128) * admitted * H


BWD_SHAPES = [(128, 1, 8192, 8192), (16, 1, 4096, 8192), (16, 64, 256, 256)]   # (H, B, n_q, n_k): a prompt, a chunk behind a prefix, many short


def backward_calls(H, B, nq, nk):
    """flash_attn_mla_prefill_bwd against torch autograd's backward over scaled_dot_product_attention on the same operands with k_pe
    expanded to every head (its forward is not timed: the graph is retained).  Five products (S, dP, dV, dK, dQ): TFLOP/s counts
    2 * (3 * 192 + 2 * 128) flops per admitted (query, key, head) for both."""
    q, kv, k_pe = u(B * nq, H, 192), u(B * nk, H, 256), u(B * nk, 64)
    k_nope, v, do = kv[..., :128], kv[..., 128:], u(B * nq, H, 128)
    cu_q, cu_k = (torch.arange(B + 1, dtype=torch.int32, device="cuda") * n for n in (nq, nk))
    out, lse = ops.flash_attn_mla_prefill(q, k_nope, k_pe, v, cu_q, cu_k)
    dkv = torch.empty(kv.shape, dtype=torch.float32, device="cuda")
    grads = (torch.empty(q.shape, dtype=torch.float32, device="cuda"), dkv[..., :128], torch.empty(k_pe.shape, dtype=torch.float32, device="cuda"), dkv[..., 128:])
    ws = ops.mla_prefill_workspace(q, k_nope, cu_q, backward=True)
    calls = {"mla prefill bwd": lambda: ops.flash_attn_mla_prefill_bwd(q, k_nope, k_pe, v, out, do, lse, cu_q, cu_k, workspace=ws, grads=grads)}
    lq, lkv, lp = (t.clone().requires_grad_() for t in (q, kv, k_pe))
    ks = torch.cat([lkv[..., :128], lp[:, None, :].expand(-1, H, -1)], -1).view(B, nk, H, 192).transpose(1, 2)
    mask = None if nq == nk else (torch.arange(nk, device="cuda")[None, :] <= torch.arange(nq, device="cuda")[:, None] + nk - nq)
    o = F.scaled_dot_product_attention(lq.view(B, nq, H, 192).transpose(1, 2), ks, lkv[..., 128:].reshape(B, nk, H, 128).transpose(1, 2),
                                       attn_mask=mask, is_causal=nq == nk)
    go = do.view(B, nq, H, 128).transpose(1, 2)
    calls["autograd over sdpa"] = lambda: torch.autograd.grad(o, (lq, lkv, lp), go, retain_graph=True)
    admitted = B * sum(min(nk, i + nk - nq + 1) for i in range(nq))
    return calls, 2 * (3 * 192 + 2 * 128) * admitted * H


def main_backward(path):
    lines = []
    for H, B, nq, nk in BWD_SHAPES:
        calls, flops = backward_calls(H, B, nq, nk)
        res = compare(calls)
        lines.append(f"backward H={H} B={B} n_q={nq} n_k={nk}: {flops / 1e9:.1f} GFLOP")
        lines += [f"  {n:32s} {ms:9.4f} ms   {flops / ms / 1e9:7.1f} TFLOP/s" for n, ms in res.items()]
        lines.append(f"  mla prefill bwd / autograd over sdpa time ratio {res['mla prefill bwd'] / res['autograd over sdpa']:.3f}")
        print("\n".join(lines[-6:]), flush=True)
        open(path, "w").write("\n".join(lines) + "\n")
        del calls
        torch.cuda.empty_cache()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "backward":   # bench_mla_prefill.py backward out.txt
        return main_backward(sys.argv[2])
    lines = []
    for H in [int(a) for a in sys.argv[2:]] or [16, 128]:
        for B, nq, nk in SHAPES:
            calls, flops = shape_calls(H, B, nq, nk)
            res = compare(calls)
            lines.append(f"H={H} B={B} n_q={nq} n_k={nk}: {flops / 1e9:.1f} GFLOP")
            for n, ms in res.items():
                lines.append(f"  {n:32s} {ms:9.4f} ms   {flops / ms / 1e9:7.1f} TFLOP/s")
            for base in ("A sdpa", "A sdpa + concat", "B extend d=256 (padded)"):
                lines.append(f"  mla prefill / {base} time ratio {res['mla prefill'] / res[base]:.3f}")
            print("\n".join(lines[-12:]), flush=True)
            if len(sys.argv) > 1:
                open(sys.argv[1], "w").write("\n".join(lines) + "\n")
            del calls
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
