"""MLA prefill backward on the GPU (csrc/fa_mla_prefill_bwd.h): flash_attn_mla_prefill_bwd against the fp64 autograd reference of
tests/test_mla_prefill_bwd_cpu.py on the packed batches of tests/test_mla_prefill_cpu.py (inputs and dout U(-1, 1) in bf16, scale
192^-1/2; max-abs 1e-3 on dq, dk_nope and dv, H x 1e-3 on dk_pe, a sum of H per-head gradients), the bit-for-bit laws, and
flash_attn_mla_prefill_train under autograd."""
import pytest
import torch

from test_gpu_decode import TOL
from test_mla_prefill_bwd_cpu import H_GROUPS, out_grad, reference_grads
from test_mla_prefill_cpu import expected, inputs

pytestmark = pytest.mark.gpu


def backward(q, kv, k_pe, cu_q, cu_k, do, in_place=True):
    """Forward, then backward; dk_nope and dv through the two views of one (Tk, H, 256) buffer (``in_place``) or contiguous.  Returns
    dq, dkv (Tk, H, 256) = dk_nope | dv, dk_pe on the host."""
    from flash_attention_minitorch_amd import device_ops as ops
    q, kv, k_pe, cu_q, cu_k, do = (t.cuda() for t in (q, kv, k_pe, cu_q, cu_k, do))
    k_nope, v = kv[..., :128], kv[..., 128:]
    out, lse = ops.flash_attn_mla_prefill(q, k_nope, k_pe, v, cu_q, cu_k)
    dkv = torch.full(kv.shape, float("nan"), device="cuda")
    views = (dkv[..., :128], dkv[..., 128:]) if in_place else (torch.full_like(dkv[..., :128].contiguous(), float("nan")) for _ in range(2))
    grads = (torch.full(q.shape, float("nan"), device="cuda"), *views, torch.full(k_pe.shape, float("nan"), device="cuda"))
    dq, dk_nope, dk_pe, dv = ops.flash_attn_mla_prefill_bwd(q, k_nope, k_pe, v, out, do, lse, cu_q, cu_k, grads=(grads[0], grads[1], grads[3], grads[2]))
    return dq.cpu(), torch.cat([dk_nope, dv], -1).cpu(), dk_pe.cpu()


@pytest.mark.parametrize("case,H", [("A", 2), ("B", 2), ("C", 2), ("B", H_GROUPS)])
def test_backward_matches_the_fp64_reference(case, H):
    q, kv, k_pe, cu_q, cu_k = inputs(case, H)
    got, (_, *want) = backward(q, kv, k_pe, cu_q, cu_k, out_grad(case, H)), reference_grads(case, H)
    errs = [(g.double() - w).abs().max().item() for g, w in zip(got, want)]
    print("max-abs dq %.2e  dk_nope|dv %.2e  dk_pe %.2e" % tuple(errs))
    assert errs[0] <= TOL["bf16"] and errs[1] <= TOL["bf16"] and errs[2] <= H * TOL["bf16"], errs
    # exact zeros: rows that admit no key, keys no query admits (those of a sequence without queries), rows no sequence owns
    live_k = torch.zeros(kv.shape[0], dtype=torch.bool)
    for b in range(len(cu_q) - 1):
        live_k[int(cu_k[b]):int(cu_k[b + 1])] = bool(cu_q[b + 1] > cu_q[b])
    assert not got[0][~expected(case, H)[2]].any() and not got[1][~live_k].any() and not got[2][~live_k].any()


def test_the_call_repeats_views_equal_contiguous_outputs_and_a_sequence_alone_gives_its_rows():
    q, kv, k_pe, cu_q, cu_k = inputs("B", H_GROUPS)
    do = out_grad("B", H_GROUPS)
    both, again, contiguous = backward(q, kv, k_pe, cu_q, cu_k, do), backward(q, kv, k_pe, cu_q, cu_k, do), backward(q, kv, k_pe, cu_q, cu_k, do, False)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(both, again, contiguous))
    (sq, eq), (sk, ek) = cu_q[2:4].tolist(), cu_k[2:4].tolist()
    z = lambda n: torch.tensor([0, n], dtype=torch.int32)
    alone = backward(q[sq:eq], kv[sk:ek], k_pe[sk:ek], z(eq - sq), z(ek - sk), do[sq:eq])
    assert torch.equal(alone[0], both[0][sq:eq]) and torch.equal(alone[1], both[1][sk:ek]) and torch.equal(alone[2], both[2][sk:ek])


def test_flash_attn_mla_prefill_train_under_autograd():
    from flash_attention_minitorch_amd import device_ops as ops
    q, kv, k_pe, cu_q, cu_k = inputs("B", 2)
    tq, tkv, tp = (t.cuda().requires_grad_() for t in (q, kv, k_pe))
    out = ops.flash_attn_mla_prefill_train(tq, tkv[..., :128], tp, tkv[..., 128:], cu_q.cuda(), cu_k.cuda())
    assert out.dtype is torch.float32 and out.grad_fn is not None
    out.backward(out_grad("B", 2).cuda().float())
    rout, *want = reference_grads("B", 2)
    assert (out.detach().cpu().double() - rout).abs().max().item() <= TOL["bf16"]
    for t, w, tol in zip((tq, tkv, tp), want, (1, 1, 2)):
        assert t.grad.dtype is torch.bfloat16 and t.grad.shape == t.shape
        err = (t.grad.cpu().double() - w).abs().max().item()
        # (the gradient's own rounding to bf16: half an ulp, 2^-8 relative, as _grad_bound of tests/test_gpu_prefix.py)
        assert err <= tol * TOL["bf16"] + 2.0 ** -8 * w.abs().max().item(), err
