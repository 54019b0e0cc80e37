"""MLA prefill backward without a GPU (include/flash_attn_mi355x_mla_prefill.h, csrc/fa_mla_prefill_bwd.h): the fp64 autograd
reference, every refusal of the backward call in front of a HIP call, the workspace law, the Python checks, and the inputs of
tests/test_gpu_mla_prefill_bwd.py, which must tell a right kernel from one that sums dk_pe over one head group only and from one
that drops the k_pe columns of dq."""
import functools
import re

import pytest
import torch

from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_mla_prefill_cpu import BAD_ARG, SCALE, TOL, _GOOD, expected, inputs

HPG = lambda H: min(8, max(2, H // 16))   # heads per group of the dK/dV kernel (csrc/fa_mla_prefill_bwd.h)
H_GROUPS = 2 * HPG(5) + 1                 # = 5: two full head groups and a partial one


@functools.lru_cache(maxsize=None)
def out_grad(case, H):
    q, _, _, cu_q, _ = inputs(case, H)
    return (torch.rand(q.shape[0], H, 128, generator=torch.Generator().manual_seed(11)) * 2 - 1).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def reference_grads(case, H, heads=None, pe=True):
    """torch float64 autograd over the dense definition, per sequence and head: bottom-right mask, scores over [k_nope_h | k_pe].
    Returns out, dq, dkv (Tk, H, 256) = dk_nope | dv, dk_pe.  ``heads``: only these heads feed the loss; ``pe`` False: the k_pe
    columns dropped from the scores."""
    q, kv, k_pe, cu_q, cu_k = (t.double().requires_grad_() if t.is_floating_point() else t for t in inputs(case, H))
    out = torch.zeros(q.shape[0], H, 128, dtype=torch.float64)
    for b in range(len(cu_q) - 1):
        (sq, eq), (sk, ek) = (int(cu_q[b]), int(cu_q[b + 1])), (int(cu_k[b]), int(cu_k[b + 1]))
        admit = torch.arange(ek - sk)[None, :] <= torch.arange(eq - sq)[:, None] + (ek - sk) - (eq - sq)
        rows = admit.any(-1)
        for h in range(H if rows.any() else 0):
            k = torch.cat([kv[sk:ek, h, :128], k_pe[sk:ek] if pe else k_pe[sk:ek] * 0], -1)
            p = torch.softmax((SCALE * q[sq:eq, h] @ k.T).masked_fill(~admit, float("-inf"))[rows], -1)
            o = torch.zeros(eq - sq, 128, dtype=torch.float64)
            o[rows] = p @ kv[sk:ek, h, 128:]
            out[sq:eq, h] = o
    pick = slice(None) if heads is None else list(heads)
    (out[:, pick] * out_grad(case, H).double()[:, pick]).sum().backward()
    return out.detach(), q.grad, kv.grad, k_pe.grad


def test_the_autograd_reference_agrees_with_the_numpy_reference():
    assert (reference_grads("B", 2)[0] - expected("B", 2)[0]).abs().max().item() < 1e-12


def test_gpu_inputs_tell_a_right_kernel_from_a_likely_wrong_one():
    H = H_GROUPS
    _, dq, _, dk_pe = reference_grads("B", H)
    first_group = reference_grads("B", H, heads=tuple(range(HPG(H))))[3]
    assert (dk_pe - first_group).abs().max().item() >= 10 * H * TOL
    assert (dq - reference_grads("B", H, pe=False)[1]).abs().max().item() >= 10 * TOL


# ---- refusals, before any HIP call ----
_GOOD_BWD = dict(_GOOD, dout=2304, dq=2560, dk_nope=2816, dk_pe=3072, dv=3328, dk_ld=1024, dk_hs=256, dv_ld=1024, dv_hs=256)
_BAD = [
    (dict(nseq=0), "positive"), (dict(Tk=0), "positive"), (dict(H=-1), "positive"), (dict(q=0), "null pointer"), (dict(out=0), "null pointer"),
    (dict(dout=0), "null pointer"), (dict(dq=0), "null pointer"), (dict(dk_nope=0), "null pointer"), (dict(dk_pe=0), "null pointer"),
    (dict(dv=0), "null pointer"), (dict(ws=0), "null pointer"), (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("nan")), "softmax_scale"),
    (dict(k_ld=1028), "k_nope: row stride and head stride must be multiples of 8"), (dict(v_ld=512), "v: row stride below"),
    (dict(dk_ld=1026), "dk_nope: row stride and head stride must be multiples of 4"), (dict(dv_hs=258), "dv: row stride and head stride must be multiples of 4"),
    (dict(dk_hs=124), "dk_nope: head stride below"), (dict(dv_ld=512), "dv: row stride below"), (dict(dk_ld=1 << 21, Tk=256), "dk_nope: byte offsets"),
    (dict(Tk=1 << 19), "dk_nope: byte offsets"), (dict(Tq=1 << 21), "q: byte offsets"), (dict(Tq=1 << 20), "out: byte offsets"),
    (dict(Tq=700000), "dq: byte offsets"), (dict(k_nope=520), "q, k_nope, k_pe, v and out must be 16-byte aligned"),
    (dict(dout=2312), "dout, dq, dk_nope, dk_pe and dv must be 16-byte aligned"), (dict(dk_pe=3080), "dout, dq, dk_nope, dk_pe and dv must be 16-byte aligned"),
    (dict(ws=2176), "256-byte aligned"),
]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_backward_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(_GOOD_BWD, **over), built.mla_prefill()
    ptrs = ("q", "k_nope", "k_pe", "v", "out", "dout", "lse", "dq", "dk_nope", "dk_pe", "dv", "cu_q", "cu_k", "ws")
    ints = ("nseq", "Tq", "Tk", "H", "k_ld", "k_hs", "v_ld", "v_hs", "dk_ld", "dk_hs", "dv_ld", "dv_hs", "scale")
    rc = lib.fa_mi355x_bwd_mla_prefill(*[a[n] or None for n in ptrs], *[a[n] for n in ints], None)
    err = lib.fa_mi355x_mla_prefill_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


@pytest.mark.parametrize("nseq,Tq,Tk,H", [(5, 394, 394, 2), (4, 197, 685, 5), (1, 1, 1, 1), (16, 16384, 16384, 128), (3, 127, 9, 33)])
def test_backward_workspace_is_the_maps_the_row_constants_and_the_partials(built, nseq, Tq, Tk, H):
    ws, al = built.mla_prefill().fa_mi355x_bwd_mla_prefill_workspace_bytes, lambda n: -(-n // 256) * 256
    groups = -(-H // built.mla_prefill_heads_per_group(H))
    assert built.mla_prefill_heads_per_group(H) == HPG(H)
    assert ws(nseq, Tq, Tk, H) == (al(32 * (Tq // 128 + nseq)) + al(32 * (Tk // 128 + nseq)) + al(3 * H * Tq * 4)
                                   + (groups * Tk * 64 * 4 if groups > 1 else 0))
    assert ws(0, Tq, Tk, H) == ws(nseq, 0, Tk, H) == ws(nseq, Tq, 0, H) == ws(nseq, Tq, Tk, 0) == 0


def test_python_checks_name_the_operand_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    monkeypatch.setattr(_lib, "mla_prefill", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype)
    q, kv, k_pe, cu = z(10, 2, 192), z(10, 2, 256), z(10, 64), torch.tensor([0, 10], dtype=torch.int32)
    k, v, o, do, lse = kv[..., :128], kv[..., 128:], z(10, 2, 128, dtype=torch.float32), z(10, 2, 128), z(2, 10, dtype=torch.float32)
    for bad, exc, msg in [
        (lambda: ops.flash_attn_mla_prefill_bwd(z(10, 2, 128), k, k_pe, v, o, do, lse, cu), ValueError, "q must be"),
        (lambda: ops.flash_attn_mla_prefill_bwd(q, k, z(9, 64), v, o, do, lse, cu), ValueError, "k_pe must have k_nope's 10 rows"),
        (lambda: ops.flash_attn_mla_prefill_bwd(q, k, k_pe, v.float(), o, do, lse, cu), TypeError, "v must be bfloat16"),
        (lambda: ops.flash_attn_mla_prefill_bwd(q, k, k_pe, v, o, do, lse, cu, softmax_scale=0.0), ValueError, "softmax_scale must be"),
        (lambda: ops.flash_attn_mla_prefill_train(q, z(10, 2, 132)[..., 4:], k_pe, v, cu), ValueError, "k_nope may be a view"),
    ]:
        with pytest.raises(exc, match=re.escape(msg)):
            bad()
