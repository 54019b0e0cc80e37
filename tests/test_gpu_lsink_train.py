"""Learned sink logits in training on the GPU (libflash_attn_mi355x_lsink.so, include/flash_attn_mi355x_lsink.h; flash_attn_gqa(...,
sink_logits=) under autograd) against the fp64 reference of tests/test_lsink_cpu.py (lsink_train_reference: the softmax with one
more column, and its analytic backward) on the same (bf16-rounded) inputs in U(-1, 1): out, lse, dq, dk and dv at the project's
tolerances (fp32 1e-4, bf16 1e-3), the gradient of the logits inside the bound derived below, the reduction bit for bit on a second
run, no grad launch when the logits do not require grad; and the train / generate law of the model: the stack under
attention_stack(window=, sink_logits=) is the stack a KVCache(window=, sink_logits=) generates."""
import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import _tdt, _torch
from test_gpu_decode_append import _stack
from test_gpu_extend import _model_tol
from test_lsink_cpu import TB, TH, THKV, TOL, TRAIN_N, TRAIN_W, train_case, train_reference

pytestmark = pytest.mark.gpu


def _dev(t, layout, dtype):
    """(B, H, N, d) numpy -> a contiguous device tensor in ``layout``."""
    x = _torch().from_numpy(np.ascontiguousarray(t if layout == "bhnd" else t.transpose(0, 2, 1, 3)))
    return x.to("cuda", _tdt(dtype)).contiguous()


def _np(t, layout):
    return to_np(t) if layout == "bhnd" else to_np(t).transpose(0, 2, 1, 3)


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_backward_and_logit_gradient_match_fp64_reference(dtype, layout, d):
    """N = 1, 33, 129, 300 (one row; part of a block; a block and a row; three blocks with a partial last one) with no window and
    with W = 64; B = 2, H = 4, Hkv = 2 (grouped heads read in place).
    The bound on sink_logits.grad, per head h:  tol * sum_{b,i} p_bhi * (|dO_bhi|_1 + 2 |delta_bhi|),  p = e^(a - lse), the terms
    from the fp64 reference.  d a = -sum p delta; delta = sum_c dO_c out_c inherits at most tol per element of out, so |d delta| <=
    tol |dO|_1; p inherits at most tol RELATIVE from lse (|d lse| <= tol), so |d p| <= tol p, which costs tol p |delta|; the second
    |delta| covers the fp32 exp2, products and the ordered sums."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    tol = TOL[dtype]
    for N in TRAIN_N:
        for W in TRAIN_W:
            c = train_case(dtype, d, N, W)
            ro, rl, rdq, rdk, rdv, rda, ps, l1, delta = train_reference(c, W)
            q, k, v, do = (_dev(c[n], layout, dtype) for n in ("q", "k", "v", "do"))
            a = torch.from_numpy(c["logits"]).cuda().requires_grad_()
            # the kernels' own fp32 results: the forward, and the EXISTING windowed backward on this forward's out and lse
            o, lse = device_ops.flash_attn_fwd_window_lsink(q, k, v, W or N, a.detach(), layout=layout)
            dq, dk, dv = device_ops.flash_attn_bwd_window(q, k, v, o, do, lse, W or N, layout=layout)
            # ... and the same through autograd, which also gives the logits their gradient
            qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
            oa = device_ops.flash_attn_gqa(qr, kr, vr, True, None, layout, W or None, sink_logits=a)
            oa.backward(do.float())
            torch.cuda.synchronize()
            assert torch.equal(oa, o) and all(torch.equal(g.grad, t.to(g.dtype)) for g, t in ((qr, dq), (kr, dk), (vr, dv)))
            assert a.grad.shape == (TH,) and a.grad.dtype == torch.float32
            errs = dict(out=maxabs(_np(o, layout), ro), lse=maxabs(to_np(lse), rl), dq=maxabs(_np(dq, layout), rdq),
                        dk=maxabs(_np(dk, layout), rdk), dv=maxabs(_np(dv, layout), rdv))
            print(f"lsink_train {dtype} {layout} d={d} N={N} W={W}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
            for n, e in errs.items():
                assert e < tol, (n, N, W, e)
            bound = tol * (ps * (l1 + 2 * np.abs(delta))).sum((0, 2))
            ea = np.abs(to_np(a.grad).astype(np.float64) - rda)
            print(f"lsink_train {dtype} {layout} d={d} N={N} W={W}: da err {ea.max():.2e} bound {bound.min():.2e} |da| {np.abs(rda).max():.2e}")
            assert np.all(ea <= bound), (N, W, ea, bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_logit_gradient_is_the_direct_call_and_repeats_bit_for_bit(dtype):
    """sink_logits_grad on the forward's own out and lse, twice, with and without a caller's workspace: the same bits, and the bits
    autograd returned.  B * N = 600 rows: two slices per head, so the second stage adds two partials."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    for layout in ("bnhd", "bhnd"):
        c = train_case(dtype, 64, 300, 64)
        q, k, v, do = (_dev(c[n], layout, dtype) for n in ("q", "k", "v", "do"))
        a = torch.from_numpy(c["logits"]).cuda()
        o, lse = device_ops.flash_attn_fwd_window_lsink(q, k, v, 64, a, layout=layout)
        ws = device_ops.lsink_workspace(q, layout)
        assert ws.numel() == TH * 2
        g1 = device_ops.sink_logits_grad(o, do, lse, a, layout)
        g2 = device_ops.sink_logits_grad(o, do, lse, a, layout, workspace=ws)
        g3 = device_ops.sink_logits_grad(o, do, lse, a, layout, workspace=ws)
        ar = a.clone().requires_grad_()
        device_ops.flash_attn_gqa(q, k, v, True, None, layout, 64, sink_logits=ar).backward(do.float())
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(g2, g3) and torch.equal(g1, ar.grad)
        o2, lse2 = device_ops.flash_attn_fwd_window_lsink(q, k, v, 64, a, layout=layout)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)


def test_no_grad_launch_when_the_logits_do_not_require_grad(monkeypatch):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    calls = []
    real = device_ops.sink_logits_grad
    monkeypatch.setattr(device_ops, "sink_logits_grad", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    c = train_case("bf16", 64, 129, 0)
    q, k, v, do = (_dev(c[n], "bnhd", "bf16") for n in ("q", "k", "v", "do"))
    for wants in (False, True):
        a = torch.from_numpy(c["logits"]).cuda().requires_grad_(wants)
        qr = q.clone().requires_grad_()
        device_ops.flash_attn_gqa(qr, k, v, True, sink_logits=a).backward(do.float())
        torch.cuda.synchronize()
        assert len(calls) == int(wants) and (a.grad is not None) == wants and qr.grad is not None


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "permuted"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stack_trained_with_logits_is_the_stack_a_cache_with_logits_generates(dtype, fused):
    """attention_stack(window=64, sink_logits=) over 300 tokens against attention_stack_prefill of the first 290 and ten single
    steps through KVCache(window=64, sink_logits=): the same rows, at the tolerance tests/test_gpu_window_train_model.py uses for
    this comparison; and in fp32 the stack without the logits is far away."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    E, H, HKV, L, B, N, W, P = 256, 4, 2, 2, 2, 300, 64, 290
    x, layers = _stack(np.random.default_rng(W), dtype, B, E, H, HKV, L, N)
    logits = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 3.0, (L, H)).astype(np.float32)).cuda()
    got = to_np(mt.attention_stack(x, layers, H, fused_layout=fused, window=W, sink_logits=logits))
    tol = _model_tol(dtype, got)
    cache = mt.KVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, window=W, sink_logits=logits)
    gen = [mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)]
    for n in range(P, N):
        gen.append(mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, cache))
    gen = to_np(torch.cat(gen, dim=1))
    assert maxabs(got, gen) < tol, (maxabs(got, gen), tol)
    assert maxabs(got[:, -10:], gen[:, -10:]) < tol
    if dtype == "f32":
        assert maxabs(got, to_np(mt.attention_stack(x, layers, H, fused_layout=fused, window=W))) > 5 * tol
