"""Logit soft-capping in the training forward and backward (fa_mi355x_fwd_window_softcap / _bwd_window_softcap) on the GPU against
the fp64 reference of tests/test_softcap_train_cpu.py: the edges of the window test (row blocks, key tiles, query slices, thin
rows, sinks) under a cap that bites, saturation, repeatability, softcap = 0, autograd, grouped heads, and the model layer against the
prefill of a capped KV cache.  Tolerances: the project's envelope, max-abs 1e-4 (fp32) and 1e-3 (bf16) on out, lse, dq, dk and dv."""
import ctypes

import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import TOL
from test_gpu_window_train import NAMES, _bits_equal, _compare, _dev, _host, _inputs, _torch
from test_softcap_train_cpu import softcap_train_reference

pytestmark = pytest.mark.gpu

CAP = 0.25   # U(-1, 1) inputs give scaled scores of standard deviation 1/3: most of them sit on the bend of the tanh


def _run(q, k, v, do, W, S, layout, dtype, scale=None, cap=CAP):
    """The capped forward and backward through device_ops; out, lse, dq, dk, dv as (B, heads, N, d) / (B, H, N) fp64 arrays."""
    from flash_attention_minitorch_amd import device_ops
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S, scale, layout, softcap=cap)
    dq, dk, dv = device_ops.flash_attn_bwd_window(tq, tk, tv, o, tdo, lse, W, S, scale, layout, softcap=cap)
    return [_host(t, layout) for t in (o, lse, dq, dk, dv)]


def _discriminates(q, k, v, do, W, S, scale, cap, want, tol, what):
    """On the references alone: the capped function is far from the uncapped one on all five tensors, and its backward is far from the
    one without the 1 - tanh^2 factor on dq and dk, so a kernel that ignores the cap, or caps only the forward, cannot pass.  A row
    that admits ONE key (W = 1 without sinks, N = 1) has P = 1 whatever the score: out, dq, dk and dv do not depend on the cap there
    (dq = dk = 0 exactly), and only lse can tell the two functions apart."""
    plain = softcap_train_reference(q, k, v, do, W, S, scale, 0.0)
    diffs = {n: maxabs(a, b) for n, a, b in zip(NAMES, want, plain)}
    loose = softcap_train_reference(q, k, v, do, W, S, scale, cap, chain=False)
    chain = {n: maxabs(want[i], loose[i]) for i, n in ((2, "dq"), (3, "dk"))}
    print(what, "capped vs uncapped", {n: f"{e:.2e}" for n, e in diffs.items()}, "chain rule", {n: f"{e:.2e}" for n, e in chain.items()})
    if W == 1 and S == 0:
        assert diffs["lse"] >= 10 * tol, (what, diffs)
        return
    assert all(e >= 10 * tol for e in diffs.values()), (what, diffs)
    assert all(e >= 10 * tol for e in chain.values()), (what, chain)


# (N, W, S, d, dtype, layout, H, Hkv, B): the edges (N, W, S) of the issue, spread so that every d, dtype, layout and head grouping
# appears and every (d, dtype) pair appears with a sink and grouped heads.  W = 0 stands for N (a cap without a window).
CASES = [
    (1, 1, 0, 32, "f32", "bhnd", 2, 2, 2),
    (33, 2, 1, 64, "bf16", "bnhd", 8, 2, 2),
    (129, 33, 32, 64, "f32", "bhnd", 8, 2, 1),
    (129, 33, 32, 32, "bf16", "bnhd", 4, 1, 2),
    (257, 63, 33, 128, "bf16", "bhnd", 4, 1, 2),
    (384, 64, 128, 32, "f32", "bnhd", 8, 2, 1),
    (515, 127, 5, 128, "f32", "bnhd", 4, 1, 1),
    (515, 127, 5, 64, "bf16", "bhnd", 2, 2, 1),
    (515, 0, 0, 64, "bf16", "bnhd", 2, 2, 2),
    (515, 0, 0, 128, "f32", "bhnd", 8, 2, 1),
    (257, 1, 0, 128, "bf16", "bhnd", 2, 2, 1),
]


def test_the_cases_cover_every_edge_and_axis_value_and_every_d_dtype_pair_with_a_sink_and_with_groups():
    assert {c[:3] for c in CASES} == {(1, 1, 0), (33, 2, 1), (129, 33, 32), (257, 63, 33), (384, 64, 128), (515, 127, 5), (515, 0, 0),
                                      (257, 1, 0)}
    col = lambda i: {c[i] for c in CASES}
    assert col(3) == {32, 64, 128} and col(4) == {"f32", "bf16"} and col(5) == {"bnhd", "bhnd"}
    assert {(c[6], c[7]) for c in CASES} == {(2, 2), (8, 2), (4, 1)}
    pairs = sorted((d, t) for d in (32, 64, 128) for t in ("f32", "bf16"))
    assert sorted((c[3], c[4]) for c in CASES if c[2] > 0 and c[6] > c[7]) == pairs   # each pair once
    assert all(c[8] <= 2 and c[6] <= 8 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}-W{}-S{}-d{}-{}-{}-h{}kv{}-B{}".format(*c))
def test_capped_forward_and_backward_match_the_fp64_reference(case):
    N, W, S, d, dtype, layout, H, Hkv, B = case
    W = W or N
    q, k, v, do = _inputs(np.random.default_rng(N * 1000 + W + S + d), dtype, B, H, Hkv, N, d)
    want = softcap_train_reference(q, k, v, do, W, S, None, CAP)
    _discriminates(q, k, v, do, W, S, None, CAP, want, TOL[dtype], str(case))
    _compare(_run(q, k, v, do, W, S, layout, dtype), want, TOL[dtype], str(case))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_capped_kernels(dtype):
    B, H, Hkv, N, d, W, S, scale = 1, 4, 2, 200, 64, 40, 3, 0.2
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, B, H, Hkv, N, d)
    want = softcap_train_reference(q, k, v, do, W, S, scale, CAP)
    _discriminates(q, k, v, do, W, S, scale, CAP, want, TOL[dtype], "scale")
    assert maxabs(want[0], softcap_train_reference(q, k, v, do, W, S, None, CAP)[0]) >= 10 * TOL[dtype]   # (the scale matters)
    _compare(_run(q, k, v, do, W, S, "bnhd", dtype, scale), want, TOL[dtype], "scale")


# ---- saturation ----

@pytest.mark.parametrize("amp,cap", [(64.0, 0.5), (16.0, 50.0)], ids=["x64-cap0.5", "x16-cap50"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_capped_backward_saturates_cleanly(dtype, amp, cap):
    """q x 64 (exact in bf16) with softcap = 0.5: tau * q.k / softcap reaches hundreds, the exp2 argument overflows, nearly every
    logit sits at +-softcap and 1 - tanh^2 = 4 r (1 - r) is 0 there, not inf * 0.  q x 16 with softcap = 50: Gemma-2's regime, logits
    of tens, the cap nearly linear.  All five tensors stay finite and inside the project's large-magnitude envelope, 5e-3 x the
    tensor's scale (README "Accuracy envelope").  Measured maxima: profiles/softcap_train_accuracy.txt."""
    B, H, Hkv, N, d, W, S = 1, 4, 2, 300, 64, 100, 3
    q, k, v, do = _inputs(np.random.default_rng(int(amp) + (3 if dtype == "bf16" else 0)), dtype, B, H, Hkv, N, d)
    q = q * np.float32(amp)
    smax = float(np.max(np.abs(np.einsum("bhid,bhjd->bhij", q[:, ::2].astype(np.float64), k)))) / np.sqrt(d)
    assert smax / cap > (100 if cap < 1 else 0.2)
    want = softcap_train_reference(q, k, v, do, W, S, None, cap)
    got = _run(q, k, v, do, W, S, "bnhd", dtype, None, cap)
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    scales = {n: max(1.0, float(np.max(np.abs(w)))) for n, w in zip(NAMES, want)}
    print(f"softcap_train_accuracy {dtype} amp={amp:g} cap={cap:g} N={N} W={W} S={S} d={d}: max|tau*s|/cap={smax / cap:.1f} "
          + " ".join(f"{n} {errs[n]:.3e} (scale {scales[n]:.2f})" for n in NAMES))
    assert all(np.all(np.isfinite(g)) for g in got)
    assert all(errs[n] < 5e-3 * scales[n] for n in NAMES), (errs, scales)


# ---- bit for bit ----

def _fwd_bwd(tq, tk, tv, tdo, W, S, layout="bnhd", **kw):
    from flash_attention_minitorch_amd import device_ops
    o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S, None, layout, **kw)
    return (o, lse) + tuple(device_ops.flash_attn_bwd_window(tq, tk, tv, o, tdo, lse, W, S, None, layout, **kw))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_capped_calls_return_the_same_bits(dtype):
    B, H, Hkv, N, d, W, S = 2, 8, 2, 515, 64, 100, 5
    q, k, v, do = _inputs(np.random.default_rng(19), dtype, B, H, Hkv, N, d)
    tq, tk, tv, tdo = (_dev(a, "bnhd", dtype) for a in (q, k, v, do))
    first, second = _fwd_bwd(tq, tk, tv, tdo, W, S, softcap=CAP), _fwd_bwd(tq, tk, tv, tdo, W, S, softcap=CAP)
    assert all(_bits_equal(a, b) for a, b in zip(first, second))
    assert not _bits_equal(first[0], _fwd_bwd(tq, tk, tv, tdo, W, S)[0])   # (and a cap is another function)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_cap_of_zero_through_the_softcap_entry_points_is_the_window_call(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    B, H, Hkv, N, d, W, S = 2, 8, 2, 300, 128, 70, 3
    q, k, v, do = _inputs(np.random.default_rng(29), dtype, B, H, Hkv, N, d)
    tq, tk, tv, tdo = (_dev(a, "bnhd", dtype) for a in (q, k, v, do))
    want = _fwd_bwd(tq, tk, tv, tdo, W, S)
    lib, p = _lib.window(), device_ops._ptr
    o, dq = (torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    dk, dv = (torch.full(tk.shape, float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    lse = torch.full((B, H, N), float("nan"), dtype=torch.float32, device="cuda")
    ws = device_ops.bwd_workspace_window(tq, tk)
    tail = (B, H, Hkv, N, d, _lib.FA_LAYOUT_BNHD, 0.0, W, 0.0, S, device_ops._dtype_code(tq), device_ops._stream_ptr())
    _lib.window_check(lib.fa_mi355x_fwd_window_softcap(p(tq), p(tk), p(tv), p(o), p(lse), *tail))
    _lib.window_check(lib.fa_mi355x_bwd_window_softcap(p(tq), p(tk), p(tv), p(o), p(tdo), p(dq), p(dk), p(dv), p(lse), p(ws), *tail))
    assert all(_bits_equal(a, b) for a, b in zip((o, lse, dq, dk, dv), want))
    assert isinstance(tail[8], float) and ctypes.c_float in lib.fa_mi355x_fwd_window_softcap.argtypes


@pytest.mark.parametrize("kw", [dict(), dict(window=50, sink=4)], ids=["no-window", "W50-S4"])
@pytest.mark.parametrize("layout,dtype", [("bnhd", "bf16"), ("bhnd", "f32")])
def test_flash_attn_gqa_softcap_under_autograd_returns_the_explicit_backward_bits(layout, dtype, kw):
    """flash_attn_gqa(softcap=) and .backward(): the gradients are flash_attn_bwd_window(softcap=)'s, cast to the input dtype; without
    a window the call is the one with W = N.  And they are the reference's, within the tolerance plus the cast's half ulp."""
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, d = 2, 4, 2, 200, 64
    W, S = kw.get("window", N), kw.get("sink", 0)
    q, k, v, do = _inputs(np.random.default_rng(31), dtype, B, H, Hkv, N, d)
    tq, tk, tv = (_dev(a, layout, dtype).requires_grad_() for a in (q, k, v))
    tdo = _dev(do, layout, "f32")
    o = device_ops.flash_attn_gqa(tq, tk, tv, True, None, layout, softcap=CAP, **kw)
    o.backward(tdo)
    eo, elg, edq, edk, edv = _fwd_bwd(tq.detach(), tk.detach(), tv.detach(), tdo.to(tq.dtype), W, S, layout, softcap=CAP)
    assert _bits_equal(o.detach(), eo)
    for g, e in ((tq.grad, edq), (tk.grad, edk), (tv.grad, edv)):
        assert _bits_equal(g, e.to(tq.dtype))
    want = softcap_train_reference(q, k, v, do, W, S, None, CAP)
    tol = TOL[dtype]
    got = [_host(t, layout) for t in (o, tq.grad, tk.grad, tv.grad)]
    errs = [maxabs(g, w) for g, w in zip(got, (want[0], want[2], want[3], want[4]))]
    bound = [tol] + [tol + (2.0 ** -8 * float(np.max(np.abs(w))) if dtype == "bf16" else 0.0) for w in want[2:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)


# ---- grouped vs expanded ----

@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_heads_match_the_capped_call_on_expanded_k_and_v(dtype, layout):
    B, H, Hkv, N, d, W, S = 2, 8, 2, 300, 128, 70, 3
    G = H // Hkv
    q, k, v, do = _inputs(np.random.default_rng(23), dtype, B, H, Hkv, N, d)
    got = _run(q, k, v, do, W, S, layout, dtype)
    o, lse, dq, dk, dv = _run(q, np.repeat(k, G, 1), np.repeat(v, G, 1), do, W, S, layout, dtype)
    want = (o, lse, dq, dk.reshape(B, Hkv, G, N, d).sum(2), dv.reshape(B, Hkv, G, N, d).sum(2))
    assert np.array_equal(got[0], o) and np.array_equal(got[1], lse) and np.array_equal(got[2], dq)   # (the same kernels on the same rows)
    _compare(got, want, TOL[dtype], "grouped vs expanded")


# ---- the model layer: what trains is what generates ----

@pytest.mark.parametrize("fused", [True, False], ids=["fused", "permuted"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_capped_stack_matches_the_prefill_of_a_capped_cache_and_its_weights_get_finite_gradients(dtype, fused):
    """attention_stack(softcap=, window=, rope=) against attention_stack_prefill on a KVCache(softcap=, window=, rope=) with the same
    weights (the extend kernels' cap: an independent set of kernels), at the model tolerance of tests/test_gpu_window_train_model.py
    (_model_tol); then a backward through the stack."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_gpu_decode import _tdt
    from test_gpu_decode_append import _stack
    from test_gpu_extend import _model_tol
    from test_gpu_window_train_model import B, E, H, HKV, L, N, W, _rope
    C = 0.1   # (scores of standard deviation about 0.1 in this stack: a cap that bites)
    x, layers = _stack(np.random.default_rng(W + 11), dtype, B, E, H, HKV, L, N)
    rope = _rope(mt)
    got = to_np(mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, window=W, softcap=C))
    cache = mt.KVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, window=W, rope=rope, softcap=C)
    gen = to_np(mt.attention_stack_prefill(x, layers, H, cache))
    tol = _model_tol(dtype, gen)
    print("capped stack vs capped prefill", maxabs(got, gen), tol)
    assert maxabs(got, gen) < tol, (maxabs(got, gen), tol)
    if dtype == "f32":   # and the capped stack is not the uncapped one
        plain = to_np(mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, window=W))
        print("capped vs uncapped stack", maxabs(got, plain))
        assert maxabs(got, plain) > 10 * tol
    ws = [tuple(w.clone().requires_grad_() for w in layer) for layer in layers]
    xg = x.clone().requires_grad_()
    mt.attention_stack(xg, ws, H, fused_layout=fused, rope=rope, window=W, softcap=C).float().square().mean().backward()
    for g in [xg.grad] + [w.grad for layer in ws for w in layer]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.float().abs().max()) > 0
