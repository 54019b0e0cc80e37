"""Sliding-window / attention-sink forward and backward (libflash_attn_mi355x_window.so) on the GPU against the fp64 reference of
tests/test_window_train_cpu.py: shapes on the edges of the row blocks (128 queries; dQ 128), the key tiles (64 bf16 / 32 fp32) and the
query slices (128 / 64 / 32), the exact sweep bounds of the three kernels, the cache kernels' mask, repeatability, grouped heads and
autograd.  Tolerances: the project's envelope, max-abs 1e-4 (fp32) and 1e-3 (bf16) on out, lse, dq, dk and dv."""
import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import TOL
from test_window_train_cpu import admitted, window_train_reference

pytestmark = pytest.mark.gpu

NAMES = ("out", "lse", "dq", "dk", "dv")


def _torch():
    import torch
    return torch


def _inputs(rng, dtype, B, H, Hkv, N, d):
    """q, k, v, do as (B, heads, N, d) float32 arrays, U(-1, 1), rounded to the dtype first."""
    rnd = (lambda s: oracle.bf16_round(rand_u(rng, s))) if dtype == "bf16" else (lambda s: rand_u(rng, s))
    return rnd((B, H, N, d)), rnd((B, Hkv, N, d)), rnd((B, Hkv, N, d)), rnd((B, H, N, d))


def _dev(a, layout, dtype):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a if layout == "bhnd" else a.transpose(0, 2, 1, 3)))
    return t.to("cuda", torch.bfloat16 if dtype == "bf16" else torch.float32).contiguous()


def _host(t, layout):
    a = t.detach().double().cpu().numpy()
    return a if layout == "bhnd" or a.ndim == 3 else a.transpose(0, 2, 1, 3)


def _run(q, k, v, do, W, S, layout, dtype, scale=None):
    """The forward and the backward through device_ops; out, lse, dq, dk, dv as (B, heads, N, d) / (B, H, N) fp64 arrays."""
    from flash_attention_minitorch_amd import device_ops
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S, scale, layout)
    dq, dk, dv = device_ops.flash_attn_bwd_window(tq, tk, tv, o, tdo, lse, W, S, scale, layout)
    return [_host(t, layout) for t in (o, lse, dq, dk, dv)]


def _compare(got, want, tol, what):
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    print(what, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(np.all(np.isfinite(g)) for g in got), what
    assert all(e < tol for e in errs.values()), (what, errs, tol)


# (N, W, S, d, dtype, layout, H, Hkv, B): a covering selection -- every N, W, S, d, dtype, layout and head grouping of the lists
# below, and every (d, dtype) pair with a sink and with grouped heads.  W = 0 stands for N - 1.
CASES = [
    (1, 1, 0, 32, "f32", "bhnd", 2, 2, 2),
    (33, 2, 1, 64, "bf16", "bnhd", 8, 2, 2),
    (127, 31, 5, 128, "f32", "bnhd", 4, 1, 1),
    (128, 32, 0, 32, "bf16", "bhnd", 2, 2, 2),
    (129, 33, 32, 64, "f32", "bhnd", 8, 2, 1),
    (257, 63, 33, 128, "bf16", "bhnd", 4, 1, 2),
    (384, 64, 128, 32, "f32", "bnhd", 8, 2, 1),
    (515, 65, 129, 64, "bf16", "bhnd", 4, 1, 2),
    (515, 127, 5, 128, "bf16", "bnhd", 8, 2, 1),
    (384, 128, 1, 32, "bf16", "bnhd", 4, 1, 2),
    (515, 129, 33, 64, "f32", "bnhd", 4, 1, 1),
    (515, 256, 5, 128, "f32", "bhnd", 8, 2, 1),
    (515, 257, 0, 64, "bf16", "bnhd", 2, 2, 2),
    (515, 0, 0, 32, "f32", "bhnd", 2, 2, 1),
    (257, 1, 0, 128, "bf16", "bhnd", 2, 2, 1),
    (257, 31, 129, 32, "bf16", "bhnd", 8, 2, 1),
    (384, 1, 32, 64, "f32", "bnhd", 2, 2, 1),
    (129, 0, 5, 128, "bf16", "bnhd", 4, 1, 1),
]


def test_the_cases_cover_every_axis_value_and_every_d_dtype_pair_with_a_sink_and_with_groups():
    col = lambda i: {c[i] for c in CASES}
    assert col(0) == {1, 33, 127, 128, 129, 257, 384, 515}
    assert col(1) == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 0}
    assert col(2) == {0, 1, 5, 32, 33, 128, 129}
    assert col(3) == {32, 64, 128} and col(4) == {"f32", "bf16"} and col(5) == {"bnhd", "bhnd"}
    assert {(c[6], c[7]) for c in CASES} == {(2, 2), (8, 2), (4, 1)}
    pairs = {(d, t) for d in (32, 64, 128) for t in ("f32", "bf16")}
    assert {(c[3], c[4]) for c in CASES if c[2] > 0 and c[6] > c[7]} == pairs
    assert all(c[8] <= 2 and c[6] <= 8 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}-W{}-S{}-d{}-{}-{}-h{}kv{}-B{}".format(*c))
def test_forward_and_backward_match_the_fp64_reference(case):
    N, W, S, d, dtype, layout, H, Hkv, B = case
    W = W or N - 1
    q, k, v, do = _inputs(np.random.default_rng(N * 1000 + W + S), dtype, B, H, Hkv, N, d)
    _compare(_run(q, k, v, do, W, S, layout, dtype), window_train_reference(q, k, v, do, W, S), TOL[dtype], str(case))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_kernels(dtype):
    B, H, Hkv, N, d, W, S, scale = 1, 4, 2, 200, 64, 40, 3, 0.2
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, B, H, Hkv, N, d)
    _compare(_run(q, k, v, do, W, S, "bnhd", dtype, scale), window_train_reference(q, k, v, do, W, S, scale), TOL[dtype], "scale")


@pytest.mark.parametrize("W,S", [(129, 0), (1000, 0), (5, 129), (7, 4000), (2 ** 31 - 1, 2 ** 31 - 1)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_window_or_sink_over_the_whole_sequence_is_causal_attention_by_these_kernels(dtype, W, S):
    """Through the C entry point (device_ops.flash_attn_fwd_window / _bwd_window pass W and S on): W >= N and S >= N are clamped."""
    B, H, Hkv, N, d = 1, 4, 2, 129, 64
    q, k, v, do = _inputs(np.random.default_rng(11), dtype, B, H, Hkv, N, d)
    ke, ve = np.repeat(k, 2, 1), np.repeat(v, 2, 1)
    ro, rL, _, _ = oracle.dense_attention_fw(q, ke, ve, causal=True)
    rdq, rdk, rdv = oracle.dense_attention_bw(q, ke, ve, do, causal=True)
    want = (ro, rL, rdq, rdk.reshape(B, Hkv, 2, N, d).sum(2), rdv.reshape(B, Hkv, 2, N, d).sum(2))
    _compare(_run(q, k, v, do, W, S, "bnhd", dtype), want, TOL[dtype], f"clamp W={W} S={S}")


def _bits_equal(a, b):
    torch = _torch()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attn_gqa_with_a_window_over_everything_returns_the_unwindowed_bits(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, d = 2, 4, 2, 200, 64
    q, k, v, do = _inputs(np.random.default_rng(13), dtype, B, H, Hkv, N, d)

    def grads(**kw):
        tq, tk, tv = (_dev(a, "bnhd", dtype).requires_grad_() for a in (q, k, v))
        o = device_ops.flash_attn_gqa(tq, tk, tv, causal=True, **kw)
        o.backward(_dev(do, "bnhd", "f32"))
        return o.detach(), tq.grad, tk.grad, tv.grad
    plain = grads()
    for kw in (dict(window=None), dict(window=0), dict(window=N), dict(window=N + 7), dict(window=3, sink=N), dict(window=3, sink=N + 1)):
        assert all(_bits_equal(a, b) for a, b in zip(grads(**kw), plain)), kw
    assert not _bits_equal(grads(window=N - 1)[0], plain[0])   # (a real window is another function)
    torch.cuda.synchronize()


# ---- the sweep bounds, exactly ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gradients_are_zero_exactly_where_the_mask_says_so(dtype):
    """N = 515, W = 100, S = 5, d = 64, dO zero except one row i (then one 128-row block): dq is zero off the row, dk and dv are zero
    at every key the row does not admit and non-zero at the ones it does.  (A row that admits ONE key has P = 1 and dS = 0: its dk is
    zero in exact arithmetic, so only dv is required to be non-zero there.)  A sweep that starts late or ends early leaves an admitted
    key at zero; one that masks too little writes to a key that is not admitted."""
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, d, W, S = 1, 4, 2, 515, 64, 100, 5
    q, k, v, do = _inputs(np.random.default_rng(17), dtype, B, H, Hkv, N, d)
    tq, tk, tv = (_dev(a, "bnhd", dtype) for a in (q, k, v))
    o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S)
    adm = admitted(N, W, S)
    for rows in [[i] for i in (0, 4, 5, 99, 100, 104, 105, 300, 514)] + [list(range(256, 384))]:
        part = np.zeros_like(do)
        part[:, :, rows] = do[:, :, rows]
        dq, dk, dv = (_host(t, "bnhd") for t in device_ops.flash_attn_bwd_window(tq, tk, tv, o, _dev(part, "bnhd", dtype), lse, W, S))
        keys = adm[rows].any(axis=0)
        off = np.ones(N, bool)
        off[rows] = False
        assert np.all(dq[:, :, off] == 0), rows
        if keys.sum() > 1:
            assert np.all(np.abs(dq[:, :, rows]).max(-1) > 0), rows
        assert np.all(dk[:, :, ~keys] == 0) and np.all(dv[:, :, ~keys] == 0), (rows, np.nonzero(np.abs(dv).max((0, 1, 3)) * ~keys))
        assert np.all(np.abs(dv[:, :, keys]).max(-1) > 0), rows
        if keys.sum() > 1:
            assert np.all(np.abs(dk[:, :, keys]).max(-1) > 0), rows


# ---- against the cache kernels: one mask, two independent sets of kernels ----

@pytest.mark.parametrize("N,W,S,d,H,Hkv", [(515, 100, 5, 64, 4, 2), (384, 33, 0, 128, 8, 2), (257, 129, 33, 32, 4, 1)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_matches_flash_attn_extend_on_a_cache_of_the_same_keys(dtype, N, W, S, d, H, Hkv):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B = 2
    q, k, v, _ = _inputs(np.random.default_rng(N + W), dtype, B, H, Hkv, N, d)
    tq, tk, tv = (_dev(a, "bnhd", dtype) for a in (q, k, v))
    o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    eo, else_ = device_ops.flash_attn_extend(tq, tk, tv, cache_seqlens=lens, window=W, sink=S or None)
    assert maxabs(to_np(o), to_np(eo)) < 2 * TOL[dtype] and maxabs(to_np(lse), to_np(else_)) < 2 * TOL[dtype]


# ---- repeatability, grouped vs expanded ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_calls_return_the_same_bits(dtype):
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, d, W, S = 2, 8, 2, 515, 64, 100, 5
    q, k, v, do = _inputs(np.random.default_rng(19), dtype, B, H, Hkv, N, d)
    tq, tk, tv, tdo = (_dev(a, "bnhd", dtype) for a in (q, k, v, do))

    def call():
        o, lse = device_ops.flash_attn_fwd_window(tq, tk, tv, W, S)
        return (o, lse) + tuple(device_ops.flash_attn_bwd_window(tq, tk, tv, o, tdo, lse, W, S))
    first, second = call(), call()
    assert all(_bits_equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_heads_match_the_call_on_expanded_k_and_v(dtype, layout):
    B, H, Hkv, N, d, W, S = 2, 8, 2, 300, 128, 70, 3
    G = H // Hkv
    q, k, v, do = _inputs(np.random.default_rng(23), dtype, B, H, Hkv, N, d)
    got = _run(q, k, v, do, W, S, layout, dtype)
    o, lse, dq, dk, dv = _run(q, np.repeat(k, G, 1), np.repeat(v, G, 1), do, W, S, layout, dtype)
    want = (o, lse, dq, dk.reshape(B, Hkv, G, N, d).sum(2), dv.reshape(B, Hkv, G, N, d).sum(2))
    assert np.array_equal(got[0], o) and np.array_equal(got[1], lse) and np.array_equal(got[2], dq)   # (the same kernels on the same rows)
    _compare(got, want, TOL[dtype], "grouped vs expanded")


# ---- autograd ----

@pytest.mark.parametrize("d,layout,dtype", [(64, "bnhd", "bf16"), (128, "bhnd", "f32"), (80, "bnhd", "bf16"), (80, "bhnd", "f32")])
def test_flash_attn_gqa_window_under_autograd(d, layout, dtype):
    """flash_attn_gqa(window=, sink=) and .backward() against the reference's gradients; d = 80 through the zero padding
    (device_ops.pad_head_dim in front of the operator, softmax_scale = 1/sqrt(80); the padding's backward drops the zero columns)."""
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, W, S = 2, 4, 2, 200, 50, 4
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, B, H, Hkv, N, d)
    tq, tk, tv = (_dev(a, layout, dtype).requires_grad_() for a in (q, k, v))
    dp = device_ops.padded_head_dim(d)
    if dp == d:
        o = device_ops.flash_attn_gqa(tq, tk, tv, True, None, layout, window=W, sink=S)
    else:
        pq, pk, pv = (device_ops.pad_head_dim(t, dp) for t in (tq, tk, tv))
        o = device_ops.flash_attn_gqa(pq, pk, pv, True, d ** -0.5, layout, window=W, sink=S)[..., :d]
    o.backward(_dev(do, layout, "f32"))
    assert tq.grad.dtype == tq.dtype and tk.grad.shape == tk.shape
    want = window_train_reference(q, k, v, do, W, S)
    got = [_host(t, layout) for t in (o, tq.grad, tk.grad, tv.grad)]
    # the gradients come back in the input dtype: bf16 (8 significant bits) adds one rounding, at most half an ulp = 2^-8 relative
    tol = TOL[dtype]
    errs = [maxabs(g, w) for g, w in zip(got, (want[0], want[2], want[3], want[4]))]
    bound = [tol] + [tol + (2.0 ** -8 * float(np.max(np.abs(w))) if dtype == "bf16" else 0.0) for w in want[2:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)
