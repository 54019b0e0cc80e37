"""Grouped-query (GQA / MQA) KV-cache decode on the GPU (fa_mi355x_fwd_decode_gqa, include/flash_attn_mi355x_decode.h) against the fp64
decode reference of tests/test_decode_cpu.py on k and v repeated G = H / Hkv times along the head axis: both dtypes and layouts,
d = 32 / 64 / 128 and 80 through a padded cache, Nq = 1 / 3 / 33 / 128, causal and not, per-batch lengths (0, 1, len < Nq, Ncap) with
NaN past the valid rows and past the caches, many splits, Hkv = H bit for bit against the ungrouped entry point, bitwise
repeatability, and the 4-layer model chain with 2 kv heads of 8.  Tolerances: those of tests/test_gpu_decode.py (the per-row
arithmetic is the ungrouped kernel's)."""
import ctypes
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import LENS, TOL, _check, _from_dev, _tdt, _to_dev, _torch

pytestmark = pytest.mark.gpu


def _inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens, coarse=False):
    """fp32 numpy q (B, H, Nq, d), k, v (B, Hkv, Ncap, d) (bf16-rounded for bf16), rows at or past lens[b] of k / v set to NaN.
    ``coarse``, for caches of 10^8 elements: k and v are drawn from the multiples of 2^-7 in (-1, 1) in one int8 pass (exact in bf16;
    a third of the time of the float passes and the rounding)."""
    q, k, v = (rand_u(rng, s) if i == 0 or not coarse else
               np.multiply(rng.integers(-127, 128, s, dtype=np.int8), np.float32(2.0 ** -7), dtype=np.float32)
               for i, s in enumerate(((B, H, Nq, d), (B, Hkv, Ncap, d), (B, Hkv, Ncap, d))))
    if dtype == "bf16":
        q, k, v = (oracle.bf16_round(t) if i == 0 or not coarse else t for i, t in enumerate((q, k, v)))
    for b, n in enumerate(lens):
        n = min(max(n, 0), Ncap)
        k[b, :, n:] = np.nan
        v[b, :, n:] = np.nan
    return q, k, v


def _decode(q, k, v, lens, causal, layout, dtype, dq, dp, nan_buffers=False):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    tq = _to_dev(q, layout, dq, dtype)
    bufs = [None, None]
    if nan_buffers:   # the caches are the front of larger NaN-filled buffers: a read past row Ncap - 1 would see NaN
        n = k.size // k.shape[-1] * dp + 4096 * dp
        bufs = [torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(2)]
    tk, tv = _to_dev(k, layout, dp, dtype, bufs[0]), _to_dev(v, layout, dp, dtype, bufs[1])
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, lse = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=causal, layout=layout)
    torch.cuda.synchronize()
    return _from_dev(out, layout), to_np(lse)


def _check_grouped(q, k, v, lens, causal, dtype, out, lse, heads=None):
    """The reference of a grouped call: decode_reference on k and v repeated G times along the head axis (query head h reads kv head
    h // G)."""
    G = q.shape[1] // k.shape[1]
    _check(q, np.repeat(k, G, axis=1), np.repeat(v, G, axis=1), lens, causal, dtype, out, lse, heads=heads)


@pytest.mark.parametrize("heads", [(8, 2), (8, 1), (6, 3)], ids=lambda t: f"H{t[0]}kv{t[1]}")
@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_decode_matches_fp64_reference(dtype, layout, d, heads):
    H, Hkv = heads
    rng = np.random.default_rng(1000 * H + 100 * Hkv + d + (7 if dtype == "bf16" else 0))
    B, Ncap = len(LENS), 520
    dp = {80: 128}.get(d, d)
    for Nq in (1, 3, 33):
        for causal in (True, False):
            q, k, v = _inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, LENS)
            out, lse = _decode(q, k, v, LENS, causal, layout, dtype, d, dp, nan_buffers=True)
            _check_grouped(q, k, v, LENS, causal, dtype, out, lse)
            # an empty batch element: out = 0, lse = -inf in every head of every group
            assert np.all(out[0] == 0) and np.all(np.isneginf(lse[0]))


@pytest.mark.parametrize("dtype,d", [("bf16", 128), ("f32", 64)])
def test_128_queries_of_8_grouped_heads_over_many_splits(dtype, d):
    """G * Nq = 1024 rows = 32 row blocks per kv head, causal, on a cache long enough for many splits."""
    from flash_attention_minitorch_amd import _lib
    B, H, Hkv, Nq, Ncap = 1, 8, 1, 128, 16384
    assert _lib.decode().fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, 1 if dtype == "bf16" else 0) > 8
    rng = np.random.default_rng(12)
    for lens in (None, [9000]):
        q, k, v = _inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens or [Ncap])
        out, lse = _decode(q, k, v, lens, True, "bnhd", dtype, d, d)
        _check_grouped(q, k, v, lens, True, dtype, out, lse)


@pytest.mark.parametrize("dtype,d", [("bf16", 128), ("f32", 64)])
def test_single_query_of_grouped_heads_over_a_long_cache(dtype, d):
    from flash_attention_minitorch_amd import _lib
    B, H, Hkv, Ncap = 1, 8, 2, 65536
    assert _lib.decode().fa_mi355x_decode_splits_gqa(B, H, Hkv, 1, Ncap, d, 1 if dtype == "bf16" else 0) > 1
    rng = np.random.default_rng(13)
    for lens, causal, layout in ((None, True, "bnhd"), ([40000], False, "bhnd")):
        q, k, v = _inputs(rng, dtype, B, H, Hkv, 1, Ncap, d, lens or [Ncap])
        out, lse = _decode(q, k, v, lens, causal, layout, dtype, d, d)
        _check_grouped(q, k, v, lens, causal, dtype, out, lse)


def _raw(sym, heads, tq, tk, tv, lens, ws, B, Nq, Ncap, d, layout, causal, dtype, out=None, lse=None, null_lse=False):
    """A direct call of one of the two C entry points on the same tensors; returns (out, lse): fresh NaN-filled ones unless the caller
    supplies them; ``null_lse`` passes lse = NULL and returns (out, None)."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    lib = _lib.decode()
    if out is None:
        out = torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda")
    H = heads[0]
    if null_lse:
        lse = None
    elif lse is None:
        lse = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    _lib.decode_check(getattr(lib, sym)(p(tq), p(tk), p(tv), p(out), p(lse), p(lens), p(ws), B, *heads, Nq, Ncap, d,
                                        _lib.FA_LAYOUT_BNHD if layout == "bnhd" else _lib.FA_LAYOUT_BHND, 0.0, int(causal),
                                        1 if dtype == "bf16" else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_heads_through_the_gqa_entry_point_equal_the_ungrouped_one_bitwise(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    lib = _lib.decode()
    rng = np.random.default_rng(14)
    code = 1 if dtype == "bf16" else 0
    # one split (a cache of one chunk), many splits with a query block past 32 rows, and the ragged lengths over three splits
    for (B, H, Nq, Ncap, d, layout, lens) in ((2, 4, 1, 200, 64, "bnhd", None), (1, 2, 33, 20000, 128, "bhnd", [17001]),
                                              (len(LENS), 3, 3, 520, 32, "bnhd", LENS)):
        ns = lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, code)
        assert ns == lib.fa_mi355x_decode_splits_gqa(B, H, H, Nq, Ncap, d, code)
        assert (ns == 1) == (Ncap == 200)
        q, k, v = _inputs(rng, dtype, B, H, H, Nq, Ncap, d, lens or [Ncap] * B)
        tq, tk, tv = (_to_dev(t, layout, d, dtype) for t in (q, k, v))
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        nbytes = lib.fa_mi355x_decode_workspace_bytes(B, H, Nq, Ncap, d)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device="cuda")
        for causal in (True, False):
            old = _raw("fa_mi355x_fwd_decode", (H,), tq, tk, tv, tl, ws, B, Nq, Ncap, d, layout, causal, dtype)
            new = _raw("fa_mi355x_fwd_decode_gqa", (H, H), tq, tk, tv, tl, ws, B, Nq, Ncap, d, layout, causal, dtype)
            assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
            assert not torch.isnan(new[0]).any()


def test_repeated_grouped_calls_are_bitwise_identical():
    rng = np.random.default_rng(15)
    for dtype, (B, H, Hkv, Nq, Ncap) in (("bf16", (1, 8, 2, 5, 20000)), ("f32", (16, 8, 1, 1, 2048))):
        q, k, v = _inputs(rng, dtype, B, H, Hkv, Nq, Ncap, 128, [Ncap] * B)
        a = _decode(q, k, v, None, True, "bnhd", dtype, 128, 128)
        b = _decode(q, k, v, None, True, "bnhd", dtype, 128, 128)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_grouped_call_equals_the_ungrouped_call_on_the_expanded_cache():
    """The row mapping changes where a row sits in the tile, not what it computes: with one split for both calls (a cache of one
    chunk) and no causal tile skipped in either (no mask at Nq = 3; at Nq = 1 every row sits at the last position), each row sees the
    same keys in the same order and the grouped call reproduces the expanded-cache call's bits."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    rng = np.random.default_rng(16)
    B, H, Hkv, Ncap, d = 3, 8, 2, 200, 64
    lib = _lib.decode()
    for dtype, Nq, causal in (("f32", 3, False), ("bf16", 3, False), ("f32", 1, True), ("bf16", 1, True)):
        assert lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, 0) == lib.fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, 0) == 1
        q, k, v = _inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, [200, 77, 2])
        tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
        tl = torch.tensor([200, 77, 2], dtype=torch.int32, device="cuda")
        got = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=causal)
        ke, ve = (t.repeat_interleave(H // Hkv, dim=2).contiguous() for t in (tk, tv))
        ref = device_ops.flash_attn_decode(tq, ke, ve, tl, causal=causal)
        torch.cuda.synchronize()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_prefill_then_steps_match_the_full_attention_stack(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(17)
    B, E, H, Hkv, P, S, T, L = 2, 256, 8, 2, 40, 5, 4, 4
    d = E // H
    tdt = _tdt(dtype)
    x = torch.from_numpy(rand_u(rng, (B, P + S + 2 * T, E))).to("cuda", tdt)
    w = lambda cols: torch.from_numpy(rand_u(rng, (E, cols)) / np.float32(math.sqrt(E))).to("cuda", tdt)
    layers = [(w(E), w(Hkv * d), w(Hkv * d), w(E)) for _ in range(L)]
    full = to_np(mt.attention_stack(x, layers, H, causal=True))
    cache = mt.KVCache(L, B, 128, H, d, tdt, "cuda", n_kv_head=Hkv)
    assert cache.k[0].shape[2] == Hkv and cache.v[0].shape == (B, 128, Hkv, d)
    pre = mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    got = [to_np(pre)]
    for i in range(S):
        got.append(to_np(mt.attention_stack_step(x[:, P + i:P + i + 1].contiguous(), layers, H, cache)))
    for j in range(2):
        a = P + S + j * T
        got.append(to_np(mt.attention_stack_step(x[:, a:a + T].contiguous(), layers, H, cache)))
    got = np.concatenate(got, axis=1)
    tol = (2e-4 if dtype == "f32" else 2e-2) * max(1.0, float(np.max(np.abs(full))))
    print(f"grouped stack {dtype}: max-abs {maxabs(got, full):.3e} (bound {tol:.3e})")
    assert maxabs(got, full) < tol, (maxabs(got, full), tol)
    assert int(cache.lengths.min()) == int(cache.lengths.max()) == P + S + 2 * T
    # the unfused layout and the autograd path take the same grouped weights (k and v expanded in front of the operator)
    unfused = to_np(mt.attention_stack(x, layers, H, causal=True, fused_layout=False))
    assert maxabs(unfused, full) < tol


def test_grouped_multi_head_attention_sums_the_group_gradients():
    """multi_head_attention with (E, Hkv * d) weights equals the same call with the weights' columns repeated per group, values and
    gradients: autograd's backward of the expansion sums the G heads' dK / dV."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(18)
    B, N, E, H, Hkv = 2, 96, 128, 4, 2
    d, G = E // H, 2
    t = lambda *s: torch.from_numpy(rand_u(rng, s) / np.float32(math.sqrt(E))).to("cuda")
    x, wq, wo = t(B, N, E), t(E, E), t(E, E)
    wk, wv = t(E, Hkv * d).requires_grad_(), t(E, Hkv * d).requires_grad_()
    wide = lambda m: m.view(E, Hkv, 1, d).expand(E, Hkv, G, d).reshape(E, E)
    y = mt.multi_head_attention(x, wq, wk, wv, wo, H)
    y.square().sum().backward()
    gk, gv = wk.grad.clone(), wv.grad.clone()
    wk.grad = wv.grad = None
    y2 = mt.multi_head_attention(x, wq, wide(wk), wide(wv), wo, H)
    y2.square().sum().backward()
    scale = max(1.0, float(gk.abs().max()), float(gv.abs().max()))
    assert maxabs(to_np(y), to_np(y2)) < 1e-5
    assert maxabs(to_np(gk), to_np(wk.grad)) < 1e-4 * scale and maxabs(to_np(gv), to_np(wv.grad)) < 1e-4 * scale
