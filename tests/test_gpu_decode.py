"""KV-cache decode attention on the GPU (fa_mi355x_fwd_decode, include/flash_attn_mi355x_decode.h) against the fp64 decode reference of
tests/test_decode_cpu.py on the same (bf16-rounded) inputs: both dtypes and layouts, d = 32 / 64 / 128 and 80 through a padded cache,
Nq up to 128, causal and not, per-batch lengths (0, 1, len < Nq, Ncap, out of range), NaN past the valid rows, many splits, bitwise
repeatability, parity with the existing causal forward, graph capture and the 4-layer model chain."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_decode_cpu import decode_reference

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "bf16": 1e-3}


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _inputs(rng, dtype, B, H, Nq, Ncap, d, lens, scale_in=1.0):
    """fp32 numpy q (B, H, Nq, d), k, v (B, H, Ncap, d) (bf16-rounded for bf16), rows at or past lens[b] of k / v set to NaN."""
    q, k, v = (rand_u(rng, s) * np.float32(scale_in) for s in ((B, H, Nq, d), (B, H, Ncap, d), (B, H, Ncap, d)))
    if dtype == "bf16":
        q, k, v = (oracle.bf16_round(t) for t in (q, k, v))
    for b, n in enumerate(lens):
        n = min(max(n, 0), Ncap)
        k[b, :, n:] = np.nan
        v[b, :, n:] = np.nan
    return q, k, v


def _to_dev(t, layout, dp, dtype, buf=None):
    """(B, H, N, d) numpy -> a contiguous device tensor in `layout` with zero columns up to dp; with `buf`, a view of buf's front."""
    torch = _torch()
    x = torch.from_numpy(np.ascontiguousarray(t))
    x = torch.nn.functional.pad(x, (0, dp - t.shape[-1]))
    if layout == "bnhd":
        x = x.transpose(1, 2)
    x = x.contiguous().to("cuda", _tdt(dtype))
    if buf is None:
        return x
    view = buf[:x.numel()].view(x.shape)
    view.copy_(x)
    return view


def _from_dev(out, layout):
    o = to_np(out)
    return o.transpose(0, 2, 1, 3) if layout == "bnhd" else o


def _decode(q, k, v, lens, causal, layout, dtype, dq, dp, scale=None, nan_buffers=False):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    tq = _to_dev(q, layout, dq, dtype)
    bufs = [None, None]
    if nan_buffers:   # the caches are the front of larger NaN-filled buffers: a read past row Ncap - 1 would see NaN
        n = k.size // k.shape[-1] * dp + 4096 * dp
        bufs = [torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(2)]
    tk, tv = _to_dev(k, layout, dp, dtype, bufs[0]), _to_dev(v, layout, dp, dtype, bufs[1])
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, lse = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=causal, softmax_scale=scale, layout=layout)
    torch.cuda.synchronize()
    return _from_dev(out, layout), to_np(lse)


def _check(q, k, v, lens, causal, dtype, out, lse, heads=None, scale=None, tol=None):
    B, H, Nq, d = q.shape
    scale = scale or 1.0 / math.sqrt(d)
    lens_bh = np.repeat(np.asarray(lens if lens is not None else [k.shape[2]] * B), H)
    qf, kf, vf = (t.reshape(B * H, t.shape[2], d) for t in (q, k, v))
    of, lf = out.reshape(B * H, Nq, d), lse.reshape(B * H, Nq)
    heads = range(B * H) if heads is None else heads
    for hh in heads:
        ro, rl = decode_reference(qf[hh:hh + 1], kf[hh:hh + 1], vf[hh:hh + 1], lens_bh[hh:hh + 1], causal, scale)
        assert np.all(np.isfinite(of[hh])), hh
        assert np.array_equal(np.isneginf(lf[hh]), np.isneginf(rl[0])), (hh, lf[hh], rl[0])
        fin = np.isfinite(rl[0])
        assert maxabs(of[hh], ro[0]) < (tol or TOL[dtype]), (hh, maxabs(of[hh], ro[0]))
        if fin.any():
            assert maxabs(lf[hh][fin], rl[0][fin]) < (tol or TOL[dtype]), hh


LENS = [0, 1, 31, 257, 520, 2]   # Ncap = 520; with Nq = 3 the lengths 1 and 2 are shorter than Nq


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_matches_fp64_reference(dtype, layout, d):
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0))
    B, H, Ncap = len(LENS), 2, 520
    dp = {80: 128}.get(d, d)
    for Nq, causal in ((1, True), (3, True), (3, False), (32, True), (33, False), (128, True)):
        q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, LENS)
        out, lse = _decode(q, k, v, LENS, causal, layout, dtype, d, dp)
        _check(q, k, v, LENS, causal, dtype, out, lse)


@pytest.mark.parametrize("dtype,d", [("bf16", 128), ("f32", 64)])
def test_long_cache_takes_many_splits(dtype, d):
    from flash_attention_minitorch_amd import _lib
    B, H, Ncap = 1, 2, 65536
    assert _lib.decode().fa_mi355x_decode_splits(B, H, 1, Ncap, d, 1 if dtype == "bf16" else 0) > 1
    rng = np.random.default_rng(11)
    for lens, causal in ((None, True), ([40000], False)):
        q, k, v = _inputs(rng, dtype, B, H, 1, Ncap, d, lens or [Ncap])
        out, lse = _decode(q, k, v, lens, causal, "bnhd", dtype, d, d)
        _check(q, k, v, lens, causal, dtype, out, lse)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_out_of_range_lengths_clamp_and_nan_rows_never_leak(dtype):
    rng = np.random.default_rng(5)
    B, H, Nq, Ncap, d = 2, 3, 4, 700, 64
    for layout in ("bnhd", "bhnd"):
        q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, [Ncap, 0])
        for causal in (True, False):
            ref = _decode(q, k, v, [Ncap, 0], causal, layout, dtype, d, d, nan_buffers=True)
            got = _decode(q, k, v, [Ncap + 7, -3], causal, layout, dtype, d, d, nan_buffers=True)
            assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
            _check(q, k, v, [Ncap, 0], causal, dtype, got[0], got[1])
            assert np.all(got[0][1] == 0) and np.all(np.isneginf(got[1][1]))


def test_repeated_calls_are_bitwise_identical():
    rng = np.random.default_rng(9)
    for dtype, (B, H, Nq, Ncap) in (("bf16", (1, 4, 5, 20000)), ("f32", (16, 8, 1, 2048))):
        q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, 128, [Ncap] * B)
        a = _decode(q, k, v, None, True, "bnhd", dtype, 128, 128)
        b = _decode(q, k, v, None, True, "bnhd", dtype, 128, 128)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_matches_last_rows_of_the_causal_forward(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    rng = np.random.default_rng(2)
    B, H, N, d = 2, 4, 1000, 64
    for Nq in (1, 17, 128):
        q, k, v = _inputs(rng, dtype, B, H, N, N, d, [N] * B)
        tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
        o, l, _ = device_ops.flash_attn_fwd_bnhd(tq, tk, tv, True, _lib.FA_VARIANT_FA2)
        out, lse = device_ops.flash_attn_decode(tq[:, N - Nq:].contiguous(), tk, tv, None, causal=True)
        torch.cuda.synchronize()
        assert maxabs(to_np(out), to_np(o[:, N - Nq:])) < TOL[dtype]
        assert maxabs(to_np(lse), to_np(l[:, :, N - Nq:])) < TOL[dtype]


def test_folded_scale_convention_and_large_inputs():
    """softmax_scale = ln 2 with log2(e)/sqrt(d) folded into q (multi_head_attention(fold_scale=True)) is the same function; bf16 x6
    inputs stay within 5e-3 x scale (scaling is fp32 on every score)."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(4)
    B, H, Nq, Ncap, d = 2, 4, 2, 900, 64
    q, k, v = _inputs(rng, "f32", B, H, Nq, Ncap, d, [Ncap, 600])
    qf = q * np.float32(math.log2(math.e) / math.sqrt(d))
    out, lse = _decode(qf, k, v, [Ncap, 600], True, "bhnd", "f32", d, d, scale=math.log(2))
    _check(qf, k, v, [Ncap, 600], True, "f32", out, lse, scale=math.log(2))
    q, k, v = _inputs(rng, "bf16", B, H, Nq, Ncap, d, [Ncap, 600], scale_in=6.0)
    out, lse = _decode(q, k, v, [Ncap, 600], True, "bnhd", "bf16", d, d)
    _check(q, k, v, [Ncap, 600], True, "bf16", out, lse, tol=5e-3 * 6.0)
    del torch, device_ops


def test_graph_capture_replays_with_new_cache_contents_and_lengths():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(8)
    B, H, Nq, Ncap, d = 2, 2, 1, 8192, 128
    q, k, v = _inputs(rng, "bf16", B, H, Nq, Ncap, d, [Ncap, Ncap])
    tq, tk, tv = (_to_dev(t, "bnhd", d, "bf16") for t in (q, k, v))
    lens = torch.tensor([5000, 300], dtype=torch.int32, device="cuda")
    ws = device_ops.decode_workspace(tq, tk)
    assert ws is not None
    out = torch.empty(tq.shape, dtype=torch.float32, device="cuda")
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device="cuda")
    call = lambda o, l: device_ops.flash_attn_decode(tq, tk, tv, lens, causal=True, out=o, lse=l, workspace=ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(out, lse)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(out, lse)
    tk.mul_(-0.5)
    tv.copy_(tv.flip(1))
    lens.copy_(torch.tensor([8000, 7], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    ref_o, ref_l = call(None, None)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_o) and torch.equal(lse, ref_l)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prefill_then_steps_match_the_full_attention_stack(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(6)
    B, E, H, P, S, T, L = 2, 256, 8, 40, 5, 4, 4
    tdt = _tdt(dtype)
    x = torch.from_numpy(rand_u(rng, (B, P + S + 2 * T, E))).to("cuda", tdt)
    layers = [tuple(torch.from_numpy(rand_u(rng, (E, E)) / np.float32(math.sqrt(E))).to("cuda", tdt) for _ in range(4))
              for _ in range(L)]
    full = to_np(mt.attention_stack(x, layers, H, causal=True))
    cache = mt.KVCache(L, B, 128, H, E // H, tdt, "cuda")
    pre = mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    got = [to_np(pre)]
    for i in range(S):
        got.append(to_np(mt.attention_stack_step(x[:, P + i:P + i + 1].contiguous(), layers, H, cache)))
    for j in range(2):
        a = P + S + j * T
        got.append(to_np(mt.attention_stack_step(x[:, a:a + T].contiguous(), layers, H, cache)))
    got = np.concatenate(got, axis=1)
    tol = (2e-4 if dtype == "f32" else 2e-2) * max(1.0, float(np.max(np.abs(full))))
    assert maxabs(got, full) < tol, (maxabs(got, full), tol)
    assert int(cache.lengths.min()) == int(cache.lengths.max()) == P + S + 2 * T
