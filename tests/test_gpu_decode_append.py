"""The fused KV-cache append on the GPU (fa_mi355x_decode_append / fa_mi355x_fwd_decode_append, include/flash_attn_mi355x_decode.h).
The append alone, bit for bit against the placement rule of tests/test_decode_append_cpu.py: both dtypes and layouts, d = 32 / 64 /
128, short rows (d_new < d, an odd d_new and unaligned sources on the element path), Nq = 1 / 3 / 128, lengths 0, below Nq, full and
out of range, sentinel rows and NaN columns.  The fused call against decode_append + flash_attn_decode (bitwise) and the fp64
reference, repeatability, NaN in the rows it overwrites, graph capture with lengths advanced on the device; and the model's step,
eager and captured (GraphedStep), against attention_stack over the whole sequence."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_decode_append_cpu import append_reference
from test_gpu_decode import TOL, _check, _inputs, _tdt, _to_dev, _torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 300, 520, 9999]   # Ncap = 520: nothing to write, len < Nq (Nq = 3, 128), interior, full, out of range
NCAP = 520


def _bits(t):
    torch = _torch()
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _dev(x, layout, dtype):
    """(B, N, H, d) numpy -> contiguous device tensor, (B, N, H, d) for "bnhd" or (B, H, N, d) for "bhnd" (no padding)."""
    return _to_dev(x.transpose(0, 2, 1, 3), layout, x.shape[-1], dtype)


def _new_and_cache(rng, dtype, B, Nq, Hkv, Ncap, d, d_new):
    """k_new, v_new (B, Nq, Hkv, d_new) and sentinel caches (B, Ncap, Hkv, d): random values with NaN in columns d_new .. d-1 (and in
    column 0 of every seventh row), all exactly representable in `dtype`."""
    rnd = (lambda s: oracle.bf16_round(rand_u(rng, s))) if dtype == "bf16" else (lambda s: rand_u(rng, s))
    new = [rnd((B, Nq, Hkv, d_new)) for _ in range(2)]
    caches = [rnd((B, Ncap, Hkv, d)) for _ in range(2)]
    for c in caches:
        c[..., d_new:] = np.nan
        c[:, ::7, :, 0] = np.nan
    return new, caches


@pytest.mark.parametrize("d,d_new", [(32, 32), (64, 64), (128, 128), (32, 20), (128, 65), (64, 56)])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_append_places_rows_bit_for_bit(dtype, layout, d, d_new):
    """(d_new = 56 of bf16 is 112 bytes, a multiple of 16 with zero columns behind it: the vector path's zero lanes; 20 of bf16 and 65
    take the element path, 20 of f32 the vector path.)"""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(d + d_new)
    B = len(LENS)
    tl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    for Nq in (1, 3, 128):
        for Hkv in (1, 3):
            (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, NCAP, d, d_new)
            tkc, tvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
            device_ops.decode_append(_dev(kn, layout, dtype), _dev(vn, layout, dtype), tkc, tvc, tl, layout=layout)
            for got, new, cache in ((tkc, kn, kc), (tvc, vn, vc)):
                want = append_reference(new, cache, LENS, Nq)
                assert torch.equal(_bits(got), _bits(_dev(want, layout, dtype))), (Nq, Hkv)
                # the reference itself says: written rows end in exact zeros where the cache held NaN, batch element 5 (out of range
                # = full) holds the tokens in its last rows, and its neighbour's rows in front of it (element 4 is full too) are
                # the sentinel's
                assert np.all(want[4, NCAP - min(Nq, NCAP):, :, d_new:] == 0) and np.array_equal(want[5, NCAP - Nq:, :, :d_new], new[5])
                assert np.array_equal(np.isnan(want[5, :NCAP - Nq]), np.isnan(cache[5, :NCAP - Nq]))
                assert np.all(np.isnan(want[0]) == np.isnan(cache[0]))   # len = 0: untouched


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_append_without_lengths_and_from_unaligned_sources(dtype):
    """No cache_seqlens: the last Nq rows.  Sources that start 2 or 4 bytes past a 16-byte boundary take the element path."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(1)
    B, Nq, Hkv, Ncap, d = 2, 5, 3, 40, 64
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, Ncap, d, d)
    for layout in ("bnhd", "bhnd"):
        for shift in (0, 1):
            news = []
            for x in (kn, vn):
                t = _dev(x, layout, dtype)
                buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
                view = buf[shift:shift + t.numel()].view(t.shape)
                view.copy_(t)
                assert view.is_contiguous() and view.data_ptr() % 16 == shift * t.element_size()
                news.append(view)
            tkc, tvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
            device_ops.decode_append(news[0], news[1], tkc, tvc, None, layout=layout)
            assert torch.equal(_bits(tkc), _bits(_dev(append_reference(kn, kc, None, Nq), layout, dtype)))
            assert torch.equal(_bits(tvc), _bits(_dev(append_reference(vn, vc, None, Nq), layout, dtype)))


# (B, H, Hkv, Nq, Ncap, d, d_new, lens, splits): G = 1 and G = 4, one split and many
FUSED = [
    (3, 4, 4, 3, 200, 64, 64, [200, 2, 77], 1),
    (3, 8, 2, 3, 200, 64, 48, [200, 2, 77], 1),
    (1, 8, 8, 1, 4096, 128, 128, [3000], 16),
    (1, 8, 2, 5, 4096, 128, 128, [4096], 16),
]


def _fused_case(rng, dtype, B, H, Hkv, Nq, Ncap, d, d_new, lens):
    """q (B, H, Nq, d_new) numpy, the new tokens and sentinel caches of _new_and_cache with NaN also in every row from the first one
    the append writes (rows at or past len - Nq: the rows about to be written, and the invalid ones behind them)."""
    q = rand_u(rng, (B, H, Nq, d_new))
    if dtype == "bf16":
        q = oracle.bf16_round(q)
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, Ncap, d, d_new)
    for b, n in enumerate(lens):
        for c in (kc, vc):
            c[b, max(min(n, Ncap) - Nq, 0):] = np.nan
            c[b, :max(min(n, Ncap) - Nq, 0), :, d_new:] = 0   # (valid older rows: zero columns, as a padded cache holds them)
            c[b, :max(min(n, Ncap) - Nq, 0):7, :, 0] = 0.25
    return q, kn, vn, kc, vc


@pytest.mark.parametrize("case", FUSED, ids=[f"B{c[0]}-H{c[1]}-Hkv{c[2]}-Nq{c[3]}-Ncap{c[4]}-d{c[6]}in{c[5]}" for c in FUSED])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_call_is_append_then_decode(dtype, case):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    B, H, Hkv, Nq, Ncap, d, d_new, lens, ns = case
    assert _lib.decode().fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, 1 if dtype == "bf16" else 0) == ns
    rng = np.random.default_rng(B + H + Ncap)
    q, kn, vn, kc, vc = _fused_case(rng, dtype, B, H, Hkv, Nq, Ncap, d, d_new, lens)
    tq, tkn, tvn = _to_dev(q, "bnhd", d_new, dtype), _dev(kn, "bnhd", dtype), _dev(vn, "bnhd", dtype)
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    runs = []
    for fused in (True, True, False):
        tkc, tvc = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
        if fused:
            out, lse = device_ops.flash_attn_decode(tq, tkc, tvc, tl, causal=True, k_new=tkn, v_new=tvn)
        else:
            device_ops.decode_append(tkn, tvn, tkc, tvc, tl)
            out, lse = device_ops.flash_attn_decode(tq, tkc, tvc, tl, causal=True)
        runs.append((out, lse, tkc, tvc))
    torch.cuda.synchronize()
    for other in runs[1:]:   # a repeated fused call, then the two separate calls: the same bits
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    # the appended caches are the rule's, and the results the fp64 reference's on them: finite, although the rows held NaN
    want_k, want_v = append_reference(kn, kc, lens, Nq), append_reference(vn, vc, lens, Nq)
    assert torch.equal(_bits(runs[0][2]), _bits(_dev(want_k, "bnhd", dtype))) and torch.equal(_bits(runs[0][3]), _bits(_dev(want_v, "bnhd", dtype)))
    out, lse = to_np(runs[0][0]).transpose(0, 2, 1, 3), to_np(runs[0][1])
    assert out.shape == q.shape and np.all(np.isfinite(out)) and not np.any(np.isnan(lse))
    G = H // Hkv
    ke, ve = (np.repeat(t.transpose(0, 2, 1, 3)[..., :d_new], G, axis=1) for t in (want_k, want_v))   # (B, H, Ncap, d_new)
    _check(q, ke, ve, lens, True, dtype, out, lse)


def test_fused_call_replays_in_a_graph_with_lengths_advanced_on_the_device():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(12)
    B, H, Hkv, Nq, Ncap, d, steps = 2, 8, 2, 1, 4096, 128, 3
    start = [3000, 17]
    q, kn, vn, kc, vc = _fused_case(rng, "bf16", B, H, Hkv, Nq * (steps + 1), Ncap, d, d, [s + steps + 1 for s in start])
    dev = lambda x: _dev(x, "bnhd", "bf16")
    tq_all, tkn_all, tvn_all = _to_dev(q, "bnhd", d, "bf16"), dev(kn), dev(vn)   # (B, steps + 1, heads, d): one token per step
    sq, sk, sv = (t[:, :1].contiguous() for t in (tq_all, tkn_all, tvn_all))    # the graph's static inputs
    ws = device_ops.decode_workspace(sq, dev(kc))
    assert ws is not None

    def run(caches, lens, out, lse):
        return device_ops.flash_attn_decode(sq, caches[0], caches[1], lens, causal=True, out=out, lse=lse, workspace=ws, k_new=sk, v_new=sv)

    def feed(i):
        for dst, src in ((sq, tq_all), (sk, tkn_all), (sv, tvn_all)):
            dst.copy_(src[:, i:i + 1])

    new_out = lambda: (torch.empty(sq.shape, dtype=torch.float32, device="cuda"), torch.empty((B, H, 1), dtype=torch.float32, device="cuda"))
    # eager: three calls, the lengths advanced on the device in between
    eager_c, eager_l, eager = (dev(kc), dev(vc)), torch.tensor(start, dtype=torch.int32, device="cuda"), []
    for i in range(steps):
        feed(i)
        eager_l.add_(1)
        o, l = run(eager_c, eager_l, *new_out())
        eager.append((o.clone(), l.clone()))
    # captured: a warm-up call on a side stream (on token `steps`, at the length the first replay uses: its row is written again)
    graph_c, graph_l = (dev(kc), dev(vc)), torch.tensor(start, dtype=torch.int32, device="cuda")
    out, lse = new_out()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        feed(steps)
        graph_l.add_(1)
        run(graph_c, graph_l, out, lse)
        graph_l.sub_(1)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph_l.add_(1)
        run(graph_c, graph_l, out, lse)
    for i in range(steps):
        feed(i)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i][0]) and torch.equal(lse, eager[i][1]), i
    assert torch.equal(graph_l, eager_l) and graph_l.tolist() == [s + steps for s in start]
    for a, b in zip(graph_c, eager_c):
        assert torch.equal(_bits(a), _bits(b))


def _stack(rng, dtype, B, E, H, Hkv, L, n_tokens):
    torch = _torch()
    tdt = _tdt(dtype)
    d = E // H
    x = torch.from_numpy(rand_u(rng, (B, n_tokens, E))).to("cuda", tdt)
    layers = [tuple(torch.from_numpy(rand_u(rng, (E, c)) / np.float32(math.sqrt(E))).to("cuda", tdt) for c in (E, Hkv * d, Hkv * d, E))
              for _ in range(L)]
    return x, layers


# (E, heads, kv heads): head_dim 64 ungrouped, and head_dim 48 (E = 4 * 48) with 2 kv heads: d_new = 48 into rows of dp = 64
MODELS = [(256, 4, 4), (192, 4, 2)]


@pytest.mark.parametrize("E,H,Hkv", MODELS, ids=["E256-h4-kv4", "E192-h4-kv2-d48"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prefill_then_graphed_steps_match_the_full_attention_stack(dtype, E, H, Hkv):
    """Prompts of 40 and 33 tokens in one batch (lengths differ per batch element), then 5 captured steps; every batch element against
    attention_stack over its own whole sequence, at the tolerance of test_prefill_then_steps_match_the_full_attention_stack.  A
    second cache stepped eagerly with the fused step, and a third with attention_stack_step (the caller-side append), end with the
    same bits, and the three steps return the same bits."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(E + H)
    B, P, S, L = 2, 40, 5, 4
    prompts = [P, P - 7]
    x, layers = _stack(rng, dtype, B, E, H, Hkv, L, P + S)
    tdt = _tdt(dtype)
    caches = [mt.KVCache(L, B, 64, H, E // H, tdt, "cuda", n_kv_head=Hkv) for _ in range(3)]
    outs = []
    for cache in caches:
        # the shorter prompt is the front of its row: its cache rows past 33 are invalid, and lengths says so
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
        cache.lengths.copy_(torch.tensor(prompts, dtype=torch.int32))
    graphed = mt.GraphedStep(layers, H, caches[0], 1)
    for i in range(S):
        xi = x[:, P + i:P + i + 1].contiguous()
        outs.append((to_np(graphed.step(xi)), to_np(mt.attention_stack_step_fused(xi, layers, H, caches[1])),
                     to_np(mt.attention_stack_step(xi, layers, H, caches[2]))))
    got, eager, unfused = (np.concatenate([o[j] for o in outs], axis=1) for j in range(3))
    for b, p in enumerate(prompts):
        seq = torch.cat([x[b:b + 1, :p], x[b:b + 1, P:]], dim=1).contiguous()
        # (head_dim 48 is no native row length of the [B][N][H][d] forward: that stack runs the head-split layout, the same function)
        full = to_np(mt.attention_stack(seq, layers, H, causal=True, fused_layout=E // H in (32, 64, 128)))[0, p:]
        tol = (2e-4 if dtype == "f32" else 2e-2) * max(1.0, float(np.max(np.abs(full))))
        assert maxabs(got[b], full) < tol, (b, maxabs(got[b], full), tol)
        assert maxabs(eager[b], full) < tol, (b, maxabs(eager[b], full), tol)
    assert np.array_equal(got, eager) and np.array_equal(eager, unfused)
    for cache in caches[1:]:
        assert caches[0].lengths.tolist() == cache.lengths.tolist() == [p + S for p in prompts]
        assert caches[0].length_bound == cache.length_bound == P + S
        for a, b in zip(caches[0].k + caches[0].v, cache.k + cache.v):
            assert torch.equal(_bits(a), _bits(b))
    # the new rows' padding columns are zero, written by the library
    if caches[0].dp > E // H:
        assert all(bool((t[..., E // H:] == 0).all()) for t in caches[0].k + caches[0].v)


def test_graphed_step_checks_its_input_and_the_capacity():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(3)
    B, E, H, L, P = 2, 128, 2, 2, 6
    x, layers = _stack(rng, "bf16", B, E, H, H, L, P + 3)
    cache = mt.KVCache(L, B, P + 2, H, E // H, torch.bfloat16, "cuda")
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    g = mt.GraphedStep(layers, H, cache, 1)
    with pytest.raises(ValueError, match="tokens at a time"):
        g.step(x[:, P:P + 2].contiguous())
    for i in range(2):
        g.step(x[:, P + i:P + i + 1].contiguous())
    assert cache.length_bound == P + 2 and cache.lengths.tolist() == [P + 2] * B
    with pytest.raises(ValueError, match="capacity"):
        g.step(x[:, P + 2:P + 3].contiguous())
    with pytest.raises(ValueError, match="tokens"):
        mt.GraphedStep(layers, H, cache, 129)
