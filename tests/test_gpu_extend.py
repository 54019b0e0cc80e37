"""The extend call on the GPU (fa_mi355x_fwd_extend / _extend_append / _fwd_extend_append, include/flash_attn_mi355x_decode.h: any
number of new queries against a KV cache) against the fp64 reference of tests/test_decode_cpu.py on the same (bf16-rounded) inputs, at
the project's tolerances (fp32 1e-4, bf16 1e-3 max-abs on out and lse, the -inf pattern of lse exact).  Small shapes at every place
the kernel can go wrong: partial last 32-row and 128-row blocks (Nq = 129, 160, 200, 257) and blocks below its natural size (1, 33),
both dtypes and layouts, d = 32 / 64 / 128 and 80 through the padded cache, per-batch lengths around Nq and around a 128-key tile
with NaN in every invalid row and around the caches, grouped heads, one split and several (counts asserted), repeatability, the
decode call and the square causal forward as second opinions, the append, graph capture, and the model layer."""
import math

import numpy as np
import pytest

from gpu_util import maxabs, rand_u, to_np
from test_decode_append_cpu import append_reference
from test_gpu_decode import TOL, _check, _from_dev, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _new_and_cache, _stack

pytestmark = pytest.mark.gpu

NCAP = 520


def _lens(Nq):
    """Per-batch lengths of one call (Ncap = 520): empty, one key, below Nq, Nq itself (an empty prefix), Nq + 1, a length whose
    last 128-key tile is partial and whose causal diagonal crosses tiles, full, and out of range (clamped to Ncap)."""
    return [0, 1, max(Nq - 1, 0), min(Nq, NCAP), min(Nq + 1, NCAP), 300, NCAP, 9999]


def _splits(B, H, Hkv, Nq, Ncap, d, dtype):
    from flash_attention_minitorch_amd import _lib
    return _lib.decode().fa_mi355x_extend_splits(B, H, Hkv, Nq, Ncap, d, 1 if dtype == "bf16" else 0)


def _grouped_inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens):
    """q (B, H, Nq, d), k and v (B, Hkv, Ncap, d) as test_gpu_decode._inputs makes them (NaN at and past lens[b])."""
    q, _, _ = _inputs(rng, dtype, B, H, Nq, 1, d, [1] * B)
    _, k, v = _inputs(rng, dtype, B, Hkv, 1, Ncap, d, lens)
    return q, k, v


def _nan_buffer(t, dp, dtype):
    torch = _torch()
    return torch.full((t.size // t.shape[-1] * dp + 4096 * dp,), float("nan"), dtype=_tdt(dtype), device="cuda")


def _extend(q, k, v, lens, causal, layout, dtype, dq, dp, scale=None, nan_buffers=True):
    """flash_attn_extend on numpy q (B, H, Nq, d), k / v (B, Hkv, Ncap, d); the caches are the front of larger NaN-filled buffers (a
    read past row Ncap - 1 would see NaN).  Returns numpy (out (B, H, Nq, d), lse (B, H, Nq))."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    tq = _to_dev(q, layout, dq, dtype)
    tk = _to_dev(k, layout, dp, dtype, _nan_buffer(k, dp, dtype) if nan_buffers else None)
    tv = _to_dev(v, layout, dp, dtype, _nan_buffer(v, dp, dtype) if nan_buffers else None)
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, lse = device_ops.flash_attn_extend(tq, tk, tv, tl, causal=causal, softmax_scale=scale, layout=layout)
    torch.cuda.synchronize()
    return _from_dev(out, layout), to_np(lse)


def _check_grouped(q, k, v, lens, causal, dtype, out, lse, heads=None):
    G = q.shape[1] // k.shape[1]
    _check(q, np.repeat(k, G, axis=1), np.repeat(v, G, axis=1), lens, causal, dtype, out, lse, heads=heads)


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_matches_fp64_reference_at_every_length(dtype, layout, d):
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0))
    H, dp = 2, {80: 128}.get(d, d)
    for Nq, causal in ((1, True), (33, False), (129, True), (160, False), (200, True), (257, True), (257, False)):
        lens = _lens(Nq)
        q, k, v = _inputs(rng, dtype, len(lens), H, Nq, NCAP, d, lens)
        out, lse = _extend(q, k, v, lens, causal, layout, dtype, d, dp)
        _check(q, k, v, lens, causal, dtype, out, lse)


# (H, Hkv, Nq): G = 1, 3, 4, 8 with G * Nq = 129, 129, 516, 296, 390 rows (no multiple of 32), multi-query caches among them
GROUPED = [(3, 3, 129), (6, 2, 43), (8, 2, 129), (8, 1, 37), (3, 1, 130)]


@pytest.mark.parametrize("H,Hkv,Nq", GROUPED, ids=[f"H{h}-Hkv{k}-Nq{n}" for h, k, n in GROUPED])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_heads_share_their_kv_head(dtype, H, Hkv, Nq):
    rng = np.random.default_rng(H * 100 + Nq)
    lens = [NCAP, 300, Nq, max(Nq - 5, 0)]
    for layout, causal in (("bnhd", True), ("bhnd", True), ("bnhd", False)):
        q, k, v = _grouped_inputs(rng, dtype, len(lens), H, Hkv, Nq, NCAP, 64, lens)
        out, lse = _extend(q, k, v, lens, causal, layout, dtype, 64, 64)
        _check_grouped(q, k, v, lens, causal, dtype, out, lse)


# (B, H, Hkv, Nq, Ncap, d, splits, lens, every n-th head checked): the counts are pinned in tests/test_extend_cpu.py
SPLIT_SHAPES = [
    (1, 2, 2, 160, 2048, 64, 8, [2048], 1),            # eight chunks of 256 keys: causal rows see 1889 .. 2048 of them
    (1, 2, 2, 160, 2048, 128, 8, [1000], 1),           # ... and chunks wholly past len
    (1, 8, 2, 129, 1300, 64, 6, [1300], 1),            # grouped, five row blocks, the last chunk of 20 keys
    (4, 128, 128, 300, 700, 32, 1, [700, 650, 300, 5], 61),   # no split: one chunk of six super tiles, three row blocks
]


@pytest.mark.parametrize("case", SPLIT_SHAPES, ids=[f"B{c[0]}-H{c[1]}-Hkv{c[2]}-Nq{c[3]}-Ncap{c[4]}-d{c[5]}" for c in SPLIT_SHAPES])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_several_splits_and_one_split_of_several_super_tiles(dtype, case):
    B, H, Hkv, Nq, Ncap, d, ns, lens, step = case
    assert _splits(B, H, Hkv, Nq, Ncap, d, dtype) == ns
    rng = np.random.default_rng(Ncap + d)
    for causal in (True, False):
        q, k, v = _grouped_inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens)
        out, lse = _extend(q, k, v, lens, causal, "bnhd", dtype, d, d)
        _check_grouped(q, k, v, lens, causal, dtype, out, lse, heads=range(0, B * H, step))


def test_repeated_calls_are_bitwise_identical():
    rng = np.random.default_rng(9)
    B, H, Nq, Ncap, d = 2, 4, 200, 1000, 64
    for dtype in ("bf16", "f32"):
        assert _splits(B, H, H, Nq, Ncap, d, dtype) == 4
        q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, [Ncap, 700])
        a = _extend(q, k, v, [Ncap, 700], True, "bnhd", dtype, d, d)
        b = _extend(q, k, v, [Ncap, 700], True, "bnhd", dtype, d, d)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_up_to_128_queries_agree_with_the_decode_call(dtype):
    """Within tolerance, not bitwise: the decode kernel's waves split the keys and merge, the extend kernel's waves walk them in order."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(21)
    B, H, Hkv, Ncap, d = 3, 4, 2, 1300, 64
    lens = [1300, 777, 40]
    for Nq in (1, 33, 128):
        q, k, v = _grouped_inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens)
        tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        o1, l1 = device_ops.flash_attn_extend(tq, tk, tv, tl, causal=True)
        o2, l2 = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=True)
        torch.cuda.synchronize()
        l1, l2 = to_np(l1), to_np(l2)
        assert np.array_equal(np.isneginf(l1), np.isneginf(l2))
        fin = np.isfinite(l2)
        assert maxabs(to_np(o1), to_np(o2)) < TOL[dtype] and maxabs(l1[fin], l2[fin]) < TOL[dtype]


@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_whole_prompt_agrees_with_the_square_causal_forward(dtype, H, Hkv):
    """len = Nq = Ncap, causal: flash_attn_fwd_bnhd (ungrouped) / flash_attn_fwd_gqa on the same tensors."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    rng = np.random.default_rng(2)
    B, N, d = 2, 257, 64
    q, k, v = _grouped_inputs(rng, dtype, B, H, Hkv, N, N, d, [N] * B)
    tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
    fwd = device_ops.flash_attn_fwd_bnhd if H == Hkv else device_ops.flash_attn_fwd_gqa
    o, l, _ = fwd(tq, tk, tv, True, _lib.FA_VARIANT_FA2)
    out, lse = device_ops.flash_attn_extend(tq, tk, tv, None, causal=True)
    torch.cuda.synchronize()
    assert maxabs(to_np(out), to_np(o)) < TOL[dtype] and maxabs(to_np(lse), to_np(l)) < TOL[dtype]
    _check_grouped(q, k, v, None, True, dtype, _from_dev(out, "bnhd"), to_np(lse))


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_append_of_200_tokens_and_the_fused_call(dtype, layout):
    """extend_append against a torch index_copy_ of the padded rows (and the placement rule of tests/test_decode_append_cpu.py), bit
    for bit, every other row untouched; flash_attn_extend(k_new=, v_new=) returns the bits of append-then-attend, and the fp64
    reference's values although the rows it wrote held NaN."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(31)
    B, H, Hkv, Nq, d, d_new = 3, 4, 2, 200, 64, 48
    lens = [NCAP, 333, Nq]
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, NCAP, d, d_new)
    for b, n in enumerate(lens):   # valid older rows: finite, zero columns past d_new, as a padded cache holds them
        for c in (kc, vc):
            c[b, :n - Nq, :, d_new:] = 0
            c[b, :n - Nq:7, :, 0] = 0.25
    q = _inputs(rng, dtype, B, H, Nq, 1, d_new, [1] * B)[0]
    tq, tkn, tvn = _to_dev(q, layout, d_new, dtype), _dev(kn, layout, dtype), _dev(vn, layout, dtype)
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    # the append alone, against index_copy_ on the (B * Ncap, Hkv, d) view of a "bnhd" copy
    tkc, tvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
    device_ops.extend_append(tkn, tvn, tkc, tvc, tl, layout=layout)
    rows = ((tl.long() - Nq + torch.arange(B, device="cuda") * NCAP)[:, None] + torch.arange(Nq, device="cuda")).reshape(B * Nq)
    for got, new, cache in ((tkc, kn, kc), (tvc, vn, vc)):
        want = _dev(cache, "bnhd", dtype)
        padded = torch.nn.functional.pad(_dev(new, "bnhd", dtype), (0, d - d_new))
        want.view(B * NCAP, Hkv, d).index_copy_(0, rows, padded.reshape(B * Nq, Hkv, d))
        if layout == "bhnd":
            want = want.transpose(1, 2).contiguous()
        assert torch.equal(_bits(got), _bits(want))
        assert torch.equal(_bits(got), _bits(_dev(append_reference(new, cache, lens, Nq), layout, dtype)))
    out2, lse2 = device_ops.flash_attn_extend(tq, tkc, tvc, tl, causal=True, layout=layout)
    # the fused call on fresh caches
    fkc, fvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
    out1, lse1 = device_ops.flash_attn_extend(tq, fkc, fvc, tl, causal=True, layout=layout, k_new=tkn, v_new=tvn)
    torch.cuda.synchronize()
    for a, b in ((out1, out2), (lse1, lse2), (fkc, tkc), (fvc, tvc)):
        assert torch.equal(_bits(a), _bits(b))
    want_k, want_v = append_reference(kn, kc, lens, Nq), append_reference(vn, vc, lens, Nq)
    ke, ve = (t.transpose(0, 2, 1, 3)[..., :d_new] for t in (want_k, want_v))   # (B, Hkv, Ncap, d_new)
    _check_grouped(q, ke, ve, lens, True, dtype, _from_dev(out1, layout), to_np(lse1))


def test_one_call_captured_in_a_graph_replays_the_eager_bits():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(8)
    B, H, Nq, Ncap, d = 2, 4, 200, 1000, 64
    assert _splits(B, H, H, Nq, Ncap, d, "bf16") == 4
    q, k, v = _inputs(rng, "bf16", B, H, Nq, Ncap, d, [Ncap, Ncap])
    tq, tk, tv = (_to_dev(t, "bnhd", d, "bf16") for t in (q, k, v))
    lens = torch.tensor([900, 250], dtype=torch.int32, device="cuda")
    ws = device_ops.extend_workspace(tq, tk)
    assert ws is not None
    out = torch.empty(tq.shape, dtype=torch.float32, device="cuda")
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device="cuda")
    call = lambda o, l: device_ops.flash_attn_extend(tq, tk, tv, lens, causal=True, out=o, lse=l, workspace=ws)
    call(out, lse)   # (the library is loaded and has launched once before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream: the split launch, then the combine launch
        call(out, lse)
    tk.mul_(-0.5)
    lens.copy_(torch.tensor([1000, 201], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    ref_o, ref_l = call(None, None)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_o) and torch.equal(lse, ref_l)


def _model_tol(dtype, full):
    """The tolerance of test_prefill_then_steps_match_the_full_attention_stack (tests/test_gpu_decode.py) for a 4-layer stack."""
    return (2e-4 if dtype == "f32" else 2e-2) * max(1.0, float(np.max(np.abs(full))))


# (E, heads, kv heads): a grouped stack of head_dim 64, and an ungrouped one of head_dim 48 (rows of dp = 64 in the cache)
MODELS = [(256, 4, 2), (192, 4, 4)]


@pytest.fixture(scope="module")
def stacks():
    """x (2, 300, E), the layers and attention_stack over the 300 tokens per (dtype, model): computed once, left unchanged."""
    made = {}

    def get(dtype, E, H, Hkv):
        key = (dtype, E, H, Hkv)
        if key not in made:
            from flash_attention_minitorch_amd import modules_transformer as mt
            x, layers = _stack(np.random.default_rng(E + H + Hkv), dtype, 2, E, H, Hkv, 4, 300)
            full = to_np(mt.attention_stack(x, layers, H, causal=True, fused_layout=E // H in (32, 64, 128)))
            made[key] = (x, layers, full)
        return made[key]
    return get


@pytest.mark.parametrize("E,H,Hkv", MODELS, ids=["E256-h4-kv2", "E192-h4-kv4-d48"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prefill_then_extend_matches_the_full_attention_stack(stacks, dtype, E, H, Hkv):
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, full = stacks(dtype, E, H, Hkv)
    P, T = 100, 200
    cache = mt.KVCache(4, 2, 320, H, E // H, _tdt(dtype), "cuda", n_kv_head=Hkv)
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    got = to_np(mt.attention_stack_extend(x[:, P:].contiguous(), layers, H, cache))
    tol = _model_tol(dtype, full)
    assert maxabs(got, full[:, P:]) < tol, (maxabs(got, full[:, P:]), tol)
    assert cache.lengths.tolist() == [P + T] * 2 and cache.length_bound == P + T
    with pytest.raises(ValueError, match="capacity"):
        mt.attention_stack_extend(x[:, :129].contiguous(), layers, H, cache)


@pytest.mark.parametrize("E,H,Hkv", MODELS, ids=["E256-h4-kv2", "E192-h4-kv4-d48"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunked_prefill_matches_prefill(stacks, dtype, E, H, Hkv):
    """Pieces of 96 tokens (through the decode kernels: 96 <= 128) and of 140 (through the extend kernels) against one
    attention_stack_prefill: outputs within the model tolerance; cache contents within the same bound -- a cache row is a projection
    (weights U(-1, 1)/sqrt(E): a gain below 1) of a layer input, which the two paths compute to within that tolerance, rounded to the
    cache's dtype."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, full = stacks(dtype, E, H, Hkv)
    tdt, tol = _tdt(dtype), _model_tol(dtype, full)
    ref_cache = mt.KVCache(4, 2, 320, H, E // H, tdt, "cuda", n_kv_head=Hkv)
    ref = to_np(mt.attention_stack_prefill(x, layers, H, ref_cache))
    for chunk in (96, 140):
        cache = mt.KVCache(4, 2, 320, H, E // H, tdt, "cuda", n_kv_head=Hkv)
        cache.lengths.fill_(17)   # (stale: chunked prefill starts from an empty cache itself)
        got = to_np(mt.attention_stack_prefill_chunked(x, layers, H, cache, chunk))
        assert maxabs(got, ref) < tol and maxabs(got, full) < tol, (chunk, maxabs(got, ref), maxabs(got, full), tol)
        assert cache.lengths.tolist() == [300] * 2 and cache.length_bound == 300
        for a, b in zip(cache.k + cache.v, ref_cache.k + ref_cache.v):
            assert maxabs(to_np(a[:, :300]), to_np(b[:, :300])) < tol, chunk
            assert bool((a[:, 300:] == 0).all()) and bool((a[..., E // H:] == 0).all())
    del torch


def test_extend_of_five_tokens_is_the_fused_step():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers = _stack(np.random.default_rng(5), "bf16", 2, 192, 4, 2, 2, 45)
    outs, caches = [], []
    for step in (mt.attention_stack_extend, mt.attention_stack_step_fused):
        cache = mt.KVCache(2, 2, 64, 4, 48, torch.bfloat16, "cuda", n_kv_head=2)
        mt.attention_stack_prefill(x[:, :40].contiguous(), layers, 4, cache)
        outs.append(step(x[:, 40:].contiguous(), layers, 4, cache))
        caches.append(cache)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and caches[0].lengths.tolist() == caches[1].lengths.tolist() == [45, 45]
    for a, b in zip(caches[0].k + caches[0].v, caches[1].k + caches[1].v):
        assert torch.equal(_bits(a), _bits(b))
