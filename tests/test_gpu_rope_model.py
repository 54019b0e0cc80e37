"""The model layer with rotary embeddings (modules_transformer: Rotary, attention_stack(rope=), KVCache(rope=)) on the GPU:
attention_stack(rope=) forward and gradients against a torch fp64 model with the rotation written in torch, at the tolerance of
tests/test_gpu_model.py; prefill plus steps -- unfused, fused and GraphedStep -- against attention_stack(rope=) over the whole
sequence, at the shapes and tolerance of test_prefill_then_graphed_steps_match_the_full_attention_stack, the three steps bit for
bit the same."""
import math

import numpy as np
import pytest

from gpu_util import maxabs, rand_u, to_np
from test_rope_cpu import rope_tables

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _bits(t):
    torch = _torch()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _rotate64(t, c, s, rot, il):
    """The rotation in torch (fp64, differentiable): t (B, N, heads, d), token i at position i; c, s (N, rot / 2)."""
    torch = _torch()
    c, s = c[None, :, None, :], s[None, :, None, :]
    x1, x2 = (t[..., 0:rot:2], t[..., 1:rot:2]) if il else (t[..., :rot // 2], t[..., rot // 2:rot])
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    head = torch.stack([y1, y2], dim=-1).flatten(-2) if il else torch.cat([y1, y2], dim=-1)
    return torch.cat([head, t[..., rot:]], dim=-1)


def _stack64(x, layers, H, c, s, rot, il):
    """attention_stack(causal=True, rope=) in torch fp64 on the CPU: grouped-query heads by repetition, dense causal softmax."""
    torch = _torch()
    B, N, E = x.shape
    d = E // H
    mask = torch.tril(torch.ones(N, N, dtype=torch.bool))
    for wq, wk, wv, wo in layers:
        Hkv = wk.shape[1] // d
        q, k, v = ((x @ w).view(B, N, w.shape[1] // d, d) for w in (wq, wk, wv))
        q, k = _rotate64(q, c, s, rot, il), _rotate64(k, c, s, rot, il)
        k, v = (t.repeat_interleave(H // Hkv, dim=2) for t in (k, v))
        sc = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(d)
        p = torch.softmax(sc.masked_fill(~mask, float("-inf")), dim=-1)
        o = torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, N, E)
        x = x + o @ wo
    return x


@pytest.mark.parametrize("N,H,Hkv,E,rot,il", [(77, 2, 2, 64, 16, False), (130, 4, 2, 256, 64, True), (192, 1, 1, 128, 128, False)],
                         ids=["d32-rot16", "gqa-d64-gptj", "d128-full"])
def test_attention_stack_with_rope_fp32_matches_a_torch_fp64_model(N, H, Hkv, E, rot, il):
    """Output, dx and every weight gradient of a causal stack that rotates q and k in every layer: the rotation's backward is the
    inverse rotation (device_ops.apply_rotary), so the path is trainable."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(5100 + N)
    B, LAYERS, d = 2, 3, E // H
    x, dout = rand_u(rng, (B, N, E)), rand_u(rng, (B, N, E))
    w = lambda cols: (rand_u(rng, (E, cols)) * np.float32(1.5 / np.sqrt(E))).astype(np.float32)
    layers = [(w(E), w(Hkv * d), w(Hkv * d), w(E)) for _ in range(LAYERS)]
    c, s = rope_tables(N, rot)
    rope = mt.Rotary(torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(), il)
    tx = torch.from_numpy(x).cuda().requires_grad_(True)
    tl = [tuple(torch.from_numpy(t).cuda().requires_grad_(True) for t in lw) for lw in layers]
    y = mt.attention_stack(tx, tl, H, causal=True, rope=rope)
    y.backward(torch.from_numpy(dout).cuda())
    rx = torch.from_numpy(x).double().requires_grad_(True)
    rl = [tuple(torch.from_numpy(t).double().requires_grad_(True) for t in lw) for lw in layers]
    ry = _stack64(rx, rl, H, torch.from_numpy(c).double(), torch.from_numpy(s).double(), rot, il)
    ry.backward(torch.from_numpy(dout).double())
    tol = lambda ref: 2e-4 * max(1.0, float(np.max(np.abs(ref))))
    ref = ry.detach().numpy()
    assert maxabs(to_np(y), ref) < tol(ref), (maxabs(to_np(y), ref), tol(ref))
    assert maxabs(to_np(tx.grad), rx.grad.numpy()) < tol(rx.grad.numpy())
    for li in range(LAYERS):
        for nm, got, want in zip(("wq", "wk", "wv", "wo"), tl[li], rl[li]):
            g = want.grad.numpy()
            assert got.grad.shape == got.shape and maxabs(to_np(got.grad), g) < tol(g), (li, nm, maxabs(to_np(got.grad), g), tol(g))
    # the rotation is part of the function: without it the stack computes something else
    plain = mt.attention_stack(tx.detach(), [tuple(t.detach() for t in lw) for lw in tl], H, causal=True)
    assert maxabs(to_np(plain), ref) > 10 * tol(ref)
    # the reference's data flow (head-split copies around the operator) rotates in front of the copies: the same values
    y2 = mt.attention_stack(tx.detach(), [tuple(t.detach() for t in lw) for lw in tl], H, causal=True, fused_layout=False, rope=rope)
    assert maxabs(to_np(y2), ref) < tol(ref)


def _stack(rng, dtype, B, E, H, Hkv, L, n_tokens):
    torch = _torch()
    tdt = _tdt(dtype)
    d = E // H
    x = torch.from_numpy(rand_u(rng, (B, n_tokens, E))).to("cuda", tdt)
    layers = [tuple(torch.from_numpy(rand_u(rng, (E, c)) / np.float32(math.sqrt(E))).to("cuda", tdt) for c in (E, Hkv * d, Hkv * d, E))
              for _ in range(L)]
    return x, layers


# (E, heads, kv heads, rot, interleaved): head_dim 64 ungrouped with the whole head rotated, and head_dim 48 (E = 4 * 48) with 2 kv
# heads: d_new = 48 into rows of dp = 64, 32 of the 48 columns rotated in GPT-J pairs
MODELS = [(256, 4, 4, 64, False), (192, 4, 2, 32, True)]


@pytest.mark.parametrize("E,H,Hkv,rot,il", MODELS, ids=["E256-h4-kv4-rot64", "E192-h4-kv2-d48-rot32-gptj"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prefill_then_graphed_steps_with_rope_match_the_full_attention_stack(dtype, E, H, Hkv, rot, il):
    """Prompts of 40 and 33 tokens in one batch, then 5 captured steps on a cache built with rope=; every batch element against
    attention_stack(rope=) over its own whole sequence.  A second cache stepped eagerly with the fused step (one rope_append launch,
    then the attend-only call) and a third with attention_stack_step (apply_rotary at offsets = lengths, then torch indexing) end
    with the same bits, and the three steps return the same bits."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(E + H)
    B, P, S, L, cap = 2, 40, 5, 4, 64
    prompts = [P, P - 7]
    x, layers = _stack(rng, dtype, B, E, H, Hkv, L, P + S)
    tdt = _tdt(dtype)
    rope = mt.Rotary.table(cap, rot, device="cuda", interleaved=il)
    caches = [mt.KVCache(L, B, cap, H, E // H, tdt, "cuda", n_kv_head=Hkv, rope=rope) for _ in range(3)]
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
        full = to_np(mt.attention_stack(seq, layers, H, causal=True, fused_layout=E // H in (32, 64, 128), rope=rope))[0, p:]
        tol = (2e-4 if dtype == "f32" else 2e-2) * max(1.0, float(np.max(np.abs(full))))
        assert maxabs(got[b], full) < tol, (b, maxabs(got[b], full), tol)
        assert maxabs(eager[b], full) < tol, (b, maxabs(eager[b], full), tol)
        # (positions matter: the same steps on a cache without rope are another function)
    assert np.array_equal(got, eager) and np.array_equal(eager, unfused)
    for cache in caches[1:]:
        assert caches[0].lengths.tolist() == cache.lengths.tolist() == [p + S for p in prompts]
        assert caches[0].length_bound == cache.length_bound == P + S
        for a, b in zip(caches[0].k + caches[0].v, cache.k + cache.v):
            assert torch.equal(_bits(a), _bits(b))
    if caches[0].dp > E // H:   # the new rows' padding columns are zero, written by the library
        assert all(bool((t[..., E // H:] == 0).all()) for t in caches[0].k + caches[0].v)
    norope = mt.KVCache(L, B, cap, H, E // H, tdt, "cuda", n_kv_head=Hkv)
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, norope)
    other = to_np(mt.attention_stack_step_fused(x[:, P:P + 1].contiguous(), layers, H, norope))
    assert not np.array_equal(other, outs[0][1])


def test_extend_ragged_and_chunked_prefill_with_rope_match_the_full_stack():
    """A paged cache with a window, sinks and rope: a chunked prefill (extend kernels), then a ragged step, against the one-piece
    prefill of a slab cache of the same geometry and, for the ragged step's tokens, against stepping that cache; bf16, at the
    tolerance of the test above."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(77)
    B, E, H, Hkv, L, P, cap = 2, 256, 4, 2, 2, 200, 512
    x, layers = _stack(rng, "bf16", B, E, H, Hkv, L, P + 3)
    rope = mt.Rotary.table(cap, 64, device="cuda")
    kw = dict(n_kv_head=Hkv, window=160, sink=4, rope=rope)
    slab = mt.KVCache(L, B, cap, H, E // H, torch.bfloat16, "cuda", **kw)
    paged = mt.PagedKVCache(L, B, cap, H, E // H, torch.bfloat16, "cuda", page_size=128, **kw)
    y1 = to_np(mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, slab))            # (windowed: one extend piece)
    y2 = to_np(mt.attention_stack_prefill_chunked(x[:, :P].contiguous(), layers, H, paged, 150))
    tol = 2e-2 * max(1.0, float(np.max(np.abs(y1))))
    assert maxabs(y2, y1) < tol, (maxabs(y2, y1), tol)
    # a ragged step: sequence 0 brings 3 tokens, sequence 1 one
    packed = torch.cat([x[0, P:P + 3], x[1, P:P + 1]], dim=0).contiguous()
    r = to_np(mt.attention_stack_ragged(packed, [3, 1], layers, H, paged))
    s3 = to_np(mt.attention_stack_extend(x[:, P:P + 3].contiguous(), layers, H, slab))
    assert maxabs(r[:3], s3[0]) < tol and maxabs(r[3], s3[1, 0]) < tol, (maxabs(r[:3], s3[0]), maxabs(r[3], s3[1, 0]), tol)
    assert paged.lengths.tolist() == [P + 3, P + 1]
