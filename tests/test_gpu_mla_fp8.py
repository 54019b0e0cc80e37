"""MLA decode on an FP8 latent cache on the GPU (csrc/fa_mla_fp8.h): flash_attn_decode_mla and mla_append on 656-byte rows against the
format's restatement in tests/test_mla_fp8_cpu.py (quantise / dequantise) and the fp64 references (1e-3 max-abs on out and lse, the
bf16 tests' figure: no input exceeds theirs), and THE LAW: bit for bit the bf16 call on the dequantised cache."""
import functools

import pytest
import torch

from test_gpu_mla import check
from test_mla_cpu import CASES, DQK, DV, NCAP, SCALE, SEED, reference
from test_mla_fp8_cpu import ROW, dequantise, edge_rows, fp8_inputs, quantise
from test_mla_sparse_cpu import CASES as SPARSE_CASES, EMPTY_QUERY, indices, sparse_reference

pytestmark = pytest.mark.gpu
PAGE = 128


def paged(cache, seed=1):
    """test_gpu_mla.paged_cache for any row type: (pool, block_table); an fp8 pool's two spare pages hold 0xFF bytes, a bf16 pool's NaN."""
    B, Ncap, W = cache.shape
    mp = Ncap // PAGE
    perm = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(seed))[:B * mp]
    pool = torch.full((B * mp + 2, PAGE, W), 0xFF if cache.dtype is torch.uint8 else float("nan"), dtype=cache.dtype)
    pool[perm] = cache.reshape(B * mp, PAGE, W)
    return pool.cuda(), perm.reshape(B, mp).int().cuda()


def attend(q, cache, lens, use_pages=False, **kw):
    from flash_attention_minitorch_amd import device_ops as ops
    dev, table = paged(cache) if use_pages else (cache.cuda(), None)
    kw = {n: (t.cuda() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    out, lse = ops.flash_attn_decode_mla(q.cuda(), dev, torch.tensor(lens, dtype=torch.int32, device="cuda"), SCALE, block_table=table, **kw)
    return out.cpu(), lse.cpu(), dev.cpu(), table


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def dense_case(H, Nq, causal):
    """(q, quantised cache, fp64 (out, lse) on the dequantised cache) of a dense case, computed once for slab and paged."""
    q, cache = fp8_inputs(SEED, 2, NCAP, H, Nq)
    return q, cache, reference(q, dequantise(cache), CASES[H, Nq], SCALE, causal)


@functools.lru_cache(maxsize=None)
def sparse_case(H, Nq, topk):
    """The same for a sparse case and its lists (-1 padding, out-of-range entries, a duplicate: test_mla_sparse_cpu.indices), causal."""
    q, cache = fp8_inputs(SEED, 2, NCAP, H, Nq)
    idx = indices(SEED, 2, Nq, topk, SPARSE_CASES[H, Nq, topk], (H, Nq, topk) == EMPTY_QUERY)
    return q, cache, idx, sparse_reference(q, dequantise(cache), SPARSE_CASES[H, Nq, topk], idx, SCALE, True)


def lawful(q, cache, lens, use_pages, want, **kw):
    """The fp8 call against fp64 on the dequantised cache, against the bf16 call on it bit for bit, and (paged) against the slab call."""
    got = attend(q, cache, lens, use_pages, **kw)
    check(got, want)
    assert same(got, attend(q, dequantise(cache), lens, use_pages, **kw))
    if use_pages:
        assert same(got, attend(q, cache, lens, **kw))


@pytest.mark.parametrize("use_pages", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Nq", list(CASES))
def test_fp8_decode_matches_fp64_and_the_bf16_call_bit_for_bit(H, Nq, causal, use_pages):
    from flash_attention_minitorch_amd import _lib
    q, cache, want = dense_case(H, Nq, causal)
    assert _lib.mla().fa_mi355x_decode_mla_splits(2, H, Nq, NCAP) > 1   # several splits and the combine launch
    lawful(q, cache, CASES[H, Nq], use_pages, want, causal=causal)


@pytest.mark.parametrize("H,Nq,lens", [(5, 1, (128, 1)), (40, 2, (65, 0))])
def test_fp8_one_split_writes_the_result_directly(H, Nq, lens):
    from flash_attention_minitorch_amd import device_ops as ops
    q, cache = fp8_inputs(SEED, 2, 128, H, Nq)
    assert ops.mla_workspace(q, cache) is None
    lawful(q, cache, lens, False, reference(q, dequantise(cache), lens, SCALE, True))


@pytest.mark.parametrize("use_pages", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("H,Nq,topk", [k for k in SPARSE_CASES if k[2] in (64, 256, 768)])
def test_fp8_sparse_decode_matches_fp64_and_the_bf16_call_bit_for_bit(H, Nq, topk, use_pages):
    from flash_attention_minitorch_amd import _lib
    q, cache, idx, want = sparse_case(H, Nq, topk)
    assert (_lib.mla().fa_mi355x_decode_mla_sparse_splits(2, H, Nq, topk) > 1) == (topk == 768)
    lawful(q, cache, SPARSE_CASES[H, Nq, topk], use_pages, want, indices=idx)


@pytest.mark.parametrize("use_pages", [False, True], ids=["slab", "paged"])
def test_fp8_append_writes_the_quantised_rows_and_nothing_else_and_the_fused_call_is_both(use_pages):
    from flash_attention_minitorch_amd import device_ops as ops
    H, Nq, lens = 16, 3, (300, 2)   # (length 2 < Nq: token 0 of that sequence has no row and is not written)
    q, cache = fp8_inputs(SEED, 2, NCAP, H, Nq)
    kv_new = edge_rows(2, Nq)
    dev, table = paged(cache) if use_pages else (cache.cuda(), None)
    before, dl = dev.cpu(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    ops.mla_append(kv_new.cuda(), dev, dl, table)
    rows = lambda pool: pool if table is None else pool[table.cpu().long()].reshape(2, NCAP, ROW)
    want = cache.clone()   # the appended rows, byte for byte, and nothing else (the spare pages included)
    want[0, 297:300], want[1, 0:2] = quantise(kv_new[0]), quantise(kv_new[1, 1:])
    assert torch.equal(rows(dev.cpu()), want)
    untouched = torch.ones(dev.shape[:2], dtype=torch.bool)
    tb = table.cpu().long() if use_pages else None
    for b, r in ((0, 297), (0, 298), (0, 299), (1, 0), (1, 1)):
        untouched[(tb[b, r // PAGE], r % PAGE) if use_pages else (b, r)] = False
    assert torch.equal(dev.cpu()[untouched], before[untouched])
    # the fused call = the append, then the attend-only call; both repeat.  (The NaN and the infinity sit in token (0, 1): attend rows
    # whose values are finite, i.e. sequence 1 alone, against fp64; the bits of both sequences against the two-call form.)
    out, lse = ops.flash_attn_decode_mla(q.cuda(), dev, dl, SCALE, block_table=table)
    fused = attend(q, cache, lens, use_pages, kv_new=kv_new)
    assert torch.equal(fused[0].view(torch.int32), out.cpu().view(torch.int32)) and torch.equal(fused[1].view(torch.int32), lse.cpu().view(torch.int32))
    assert torch.equal(fused[2], dev.cpu())
    again = ops.flash_attn_decode_mla(q.cuda(), dev, dl, SCALE, block_table=table)
    assert torch.equal(again[0].view(torch.int32), out.view(torch.int32)) and torch.equal(again[1].view(torch.int32), lse.view(torch.int32))
    ref = reference(q[1:], dequantise(want[1:]), lens[1:], SCALE, True)
    check((fused[0][1:], fused[1][1:]), ref)


def test_two_fp8_model_steps_match_the_restated_format_under_fp64_attention(monkeypatch):
    """test_two_model_steps_match_unabsorbed_fp64_attention's shape and margin rule on LatentKVCache(fp8=True): the kernel steps against
    the same steps with the call replaced by quantise, write, fp64 reference on the dequantised cache.  The margin: 3 x the error of
    that fp64-middle run against the fp64-middle run on a bf16 cache (the quantisation's own error at this size), measured here."""
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    B, E, H, dn, dv, T, dev = 2, 64, 4, 32, 32, 2, "cuda"
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, DQK), u(H, dn, DV), u(H, DV, dv), u(H * dv, E))
    rope = mt.Rotary.table(64, 64, device=dev)
    xs = [(torch.rand(B, T, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev) for _ in range(2)]

    def run(attention, fp8):
        cache, ys = mt.LatentKVCache(1, B, 128, dev, fp8=fp8), []
        assert cache.kv[0].dtype is (torch.uint8 if fp8 else torch.bfloat16) and cache.kv[0].shape[-1] == (ROW if fp8 else DQK)
        with monkeypatch.context() as m:
            if attention:
                m.setattr(ops, "flash_attn_decode_mla", attention)
            for x in xs:
                cache.advance(T)
                ys.append(mt.mla_attention_step(x, cache, 0, w, H, rope).double().cpu())
        return torch.stack(ys)

    def fp64_middle(q, kv_cache, lens, scale, causal, kv_new, table, workspace=None):
        fp8 = kv_cache.dtype is torch.uint8
        for b, n in enumerate(lens.tolist()):
            kv_cache[b, n - T:n] = quantise(kv_new[b].cpu()).to(dev) if fp8 else kv_new[b]
        out, lse = reference(q.cpu(), dequantise(kv_cache.cpu()) if fp8 else kv_cache.cpu(), lens.tolist(), scale, causal)
        return out.float().to(dev), lse.float().to(dev)

    want = run(fp64_middle, True)
    err_ref = (want - run(fp64_middle, False)).abs().max().item()
    err = (run(None, True) - want).abs().max().item()
    print(f"fp8 model: kernel against the restated format {err:.3e}, the format against a bf16 cache {err_ref:.3e}")
    assert err <= 3 * err_ref
