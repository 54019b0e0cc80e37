"""Sparse MLA decode on the GPU (csrc/fa_mla_sparse.h): flash_attn_decode_mla(indices=) against the fp64 definition of
tests/test_mla_sparse_cpu.py on its index lists (1e-3 max-abs on out and lse, the dense MLA tests' figure), the bit-for-bit laws, one
model step against un-absorbed fp64 sparse attention."""
import pytest
import torch

from test_gpu_mla import check, gathered, paged_cache
from test_mla_cpu import DQK, DV, NCAP, SCALE, SEED, inputs
from test_mla_sparse_cpu import CASES, case, indices, sparse_reference

pytestmark = pytest.mark.gpu


def attend(q, kv, lens, idx, paged=False, **kw):
    from flash_attention_minitorch_amd import device_ops as ops
    cache, table = paged_cache(kv) if paged else (kv.cuda(), None)
    kw = {n: (t.cuda() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    out, lse = ops.flash_attn_decode_mla(q.cuda(), cache, torch.tensor(lens, dtype=torch.int32, device="cuda"), SCALE, block_table=table,
                                         indices=idx.cuda(), **kw)
    return out.cpu(), lse.cpu(), cache.cpu(), table


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Nq,topk", list(CASES))
def test_sparse_decode_matches_the_fp64_reference(H, Nq, topk, causal, paged):
    from flash_attention_minitorch_amd import _lib
    q, kv, lens, idx, want = case(H, Nq, topk, causal)
    assert (_lib.mla().fa_mi355x_decode_mla_sparse_splits(2, H, Nq, topk) > 1) == (topk == 768)   # the combine launch, or one split
    got = attend(q, kv, lens, idx, paged, causal=causal)
    check(got, want)
    if paged:   # bit for bit the slab call on the gathered cache
        slab = attend(q, kv, lens, idx, causal=causal)
        assert torch.equal(got[0], slab[0]) and torch.equal(got[1], slab[1])


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_fused_sparse_call_is_the_append_then_the_attention_and_both_repeat(paged):
    from flash_attention_minitorch_amd import device_ops as ops
    H, Nq, lens = 16, 3, (300, 2)   # (length 2 < Nq: token 0 of that sequence has no row and is not written)
    q, kv = inputs(SEED, 2, NCAP, H, Nq)
    kv_new, idx = inputs(SEED + 1, 2, Nq, 1, 1)[1], indices(SEED, 2, Nq, 128, lens)
    idx[0, :, 6:9] = torch.tensor([297, 298, 299], dtype=torch.int32)   # the appended rows, each admitted from its own token on
    fused = attend(q, kv, lens, idx, paged, kv_new=kv_new)
    cache, table = paged_cache(kv) if paged else (kv.cuda(), None)
    dl, di = torch.tensor(lens, dtype=torch.int32, device="cuda"), idx.cuda()
    ops.mla_append(kv_new.cuda(), cache, dl, table)
    out, lse = ops.flash_attn_decode_mla(q.cuda(), cache, dl, SCALE, block_table=table, indices=di)
    assert torch.equal(fused[0], out.cpu()) and torch.equal(fused[1], lse.cpu())
    assert torch.equal(fused[2].view(torch.int16), cache.cpu().view(torch.int16))   # (bits: the spare pages hold NaN)
    again = ops.flash_attn_decode_mla(q.cuda(), cache, dl, SCALE, block_table=table, indices=di)   # the same call twice: the same bits
    assert torch.equal(again[0], out) and torch.equal(again[1], lse)
    check(fused, sparse_reference(q, gathered(fused[2], table), lens, idx, SCALE, True))
    dense, none = (ops.flash_attn_decode_mla(q.cuda(), cache, dl, SCALE, block_table=table, **kw) for kw in ({}, {"indices": None}))
    assert torch.equal(dense[0], none[0]) and torch.equal(dense[1], none[1]) and not torch.equal(dense[0], out)


def test_a_sparse_model_step_matches_unabsorbed_fp64_sparse_attention(monkeypatch):
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    B, E, H, dn, dv, T, dev = 2, 64, 4, 32, 32, 4, "cuda"
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, DQK), u(H, dn, DV), u(H, DV, dv), u(H * dv, E))
    rope = mt.Rotary.table(64, 64, device=dev)
    x = (torch.rand(B, T, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    idx = torch.randint(-1, T + 1, (B, T, 64), generator=g).int()   # positions 0 .. T - 1 many times over, -1 and T (never admitted)
    idx[:, :, 0] = torch.arange(T)   # (every token names itself: no empty row)

    def run(attention):
        """The step through a fresh cache with ``attention`` in the place of the kernel call; its output, fp64."""
        cache = mt.LatentKVCache(1, B, 128, dev)
        cache.advance(T)
        with monkeypatch.context() as m:
            if attention:
                m.setattr(ops, "flash_attn_decode_mla", attention)
            return mt.mla_attention_step(x, cache, 0, w, H, rope, indices=idx.to(dev)).double().cpu()

    def fp64_middle(q, kv_cache, lens, scale, causal, kv_new, table, workspace=None, indices=None):
        kv_cache[:, :T] = kv_new   # (the append, by hand)
        out, lse = sparse_reference(q.cpu(), kv_cache.cpu(), lens.tolist(), indices.cpu(), scale, causal)
        return out.float().to(dev), lse.float().to(dev)

    # the un-absorbed definition in fp64 over each token's admitted entries (j <= i, each entry a key of its own)
    wq, w_dkv, w_uk, w_uv, wo = (t.double().cpu() for t in w)
    cos, sin = rope.cos.double().cpu(), rope.sin.double().cpu()
    rot = lambda t, pos: torch.cat([t[..., :32] * cos[pos] - t[..., 32:] * sin[pos], t[..., 32:] * cos[pos] + t[..., :32] * sin[pos]], -1)
    xd = x.double().cpu()
    q, ckv = (xd @ wq).view(B, T, H, dn + 64), xd @ w_dkv
    want = torch.zeros(B, T, E, dtype=torch.float64)
    for b in range(B):
        k_pe = torch.stack([rot(ckv[b, j, DV:], j) for j in range(T)])
        for i in range(T):
            j = idx[b, i][(idx[b, i] >= 0) & (idx[b, i] <= i)].long()
            heads = []
            for h in range(H):
                k_h = torch.cat([ckv[b, j, :DV] @ w_uk[h].T, k_pe[j]], -1)
                p = torch.softmax((dn + 64) ** -0.5 * k_h @ torch.cat([q[b, i, h, :dn], rot(q[b, i, h, dn:], i)]), 0)
                heads.append(p @ (ckv[b, j, :DV] @ w_uv[h]))
            want[b, i] = torch.cat(heads) @ wo
    err_ref = (run(fp64_middle) - want).abs().max().item()   # the bf16 projections' own error, measured against the reference
    err = (run(None) - want).abs().max().item()
    print(f"model: kernel {err:.3e}, fp64 middle {err_ref:.3e}")
    assert err <= 3 * err_ref
