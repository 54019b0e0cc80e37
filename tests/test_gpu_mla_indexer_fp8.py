"""FP8 index keys of the lightning indexer on the GPU (csrc/fa_mla_indexer_fp8.h): scores against fp64 on the quantised operands within
the project's bound, the append byte for byte against the restated format, the fused call's laws, the model step's wiring."""
import pytest
import torch

from test_gpu_mla_indexer import SENTINEL, dev_lens
from test_mla_cpu import SEED
from test_mla_indexer_cpu import DI, FUSED, HEADS, LENS, NCAP, index_inputs, topk_reference
from test_mla_indexer_fp8_cpu import ROW, edge_rows, fp8_inputs, quantise_idx, quantised_reference, score_case

pytestmark = pytest.mark.gpu
LAYOUTS = pytest.mark.parametrize("paged_cache", [False, True], ids=["slab", "paged"])


def layout(cache, paged_cache, seed=1):
    """(device cache, block_table, what gives the slab back): the slab, or a pool of 128-row pages under a permuted table with two
    spare pages of 0x7F bytes."""
    if not paged_cache:
        return cache.cuda(), None, lambda c: c.cpu()
    n = cache.shape[0] * NCAP // 128
    perm = torch.randperm(n + 2, generator=torch.Generator().manual_seed(seed))[:n]
    pool = torch.full((n + 2, 128, ROW), 0x7F, dtype=torch.uint8)
    pool[perm] = cache.reshape(n, 128, ROW)
    return pool.cuda(), perm.reshape(-1, NCAP // 128).int().cuda(), lambda c: c.cpu()[perm].reshape(-1, NCAP, ROW)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("HI,Nq", HEADS)
def test_fp8_scores_match_the_fp64_reference_on_the_quantised_operands(HI, Nq, lens, causal):
    from flash_attention_minitorch_amd import device_ops as ops
    q, w, kb, (ref, bound) = score_case(HI, Nq, lens, causal)
    got = []
    for cache, table, _ in (layout(kb, False), layout(kb, True)):
        s = torch.full((2, Nq, NCAP), SENTINEL, device="cuda")
        assert ops.mla_index_scores(q.cuda(), w.cuda(), cache, dev_lens(lens), causal, block_table=table, scores=s) is s
        got.append(s.cpu())
    assert torch.equal(got[0], got[1])   # paged = slab, bit for bit
    s, worst = got[0].double(), 0.0
    for b, n in enumerate(lens):
        out = torch.isneginf(ref[b, :, :n])
        assert (s[b, :, n:] == SENTINEL).all() and torch.equal(torch.isneginf(s[b, :, :n]), out)   # not written; -inf where not admitted
        ratio = ((s[b, :, :n] - ref[b, :, :n]).abs() / bound[b, :, :n])[~out]
        worst = max(worst, ratio.max().item() if ratio.numel() else 0.0)
    print(f"largest error / bound {worst:.2e}")
    assert worst <= 1.0


@LAYOUTS
def test_fp8_append_writes_the_restated_format_and_nothing_else(paged_cache):
    from flash_attention_minitorch_amd import device_ops as ops
    new, want = edge_rows(), torch.full((2, NCAP, ROW), 0xAB, dtype=torch.uint8)
    cache, table, slab = layout(want, paged_cache)
    ops.mla_index_append(new.cuda(), cache, dev_lens((2, 700)), table)   # token (0, 0) would go to row -1
    want[0, 0:2], want[1, 697:700] = quantise_idx(new[0, 1:]), quantise_idx(new[1])
    assert torch.equal(slab(cache), want) and (not paged_cache or (cache.cpu() == 0x7F).all(-1).all(-1).sum() == 2)


@LAYOUTS
def test_fp8_fused_call_is_its_three_parts_and_selects_what_the_reference_selects(paged_cache):
    from flash_attention_minitorch_amd import device_ops as ops
    HI, Nq, lens, topk = FUSED
    q, w, kb = fp8_inputs(SEED, 2, NCAP, HI, Nq)
    k_new, dl = index_inputs(SEED + 1, 2, Nq, 1, 1)[2], dev_lens(lens)
    (c1, table, slab), (c2, _, _) = layout(kb, paged_cache), layout(kb, paged_cache)
    s1 = torch.full((2, Nq, NCAP), SENTINEL, device="cuda")
    s2 = s1.clone()
    fused = ops.mla_indexer(q.cuda(), w.cuda(), c1, dl, topk, True, k_new.cuda(), table, scores=s1)
    ops.mla_index_append(k_new.cuda(), c2, dl, table)
    parts = ops.mla_index_topk(ops.mla_index_scores(q.cuda(), w.cuda(), c2, dl, True, block_table=table, scores=s2), dl, topk)
    assert torch.equal(fused, parts) and torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(c1, c2)
    again = ops.mla_indexer(q.cuda(), w.cuda(), c1, dl, topk, True, None, table, scores=s2)   # the same call twice: the same bits
    assert torch.equal(again, fused) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    # against fp64 on the appended, dequantised cache: the band rule of tests/test_gpu_mla_indexer.py
    want = kb.clone()
    for b, n in enumerate(lens):
        want[b, n - Nq:n] = quantise_idx(k_new[b])
    assert torch.equal(slab(c1), want)
    ref, bound = quantised_reference(q, w, want, lens, True)
    ref_list, fused = topk_reference(ref, lens, topk), fused.cpu()
    for b in range(2):
        for i in range(Nq):
            adm = ~torch.isneginf(ref[b, i])
            sel = fused[b, i][fused[b, i] >= 0].long()
            assert sel.numel() == min(topk, int(adm.sum())) and (sel[1:] > sel[:-1]).all() and (fused[b, i, sel.numel():] == -1).all()
            assert adm[sel].all()
            if adm.sum() > topk:
                kth = ref_list[b, i].long()[ref[b, i][ref_list[b, i].long()].argmin()]
                t, eps = ref[b, i, kth], 2 * bound[b, i, kth]
                chosen = torch.zeros(NCAP, dtype=torch.bool)
                chosen[sel] = True
                assert chosen[adm & (ref[b, i] > t + eps)].all() and not chosen[adm & (ref[b, i] < t - eps)].any()


@pytest.mark.parametrize("keys", [True, "fp8"], ids=["bf16-keys", "fp8-keys"])
def test_the_model_step_selects_its_own_lists_on_either_index_cache(keys):
    """The step's lists are device_ops.mla_indexer's on the same projections and the cache's own rows, bf16 or bytes."""
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    B, E, H, HI, dn, dv, dev = 2, 64, 4, 8, 32, 32, "cuda"
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, 576), u(H, dn, 512), u(H, 512, dv), u(H * dv, E))
    iw, rope = mt.IndexerWeights(u(E, HI * DI), u(E, DI), u(E, HI)), mt.Rotary.table(256, 64, device=dev)
    x = lambda t: (torch.rand(B, t, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    cache = mt.LatentKVCache(1, B, 128, dev, index_keys=keys)
    assert cache.kidx[0].shape[-1] == (ROW if keys == "fp8" else DI)
    for t in (64, 6):   # lengths 64 -> 70: the next step has to choose 64 of 72
        cache.advance(t)
        mt.mla_attention_step(x(t), cache, 0, w, H, rope, indexer=iw, topk=64)
    x2, off, k_before, seen, real = x(2), cache.lengths.clone(), cache.kidx[0].clone(), [], ops.mla_indexer
    q_idx = rope.apply((x2 @ iw.wq_idx).view(B, 2, HI, DI), off)
    k_idx = rope.apply((x2 @ iw.wk_idx).view(B, 2, 1, DI), off).view(B, 2, DI)
    mine = real(q_idx, ((x2 @ iw.w_head).float() * (HI ** -0.5 * DI ** -0.5)).contiguous(), k_before, off + 2, 64, True, k_idx)
    ops.mla_indexer = lambda *a, **kw: seen.append(real(*a, **kw)) or seen[-1]
    try:
        cache.advance(2)
        mt.mla_attention_step(x2, cache, 0, w, H, rope, indexer=iw, topk=64)
    finally:
        ops.mla_indexer = real
    assert torch.equal(seen[-1], mine) and (mine[:, :, -1] >= 0).all() and torch.equal(cache.kidx[0], k_before)
