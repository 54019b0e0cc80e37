"""The lightning indexer on the GPU (csrc/fa_mla_indexer.h): the scores against the fp64 definition of tests/test_mla_indexer_cpu.py
within its derived bound, the selection alone for equality with the stable sort, the fused call's laws, the model step's wiring."""
import pytest
import torch

from test_mla_cpu import SEED
from test_mla_indexer_cpu import DI, FUSED, HEADS, LENS, NCAP, index_inputs, index_scores_reference, score_case, topk_reference

pytestmark = pytest.mark.gpu
PAGE, SENTINEL = 128, 12345.0


def paged(k, seed=1):
    """The slab of index keys as a pool of 128-row pages under a permuted table, two spare pages of NaN: (pool, block_table)."""
    B, Ncap, _ = k.shape
    mp = Ncap // PAGE
    perm = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(seed))[:B * mp]
    pool = torch.full((B * mp + 2, PAGE, DI), float("nan"), dtype=k.dtype)
    pool[perm] = k.reshape(B * mp, PAGE, DI)
    return pool.cuda(), perm.reshape(B, mp).int().cuda()


def dev_lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("HI,Nq", HEADS)
def test_scores_match_the_fp64_reference_within_the_derived_bound(HI, Nq, lens, causal):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    q, w, k, (ref, bound) = score_case(HI, Nq, lens, causal)
    assert _lib.mla().fa_mi355x_mla_index_chunks(2, HI, Nq, NCAP) == 2   # 1000 keys reach the second chunk, 300 leave it empty
    got = {}
    for name, (cache, table) in (("slab", (k.cuda(), None)), ("paged", paged(k))):
        s = torch.full((2, Nq, NCAP), SENTINEL, device="cuda")
        assert ops.mla_index_scores(q.cuda(), w.cuda(), cache, dev_lens(lens), causal, block_table=table, scores=s) is s
        got[name] = s.cpu()
    assert torch.equal(got["slab"], got["paged"])   # bit for bit
    s, worst = got["slab"].double(), 0.0
    for b, n in enumerate(lens):
        assert (s[b, :, n:] == SENTINEL).all()   # at or past len_b: not written
        out = torch.isneginf(ref[b, :, :n])
        assert torch.equal(torch.isneginf(s[b, :, :n]), out)   # below len_b and not admitted: exactly -inf
        ratio = ((s[b, :, :n] - ref[b, :, :n]).abs() / bound[b, :, :n])[~out]
        worst = max(worst, ratio.max().item() if ratio.numel() else 0.0)
    print(f"largest error / bound {worst:.2e}")
    assert worst <= 1.0


TOPK_LENS = (1, 63, 64, 65, 1000, 5000, 0)


def synthetic(kind, ncap):
    """fp32 scores (7, 2, ncap) of one kind, the same for every topk."""
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(len(TOPK_LENS), 2, ncap, generator=g)
    pick = lambda *values: torch.tensor(values)[torch.randint(0, len(values), x.shape, generator=g)]
    if kind == "levels":
        x = pick(0.25, 0.5, -1.0, 3.0)   # four values: massive ties across the threshold
    elif kind == "equal":
        x = torch.full_like(x, 1.5)
    elif kind == "zeros":
        x = pick(0.0, -0.0, 0.0, -0.0, 1.0, -1.0)
    elif kind == "some-inf":
        x[torch.rand(x.shape, generator=g) < 0.3] = -float("inf")
    elif kind == "all-inf":
        x = torch.full_like(x, -float("inf"))
    elif kind == "nan":
        x[:, :, ::7] = float("nan")
    return x


@pytest.mark.parametrize("ncap", [5000, 5001], ids=["aligned-rows", "odd-rows"])
@pytest.mark.parametrize("topk", [64, 128, 2048])
@pytest.mark.parametrize("kind", ["distinct", "levels", "equal", "zeros", "some-inf", "all-inf", "nan"])
def test_topk_alone_is_the_stable_sort_exactly(kind, topk, ncap):
    from flash_attention_minitorch_amd import device_ops as ops
    x = synthetic(kind, ncap)
    got = ops.mla_index_topk(x.cuda(), dev_lens(TOPK_LENS), topk).cpu()
    assert torch.equal(got, topk_reference(x, TOPK_LENS, topk))


@pytest.mark.parametrize("paged_cache", [False, True], ids=["slab", "paged"])
def test_fused_call_is_its_three_parts_and_selects_what_the_reference_selects(paged_cache):
    from flash_attention_minitorch_amd import device_ops as ops
    HI, Nq, lens, topk = FUSED
    q, w, k = index_inputs(SEED, 2, NCAP, HI, Nq)
    k_new = index_inputs(SEED + 1, 2, Nq, 1, 1)[2]
    make = lambda: paged(k) if paged_cache else (k.cuda(), None)
    (c1, table), (c2, _), dl = make(), make(), dev_lens(lens)
    s1 = torch.full((2, Nq, NCAP), SENTINEL, device="cuda")
    s2 = s1.clone()
    fused = ops.mla_indexer(q.cuda(), w.cuda(), c1, dl, topk, True, k_new.cuda(), table, scores=s1)
    ops.mla_index_append(k_new.cuda(), c2, dl, table)
    parts = ops.mla_index_topk(ops.mla_index_scores(q.cuda(), w.cuda(), c2, dl, True, block_table=table, scores=s2), dl, topk)
    bits = lambda t: t.view(torch.int16) if t.dtype is torch.bfloat16 else t.view(torch.int32)   # (the spare pages hold NaN)
    assert torch.equal(fused, parts) and torch.equal(bits(s1), bits(s2)) and torch.equal(bits(c1), bits(c2))
    again = ops.mla_indexer(q.cuda(), w.cuda(), c1, dl, topk, True, None, table, scores=s2)   # the same call twice: the same bits
    assert torch.equal(again, fused) and torch.equal(bits(s1), bits(s2))
    # against fp64 on the appended cache: with t the k-th reference score and eps twice the bound there, everything above t + eps
    # is in the list, nothing below t - eps is, and the list is min(topk, admitted) ascending positions without a duplicate
    want = k.clone()
    for b, n in enumerate(lens):
        want[b, n - Nq:n] = k_new[b]
    slab = c1.cpu() if table is None else c1.cpu()[table.cpu().long()].reshape(2, NCAP, DI)
    assert torch.equal(bits(slab), bits(want))
    ref, bound = index_scores_reference(q, w, want, lens, True)
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


def test_the_model_step_selects_its_own_lists():
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    B, E, H, HI, dn, dv, T, dev = 2, 64, 4, 8, 32, 32, 4, "cuda"
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, 576), u(H, dn, 512), u(H, 512, dv), u(H * dv, E))
    iw = mt.IndexerWeights(u(E, HI * DI), u(E, DI), u(E, HI))
    rope = mt.Rotary.table(256, 64, device=dev)
    x = lambda t: (torch.rand(B, t, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    caches = [mt.LatentKVCache(1, B, 128, dev, index_keys=True) for _ in range(3)]   # the step's own lists; given lists; dense
    seen = []

    def step(xs, kind):
        """One step on each cache; returns (own lists' output, the lists the indexer returned, given lists' output)."""
        for c in caches:
            c.advance(xs.shape[1])
        real = ops.mla_indexer
        ops.mla_indexer = lambda *a, **kw: seen.append(real(*a, **kw)) or seen[-1]
        try:
            own = mt.mla_attention_step(xs, caches[0], 0, w, H, rope, indexer=iw, topk=64)
        finally:
            ops.mla_indexer = real
        given = mt.mla_attention_step(xs, caches[1], 0, w, H, rope, indices=kind(seen[-1]))
        return own, seen[-1], given

    # topk = 64 >= T: token t's list is 0 .. t, then -1
    own, lists, given = step(x(T), lambda lists: lists)
    want = torch.full((B, T, 64), -1, dtype=torch.int32)
    for t in range(T):
        want[:, t, :t + 1] = torch.arange(t + 1)
    assert torch.equal(lists.cpu(), want) and torch.equal(own, given)
    # lengths 4 -> 70 -> 72: selection is real (72 > 64), and the step equals the step given device_ops.mla_indexer's list on the same
    # projections: the rotation at positions 70 and 71, the weights and the fused append into kidx, recomputed here
    fill = x(66)
    step(fill[:, :64], lambda lists: lists), step(fill[:, 64:], lambda lists: lists)
    x2 = x(2)
    off = caches[1].lengths.clone()   # (70: the new tokens' first position)
    k_before = caches[0].kidx[0].clone()
    q_idx = rope.apply((x2 @ iw.wq_idx).view(B, 2, HI, DI), off)
    k_idx = rope.apply((x2 @ iw.wk_idx).view(B, 2, 1, DI), off).view(B, 2, DI)
    w_idx = ((x2 @ iw.w_head).float() * (HI ** -0.5 * DI ** -0.5)).contiguous()
    mine = ops.mla_indexer(q_idx, w_idx, k_before, off + 2, 64, True, k_idx)
    own, lists, given = step(x2, lambda lists: mine)
    assert torch.equal(lists, mine) and (mine[:, :, -1] >= 0).all() and torch.equal(own, given)
    assert torch.equal(caches[0].kidx[0], k_before) and torch.equal(caches[0].kv[0], caches[1].kv[0])
    # indexer=None is the step it was: the dense call's bits, with or without the new keywords
    caches[2].advance(2)
    a = mt.mla_attention_step(x2, caches[2], 0, w, H, rope)
    b = mt.mla_attention_step(x2, caches[2], 0, w, H, rope, indexer=None, topk=None)
    assert torch.equal(a, b) and caches[2].kidx[0].count_nonzero() == 0
