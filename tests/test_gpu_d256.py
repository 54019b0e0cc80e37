"""Head dim 256 on the GPU (csrc/fa_decode_d256.h): flash_attn_decode / flash_attn_extend on 256-wide bf16 caches against the fp64
reference of tests/test_d256_cpu.py (inputs U(-1, 1), tau = 1/16; 1e-3 max-abs on out and lse), the bit-for-bit laws, one model case."""
import pytest
import torch

from test_d256_cpu import TOL, reference

pytestmark = pytest.mark.gpu
D, NCAP, PAGE = 256, 768, 128
CASE_SEEDS = (5,)   # (tests/test_d256_cpu.py holds the references of these inputs apart by 10 tolerances)


def inputs(seed, B, Ncap, H, Hkv, Nq):
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).to(torch.bfloat16)
    return u(B, Nq, H, D), u(B, Ncap, Hkv, D), u(B, Ncap, Hkv, D)


def paged_cache(k, v, seed=1):
    """The slabs as pools of 128-row pages under a permuted table, two spare pages of NaN: (k_pool, v_pool, block_table)."""
    B, Ncap, Hkv, _ = k.shape
    mp = Ncap // PAGE
    perm = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(seed))[:B * mp]
    pools = []
    for t in (k, v):
        pool = torch.full((B * mp + 2, PAGE, Hkv, D), float("nan"), dtype=t.dtype)
        pool[perm] = t.reshape(B * mp, PAGE, Hkv, D)
        pools.append(pool.cuda())
    return pools[0], pools[1], perm.reshape(B, mp).int().cuda()


def attend(family, q, k, v, lens, paged=False, **kw):
    from flash_attention_minitorch_amd import device_ops as ops
    fn = ops.flash_attn_decode if family == "decode" else ops.flash_attn_extend
    if paged:
        kd, vd, table = paged_cache(k, v)
        kw["block_table"] = table
    else:
        kd, vd = k.cuda(), v.cuda()
    kw = {n: (t.cuda() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    out, lse = fn(q.cuda(), kd, vd, torch.tensor(lens, dtype=torch.int32, device="cuda"), **kw)
    return out.cpu(), lse.cpu(), kd.cpu(), vd.cpu()


def check(got, want):
    (out, lse), (rout, rlse) = got[:2], want
    empty = torch.isneginf(rlse)
    assert torch.equal(torch.isneginf(lse), empty) and not out.isnan().any()
    eo, el = (out.double() - rout).abs().max().item(), (lse.double() - rlse)[~empty].abs().max().item() if (~empty).any() else 0.0
    print(f"max-abs out {eo:.2e} lse {el:.2e}")
    assert eo <= TOL and el <= TOL, (eo, el)


LENS = {1: (768, 127), 3: (300, 129), 33: (128, 768)}   # by Nq; every one of {1, 127, 128, 129, 300, 768} appears (1: the empty-row test)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("softcap", [None, 0.25])
@pytest.mark.parametrize("causal,window", [(True, None), (True, 100), (False, None)])
@pytest.mark.parametrize("Nq", [1, 3, 33])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (8, 2)])
def test_decode_matches_the_fp64_reference(H, Hkv, Nq, causal, window, softcap, paged):
    from flash_attention_minitorch_amd import _lib
    q, k, v = inputs(CASE_SEEDS[0], 2, NCAP, H, Hkv, Nq)
    if window is None:   # three splits and the combine launch (a window's span of 100 + Nq + 126 keys is one or two)
        assert _lib.decode().fa_mi355x_decode_d256_splits(2, H, Hkv, Nq, NCAP, D, 1, 0) > 1
    kw = dict(causal=causal, window=window, softcap=softcap)
    got = attend("decode", q, k, v, LENS[Nq], paged, **kw)
    check(got, reference(q, k, v, LENS[Nq], causal, window, softcap))
    if paged:   # bit for bit the slab call on the gathered cache
        slab = attend("decode", q, k, v, LENS[Nq], False, **kw)
        assert torch.equal(got[0], slab[0]) and torch.equal(got[1], slab[1])


@pytest.mark.parametrize("family,Nq", [("decode", 3), ("extend", 130)])
def test_one_split_writes_the_result_directly(family, Nq):
    from flash_attention_minitorch_amd import _lib
    assert getattr(_lib.decode(), f"fa_mi355x_{family}_d256_splits")(2, 4, 2, Nq, 256, D, 1, 0) == 1   # Ncap = 256: one chunk
    q, k, v = inputs(7, 2, 256, 4, 2, Nq)
    check(attend(family, q, k, v, (256, 199)), reference(q, k, v, (256, 199)))


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("softcap", [None, 0.25])
@pytest.mark.parametrize("window", [None, 100])
@pytest.mark.parametrize("Nq", [129, 200])
def test_extend_matches_the_fp64_reference(Nq, window, softcap, paged):
    q, k, v = inputs(CASE_SEEDS[0], 2, NCAP, 4, 2, Nq)
    lens, kw = (200, 700), dict(window=window, softcap=softcap)
    got = attend("extend", q, k, v, lens, paged, **kw)
    check(got, reference(q, k, v, lens, True, window, softcap))
    if paged:
        slab = attend("extend", q, k, v, lens, False, **kw)
        assert torch.equal(got[0], slab[0]) and torch.equal(got[1], slab[1])


def test_extend_of_64_tokens_agrees_with_decode():
    q, k, v = inputs(3, 2, NCAP, 4, 2, 64)
    a, b = attend("extend", q, k, v, (300, 768)), attend("decode", q, k, v, (300, 768))
    check(a, reference(q, k, v, (300, 768)))
    assert (a[0] - b[0]).abs().max() <= TOL and (a[1] - b[1]).abs().max() <= TOL


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("family,Nq", [("decode", 3), ("extend", 150)])
def test_bit_for_bit_laws(family, Nq, paged):
    from flash_attention_minitorch_amd import device_ops as ops
    q, k, v = inputs(11, 2, NCAP, 4, 2, Nq)
    lens = (400, 768)
    plain = attend(family, q, k, v, lens, paged)
    again = attend(family, q, k, v, lens, paged)   # two runs
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])
    same = attend(family, q, k, v, lens, paged, window=NCAP, softcap=0.0)   # a window that admits every key, no cap: the plain call
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    # the fused append: the caches hold NaN where the new tokens go; d_new = 192 leaves zero columns behind them
    rows = [torch.arange(n - Nq, n) for n in lens]
    k_new, v_new = (torch.stack([t[b, r, :, :192] for b, r in enumerate(rows)]).contiguous() for t in (k, v))
    k0, v0 = k.clone(), v.clone()
    for b, r in enumerate(rows):
        k0[b, r] = v0[b, r] = float("nan")
    fused = attend(family, q, k0, v0, lens, paged, k_new=k_new, v_new=v_new)
    kd, vd, table = paged_cache(k0, v0) if paged else (k0.cuda(), v0.cuda(), None)
    append = ops.decode_append if family == "decode" else ops.extend_append
    append(k_new.cuda(), v_new.cuda(), kd, vd, torch.tensor(lens, dtype=torch.int32, device="cuda"), block_table=table)
    assert torch.equal(fused[2].view(torch.int16), kd.cpu().view(torch.int16)) and torch.equal(fused[3].view(torch.int16), vd.cpu().view(torch.int16))
    fn = ops.flash_attn_decode if family == "decode" else ops.flash_attn_extend
    out, lse = fn(q.cuda(), kd, vd, torch.tensor(lens, dtype=torch.int32, device="cuda"), block_table=table)
    assert torch.equal(fused[0], out.cpu()) and torch.equal(fused[1], lse.cpu())


def test_rows_without_an_admissible_key():
    q, k, v = inputs(13, 2, NCAP, 4, 2, 33)
    got = attend("decode", q, k, v, (1, 20))   # len_b < Nq: the first 32 / 13 queries sit at negative positions
    ref = reference(q, k, v, (1, 20))
    assert torch.isneginf(ref[1][0, :, :32]).all() and torch.isneginf(ref[1][1, :, :13]).all()
    check(got, ref)
    assert not got[0][0, :32].any() and not got[0][1, :13].any()


def test_model_steps_on_a_256_wide_cache_match_its_chunked_prefill():
    """Four tokens one at a time through attention_stack_step_fused (Nq = 1) against attention_stack_prefill_chunked as one piece
    (Nq = 4).  Activations stay below 1/4, where bf16 values are 2^-10 < 1e-3 apart: one rounding of the residual stays inside."""
    from flash_attention_minitorch_amd import modules_transformer as mt
    g = torch.Generator().manual_seed(17)
    H, HKV, E = 2, 1, 512
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)
    layers = [tuple((u(E, n) / E ** 0.5).to(torch.bfloat16).cuda() for n in (E, HKV * D, HKV * D, E))]
    x = (u(1, 4, E) / 8).to(torch.bfloat16).cuda()
    caches = [mt.KVCache(1, 1, 256, H, D, torch.bfloat16, "cuda", n_kv_head=HKV, window=64, softcap=50.0) for _ in range(2)]
    steps = torch.cat([mt.attention_stack_step_fused(x[:, t:t + 1].contiguous(), layers, H, caches[0]) for t in range(4)], 1)
    whole = mt.attention_stack_prefill_chunked(x, layers, H, caches[1], 4)
    assert (steps.float() - whole.float()).abs().max() <= TOL and (steps.float() - x.float()).abs().max() > 0
    assert caches[0].lengths.tolist() == caches[1].lengths.tolist() == [4]
