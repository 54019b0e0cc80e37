"""Multi-head latent attention decode on the GPU (csrc/fa_mla.h): flash_attn_decode_mla on a 576-wide bf16 latent cache against the
fp64 reference of tests/test_mla_cpu.py (inputs U(-1, 1), scale 192^-1/2; 1e-3 max-abs on out and lse), the bit-for-bit laws, one
model case against un-absorbed fp64 attention."""
import pytest
import torch

from test_mla_cpu import CASES, DQK, DV, NCAP, SCALE, SEED, TOL, inputs, reference

pytestmark = pytest.mark.gpu
PAGE = 128


def paged_cache(kv, seed=1):
    """The slab as a pool of 128-row pages under a permuted table, two spare pages of NaN: (pool, block_table)."""
    B, Ncap, _ = kv.shape
    mp = Ncap // PAGE
    perm = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(seed))[:B * mp]
    pool = torch.full((B * mp + 2, PAGE, DQK), float("nan"), dtype=kv.dtype)
    pool[perm] = kv.reshape(B * mp, PAGE, DQK)
    return pool.cuda(), perm.reshape(B, mp).int().cuda()


def attend(q, kv, lens, paged=False, **kw):
    from flash_attention_minitorch_amd import device_ops as ops
    cache, table = paged_cache(kv) if paged else (kv.cuda(), None)
    kw = {n: (t.cuda() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    out, lse = ops.flash_attn_decode_mla(q.cuda(), cache, torch.tensor(lens, dtype=torch.int32, device="cuda"), SCALE, block_table=table, **kw)
    return out.cpu(), lse.cpu(), cache.cpu(), table


def gathered(cache, table):
    return cache if table is None else cache[table.cpu().long()].reshape(table.shape[0], -1, DQK)


def check(got, want):
    (out, lse), (rout, rlse) = got[:2], want
    empty = torch.isneginf(rlse)
    assert torch.equal(torch.isneginf(lse), empty) and not out.isnan().any()
    eo, el = (out.double() - rout).abs().max().item(), (lse.double() - rlse)[~empty].abs().max().item() if (~empty).any() else 0.0
    print(f"max-abs out {eo:.2e} lse {el:.2e}")
    assert eo <= TOL and el <= TOL, (eo, el)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Nq", list(CASES))
def test_decode_matches_the_fp64_reference(H, Nq, causal, paged):
    from flash_attention_minitorch_amd import _lib
    q, kv = inputs(SEED, 2, NCAP, H, Nq)
    assert _lib.mla().fa_mi355x_decode_mla_splits(2, H, Nq, NCAP) > 1   # several splits and the combine launch
    got = attend(q, kv, CASES[H, Nq], paged, causal=causal)
    check(got, reference(q, kv, CASES[H, Nq], SCALE, causal))
    if paged:   # bit for bit the slab call on the gathered cache
        slab = attend(q, kv, CASES[H, Nq], causal=causal)
        assert torch.equal(got[0], slab[0]) and torch.equal(got[1], slab[1])


@pytest.mark.parametrize("H,Nq,lens", [(5, 1, (128, 1)), (40, 2, (65, 0))])
def test_one_split_writes_the_result_directly(H, Nq, lens):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    q, kv = inputs(SEED, 2, 128, H, Nq)
    assert _lib.mla().fa_mi355x_decode_mla_splits(2, H, Nq, 128) == 1 and ops.mla_workspace(q, kv) is None
    check(attend(q, kv, lens), reference(q, kv, lens, SCALE, True))


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_fused_call_is_the_append_then_the_attention_and_both_repeat(paged):
    from flash_attention_minitorch_amd import device_ops as ops
    H, Nq, lens = 16, 3, (300, 2)   # (length 2 < Nq: token 0 of that sequence has no row and is not written)
    q, kv = inputs(SEED, 2, NCAP, H, Nq)
    kv_new = inputs(SEED + 1, 2, Nq, 1, 1)[1]
    fused = attend(q, kv, lens, paged, kv_new=kv_new)
    cache, table = paged_cache(kv) if paged else (kv.cuda(), None)
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ops.mla_append(kv_new.cuda(), cache, dl, table)
    out, lse = ops.flash_attn_decode_mla(q.cuda(), cache, dl, SCALE, block_table=table)
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))   # (bits: the spare pages hold NaN)
    assert torch.equal(fused[0], out.cpu()) and torch.equal(fused[1], lse.cpu()) and same(fused[2], cache.cpu())
    again = ops.flash_attn_decode_mla(q.cuda(), cache, dl, SCALE, block_table=table)   # the same call twice: the same bits
    assert torch.equal(again[0], out) and torch.equal(again[1], lse)
    want = kv.clone()   # the appended rows and nothing else
    want[0, 297:300], want[1, 0:2] = kv_new[0], kv_new[1, 1:]
    assert same(gathered(fused[2], table), want)
    check(fused, reference(q, want, lens, SCALE, True))


def test_two_model_steps_match_unabsorbed_fp64_attention(monkeypatch):
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    B, E, H, dn, dv, T, dev = 2, 64, 4, 32, 32, 2, "cuda"
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, DQK), u(H, dn, DV), u(H, DV, dv), u(H * dv, E))
    rope = mt.Rotary.table(64, 64, device=dev)
    xs = [(torch.rand(B, T, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev) for _ in range(2)]

    def run(attention):
        """Two steps through a fresh cache with ``attention`` in the place of the kernel call; the steps' outputs, fp64."""
        cache, ys = mt.LatentKVCache(1, B, 128, dev), []
        with monkeypatch.context() as m:
            if attention:
                m.setattr(ops, "flash_attn_decode_mla", attention)
            for x in xs:
                cache.advance(T)
                ys.append(mt.mla_attention_step(x, cache, 0, w, H, rope).double().cpu())
        return torch.stack(ys)

    def fp64_middle(q, kv_cache, lens, scale, causal, kv_new, table, workspace=None):
        """The fp64 reference on the same bf16-rounded inputs, appended by hand."""
        for b, n in enumerate(lens.tolist()):
            kv_cache[b, n - T:n] = kv_new[b]
        out, lse = reference(q.cpu(), kv_cache.cpu(), lens.tolist(), scale, causal)
        return out.float().to(dev), lse.float().to(dev)

    # the un-absorbed definition in fp64: k_h = [c W_UK[h]^T | rope(k_pe)], v_h = c W_UV[h], softmax((dn + 64)^-1/2 q_h k_h^T) v_h, then wo
    wq, w_dkv, w_uk, w_uv, wo = (t.double().cpu() for t in w)
    cos, sin = rope.cos.double().cpu(), rope.sin.double().cpu()
    def rot(t, pos):   # NeoX pairs (x[j], x[j + 32]) at position pos
        a, b_ = t[..., :32], t[..., 32:]
        return torch.cat([a * cos[pos] - b_ * sin[pos], b_ * cos[pos] + a * sin[pos]], -1)
    x_all = torch.cat([x.double().cpu() for x in xs], 1)   # (B, 2T, E): the two steps are four causal positions
    q = (x_all @ wq).view(B, 2 * T, H, dn + 64)
    ckv = x_all @ w_dkv
    want = torch.zeros(B, 2 * T, E, dtype=torch.float64)
    for b in range(B):
        for i in range(2 * T):
            k_pe = torch.stack([rot(ckv[b, j, DV:], j) for j in range(i + 1)])
            heads = []
            for h in range(H):
                k_h = torch.cat([ckv[b, :i + 1, :DV] @ w_uk[h].T, k_pe], -1)
                q_h = torch.cat([q[b, i, h, :dn], rot(q[b, i, h, dn:], i)])
                p = torch.softmax((dn + 64) ** -0.5 * k_h @ q_h, 0)
                heads.append(p @ (ckv[b, :i + 1, :DV] @ w_uv[h]))
            want[b, i] = torch.cat(heads) @ wo
    want = want.view(B, 2, T, E).transpose(0, 1)
    err_ref = (run(fp64_middle) - want).abs().max().item()   # the bf16 projections' own error, measured against the reference
    err = (run(None) - want).abs().max().item()
    print(f"model: kernel {err:.3e}, fp64 middle {err_ref:.3e}")
    assert err <= 3 * err_ref
