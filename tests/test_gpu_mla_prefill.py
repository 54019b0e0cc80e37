"""MLA prefill on the GPU (csrc/fa_mla_prefill.h): flash_attn_mla_prefill against the fp64 reference of tests/test_mla_prefill_cpu.py
on its three packed batches (inputs U(-1, 1), scale 192^-1/2; 1e-3 max-abs on out and lse), the bit-for-bit laws, and one model case,
mla_attention_prefill followed by an absorbed step, against un-absorbed fp64 attention."""
import pytest
import torch

from test_gpu_decode import TOL
from test_mla_prefill_cpu import CASES, expected, inputs, reference

pytestmark = pytest.mark.gpu


def attend(q, k_nope, k_pe, v, cu_q, cu_k):
    from flash_attention_minitorch_amd import device_ops as ops
    out, lse = ops.flash_attn_mla_prefill(q.cuda(), k_nope, k_pe.cuda(), v, cu_q.cuda(), None if cu_k is None else cu_k.cuda())
    return out.cpu(), lse.cpu()


def packed(case, H, views=True):
    """The batch's call: k_nope and v as the two views of the (Tk, H, 256) buffer, or as contiguous copies; A passes one array."""
    q, kv, k_pe, cu_q, cu_k = inputs(case, H)
    k_nope, v = kv.cuda()[..., :128], kv.cuda()[..., 128:]
    return attend(q, *((k_nope, k_pe, v) if views else (k_nope.contiguous(), k_pe, v.contiguous())), cu_q, None if case == "A" else cu_k)


@pytest.mark.parametrize("case,H", [("A", 2), ("B", 2), ("C", 2), ("B", 5)])
def test_prefill_matches_the_fp64_reference(case, H):
    (out, lse), (rout, rlse, live) = packed(case, H), expected(case, H)
    eo, el = (out.double() - rout).abs().max().item(), (lse.double() - rlse).abs().max().item()
    print(f"max-abs out {eo:.2e} lse {el:.2e}")
    assert eo <= TOL["bf16"] and el <= TOL["bf16"], (eo, el)
    assert not out[~live].any() and not lse[:, ~live].any()   # exact zeros: rows without a key, rows no sequence owns


def test_views_of_one_buffer_give_the_bits_of_contiguous_copies():
    a, b = packed("B", 2), packed("B", 2, views=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_sequence_alone_gives_its_rows_of_the_packed_call_and_the_call_repeats():
    q, kv, k_pe, cu_q, cu_k = inputs("B", 2)
    both, again = packed("B", 2), packed("B", 2)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    (sq, eq), (sk, ek) = cu_q[2:4].tolist(), cu_k[2:4].tolist()
    z = lambda n: torch.tensor([0, n], dtype=torch.int32)
    out, lse = attend(q[sq:eq], kv[sk:ek, :, :128].contiguous().cuda(), k_pe[sk:ek], kv[sk:ek, :, 128:].contiguous().cuda(), z(eq - sq), z(ek - sk))
    assert torch.equal(out, both[0][sq:eq]) and torch.equal(lse, both[1][:, sq:eq])


def test_model_prefill_then_a_step_match_unabsorbed_fp64_attention(monkeypatch):
    from flash_attention_minitorch_amd import device_ops as ops, modules_transformer as mt
    from test_mla_cpu import reference as decode_reference
    B, E, H, dn, dv, P, T, dev = 2, 64, 2, 128, 128, 130, 2, "cuda"
    N = P + T
    g = torch.Generator().manual_seed(3)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / s[-2] ** 0.5).to(torch.bfloat16).to(dev)
    w = mt.MLAWeights(u(E, H * (dn + 64)), u(E, 576), u(H, dn, 512), u(H, 512, dv), u(H * dv, E))
    rope = mt.Rotary.table(256, 64, device=dev)
    x_all = (torch.rand(B, N, E, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)

    def run(prefill, decode):
        """The prompt, then one step, through a fresh cache with the two in the place of the kernel calls; both outputs, fp64."""
        cache = mt.LatentKVCache(1, B, 256, dev)
        with monkeypatch.context() as m:
            if prefill:
                m.setattr(ops, "flash_attn_mla_prefill", prefill)
                m.setattr(ops, "flash_attn_decode_mla", decode)
            cache.advance(P)
            y0 = mt.mla_attention_prefill(x_all[:, :P], cache, 0, w, H, rope)
            cache.advance(T)
            return torch.cat([y0, mt.mla_attention_step(x_all[:, P:], cache, 0, w, H, rope)], 1).double().cpu()

    def fp64_prefill(q, k_nope, k_pe, v, cu_q, cu_k=None, softmax_scale=None):
        out, lse, _ = reference(q.cpu(), k_nope.cpu(), k_pe.cpu(), v.cpu(), cu_q.cpu(), cu_q.cpu())
        return out.float().to(dev), lse.float().to(dev)

    def fp64_decode(q, kv_cache, lens, scale, causal, kv_new, table, workspace=None):
        for b, n in enumerate(lens.tolist()):
            kv_cache[b, n - T:n] = kv_new[b]
        out, lse = decode_reference(q.cpu(), kv_cache.cpu(), lens.tolist(), scale, causal)
        return out.float().to(dev), lse.float().to(dev)

    # the un-absorbed definition in fp64 over all N positions: k_h = [c W_UK[h]^T | rope(k_pe)], v_h = c W_UV[h], causal softmax, wo
    wq, w_dkv, w_uk, w_uv, wo = (t.double().cpu() for t in w)
    cos, sin = rope.cos.double().cpu()[:N], rope.sin.double().cpu()[:N]
    def rot(t, c, s):   # NeoX pairs (x[j], x[j + 32]) at each row's position
        a, b_ = t[..., :32], t[..., 32:]
        return torch.cat([a * c - b_ * s, b_ * c + a * s], -1)
    xd = x_all.double().cpu()
    q, ckv = (xd @ wq).view(B, N, H, dn + 64), xd @ w_dkv
    k_pe, causal = rot(ckv[..., 512:], cos, sin), torch.ones(N, N).tril().bool()
    heads = []
    for h in range(H):
        q_h = torch.cat([q[:, :, h, :dn], rot(q[:, :, h, dn:], cos, sin)], -1)
        k_h = torch.cat([ckv[..., :512] @ w_uk[h].T, k_pe], -1)
        p = torch.softmax((192 ** -0.5 * q_h @ k_h.transpose(1, 2)).masked_fill(~causal, float("-inf")), -1)
        heads.append(p @ (ckv[..., :512] @ w_uv[h]))
    want = torch.cat(heads, -1) @ wo
    err_ref = (run(fp64_prefill, fp64_decode) - want).abs().max().item()   # the bf16 projections' own error, measured against the reference
    err = (run(None, None) - want).abs().max().item()
    print(f"model: kernel {err:.3e}, fp64 middle {err_ref:.3e}")
    assert err <= 3 * err_ref
