"""The model layer behind a prefix (modules_transformer.attention_stack_packed_prefix) on the GPU: 2 layers, E = 128, 4 heads, 2 kv
heads, fp32, three sequences with prefixes of 0, 37 and 130 rows.  Each layer's prefix k and v are the keys and values that
attention_stack_packed projects for the prefix tokens when it runs over the FULL sequences, so the stack behind the prefixes must
return that run's suffix rows; prefix_k.grad is held to torch autograd through a dense fp64 implementation of the same function.
Both within 1e-4 relative to the compared quantity's max-abs (fp32: the projections run in the input dtype on the GPU, and the
attention calls sit inside the project's 1e-4 envelope)."""
import math

import numpy as np
import pytest

from gpu_util import rand_u
from test_gpu_bidir import _i32, _torch
from test_gpu_decode_append import _stack
from test_varlen_cpu import pack

pytestmark = pytest.mark.gpu

E, H, HKV, L = 128, 4, 2, 2
D = E // H
PREFIX, SUFFIX = (0, 37, 130), (50, 33, 70)
REL = 1e-4


def _rows(cu, part, other, first):
    """Row indices, in the packing of the full sequences, of every sequence's prefix rows (first) or suffix rows."""
    return np.concatenate([np.arange(s, s + p) if first else np.arange(s + p, s + p + n) for s, p, n in zip(cu[:-1], part, other)]).astype(np.int64)


def _dense_prefix_stack(x, cu, prefixes, cup, layers):
    """fp64 torch on the CPU: x <- x + MHA_l(x) where the tokens of sequence b attend its prefix rows and, causally, its own tokens."""
    torch = _torch()
    G = H // HKV
    for (pk, pv), (wq, wk, wv, wo) in zip(prefixes, layers):
        q, k, v = (x @ wq).view(-1, H, D), (x @ wk).view(-1, HKV, D), (x @ wv).view(-1, HKV, D)
        o = torch.zeros_like(q)
        for b in range(len(cu) - 1):
            s, e, ps, pe = int(cu[b]), int(cu[b + 1]), int(cup[b]), int(cup[b + 1])
            kk, vv = (torch.cat((p[ps:pe], t[s:e])).repeat_interleave(G, dim=1) for p, t in ((pk, k), (pv, v)))
            sc = torch.einsum("ihd,jhd->hij", q[s:e], kk) / math.sqrt(D)
            admit = torch.arange(kk.shape[0])[None, :] <= torch.arange(e - s)[:, None] + (pe - ps)
            p = torch.softmax(sc.masked_fill(~admit, float("-inf")), dim=-1)
            o = o.index_put((torch.arange(s, e),), torch.einsum("hij,jhd->ihd", p, vv))
        x = x + o.reshape(-1, E) @ wo
    return x


def test_the_stack_behind_prefixes_returns_the_full_runs_suffix_rows_and_the_dense_gradient_of_the_prefix():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    full = [p + n for p, n in zip(PREFIX, SUFFIX)]
    cu_full, T_full = pack(full)
    (cu, T), (cup, Tp) = pack(SUFFIX), pack(PREFIX)
    x3, layers = _stack(np.random.default_rng(41), "f32", 1, E, H, HKV, L, T_full)
    x_full = x3[0].contiguous()
    pre, suf = (torch.from_numpy(_rows(cu_full, *a)).cuda() for a in ((PREFIX, SUFFIX, True), (PREFIX, SUFFIX, False)))
    assert len(pre) == Tp == 167 and len(suf) == T == 153

    # the full run, layer by layer (attention_stack_packed's loop), keeping what every layer projects for the prefix tokens
    prefixes, xl = [], x_full
    for (wq, wk, wv, wo) in layers:
        prefixes.append(tuple((xl @ w).view(T_full, HKV, D)[pre].contiguous().requires_grad_() for w in (wk, wv)))
        xl = xl + mt.multi_head_attention_packed(xl, _i32(cu_full), wq, wk, wv, wo, H)
    want = mt.attention_stack_packed(x_full, _i32(cu_full), layers, H)
    assert torch.equal(want, xl)

    x = x_full[suf].contiguous()
    y = mt.attention_stack_packed_prefix(x, _i32(cu), prefixes, _i32(cup), layers, H)
    assert y.shape == (T, E) and y.dtype == x.dtype
    err, scale = float((y.detach() - want[suf]).abs().max()), float(want[suf].abs().max())
    print("output", err, scale)
    assert err < REL * scale, (err, scale)

    dy = torch.from_numpy(rand_u(np.random.default_rng(42), (T, E))).cuda()
    y.backward(dy)
    r_prefixes = [tuple(t.detach().double().cpu().requires_grad_() for t in pkv) for pkv in prefixes]
    r_layers = [tuple(w.double().cpu() for w in layer) for layer in layers]
    ry = _dense_prefix_stack(x.double().cpu(), cu, r_prefixes, cup, r_layers)
    assert float((y.detach().double().cpu() - ry.detach()).abs().max()) < REL * float(ry.detach().abs().max())
    ry.backward(dy.double().cpu())
    for li, ((pk, pv), (rk, rv)) in enumerate(zip(prefixes, r_prefixes)):
        for name, got, ref in (("prefix_k", pk.grad, rk.grad), ("prefix_v", pv.grad, rv.grad)):
            assert got is not None and got.shape == (Tp, HKV, D)
            err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
            print(name, li, err, scale)
            assert scale > 0 and err < REL * scale, (name, li, err, scale)
