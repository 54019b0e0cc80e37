"""FP8 index keys of the lightning indexer without a GPU (include/flash_attn_mi355x_mla_indexer_fp8.h): the 144-byte row restated in
torch, the inputs of tests/test_gpu_mla_indexer_fp8.py and how sharp they are, the C ABI, the refusals, the kernels' registers."""
import functools
import re

import numpy as np
import pytest
import torch

import test_mla_indexer_cpu as bf16
from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_mla_cpu import BAD_ARG, SEED
from test_mla_indexer_cpu import DI, FUSED, HEADS, LENS, NCAP, index_inputs, index_scores_reference, topk_reference

HEADER, ROW, E4M3 = "flash_attn_mi355x_mla_indexer_fp8.h", 144, torch.float8_e4m3fn


def quantise_idx(rows):
    """bf16 (..., 128) -> uint8 (..., 144), the header's append: a = max |x| of the row (NaN ignored, inf counts), s = 2^(e - 9) if
    m <= 0.875 else 2^(e - 8) for a = m 2^e, clamped to [2^-100, 2^120]; rne_e4m3(clamp(x / s, -448, 448)), NaN -> 0x7F; s; 12 zeros."""
    x = rows.float()
    a = torch.where(x.isnan(), 0.0, x.abs()).amax(-1, keepdim=True)
    m, e = torch.frexp(a)
    e = torch.where(a == 0, -100, torch.where(a.isinf(), 120, torch.where(m <= 0.875, e - 9, e - 8))).clamp(-100, 120)
    s = torch.ldexp(torch.ones_like(a), e)
    codes = (x * (1.0 / s)).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
    codes[x.isnan()] = 0x7F
    return torch.cat([codes, s.contiguous().view(torch.uint8), torch.zeros(*rows.shape[:-1], 12, dtype=torch.uint8)], -1)


def dequantise_idx(cache, key_scale=True):
    """uint8 (..., 144) -> bf16 (..., 128): s * e4m3(code_c), exact in bf16 (key_scale=False: the codes' values alone)."""
    s = cache[..., DI:DI + 4].contiguous().view(torch.float32) if key_scale else 1.0
    return (cache[..., :DI].contiguous().view(E4M3).float() * s).to(torch.bfloat16)


def edge_rows():
    """kidx_new (2, 3, 128), U(-1, 1) with: (0, 1) all zeros; (0, 2) a maximum of exactly 448 * 2^3; (1, 0) one bf16 ulp above that
    (3600); (1, 1) a NaN; (1, 2) an infinity.  (0, 0) stays plain: the append test gives it a row below 0."""
    k = index_inputs(SEED + 1, 2, 3, 1, 1)[2]
    k[0, 1] = 0
    k[0, 2, 2], k[1, 0, 7], k[1, 1, 5], k[1, 2, 9] = -3584.0, 3600.0, float("nan"), float("-inf")
    return k


def fp8_inputs(seed, B, Ncap, HI, Nq):
    """index_inputs with every key row under a gain of {1, 1/2, 1/4} (rows carry different scales), quantised: (q_idx, weights, bytes)."""
    q, w, k = index_inputs(seed, B, Ncap, HI, Nq)
    gain = torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (B, Ncap, 1), generator=torch.Generator().manual_seed(seed + 100))]
    return q, w, quantise_idx((k.float() * gain).to(torch.bfloat16))


def quantised_reference(q, w, cache, lens, causal, **kw):
    """index_scores_reference on what the kernel multiplies: q_idx through the format row by row, the keys dequantised."""
    return index_scores_reference(dequantise_idx(quantise_idx(q)), w, dequantise_idx(cache, **kw), lens, causal)


@functools.lru_cache(maxsize=None)
def score_case(HI, Nq, lens, causal):
    """(q_idx, weights, cache bytes, (score, bound)) of a GPU case, computed once and shared."""
    q, w, kb = fp8_inputs(SEED, 2, NCAP, HI, Nq)
    return q, w, kb, quantised_reference(q, w, kb, lens, causal)


def test_the_restated_format_on_the_edge_rows():
    k = edge_rows()
    b = quantise_idx(k)
    s = b[..., DI:DI + 4].contiguous().view(torch.float32)[..., 0]
    assert b.shape == (2, 3, ROW) and not b[..., DI + 4:].any() and torch.equal(torch.frexp(s)[0], torch.full_like(s, 0.5))
    assert s[0, 1] == 2.0 ** -100 and not b[0, 1, :DI].any()
    assert s[0, 2] == 8.0 and b[0, 2, 2] == 0xFE and s[1, 0] == 16.0 and b[1, 0, 7] == 0x76   # -448 exactly; 3600 / 16 = 225 -> 224
    assert b[1, 1, 5] == 0x7F and s[1, 1] < 1 and s[1, 2] == 2.0 ** 120 and b[1, 2, 9] == 0xFE
    assert (dequantise_idx(b[0, 0]).float() - k[0, 0].float()).abs().max() <= 2.0 ** -8 * 16   # half an e4m3 step at the row's scale


@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("HI,Nq", HEADS)
def test_the_score_cases_see_the_quantisation_and_the_key_scale(HI, Nq, lens):
    """Somewhere in every case the reference moves by 10 x the bound when q_idx skips the format (the keys still dequantised: less of
    a change than both operands unquantised) and when the key's scale is ignored."""
    q, w, kb, (ref, bound) = score_case(HI, Nq, lens, False)
    ok = ~torch.isneginf(ref)
    for other in (index_scores_reference(q, w, dequantise_idx(kb), lens, False)[0], quantised_reference(q, w, kb, lens, False, key_scale=False)[0]):
        assert ((other - ref).abs()[ok] / bound[ok]).max() >= 10


def test_the_fused_case_is_sharp_on_the_quantised_operands():
    """test_mla_indexer_cpu's band condition: |score - t| <= 2 x bound holds at most 1 % of a row's admitted entries."""
    HI, Nq, lens, topk = FUSED
    score, bound = score_case(HI, Nq, lens, True)[3]
    lists = topk_reference(score, lens, topk)
    for b, i in np.ndindex(2, Nq):
        row = score[b, i][~torch.isneginf(score[b, i])]
        if row.numel() > topk:
            kth = lists[b, i].long()[score[b, i][lists[b, i].long()].argmin()]
            assert ((row - score[b, i, kth]).abs() <= 2 * bound[b, i, kth]).sum().item() <= 0.01 * row.numel()


def test_fp8_indexer_abi_matches_the_header_and_the_kernels_run_without_scratch(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos, twins, lib = _prototypes(HEADER), _prototypes(bf16.HEADER), built.mla()
    assert sorted(protos) == sorted(built.MLA_INDEXER_FP8_ABI) and not set(protos) & (set(built.MLA_INDEXER_ABI) | set(built.MLA_FP8_ABI))
    for s, (res, args) in built.MLA_INDEXER_FP8_ABI.items():
        assert ([_ctypes_kind(x) for x in args], _ctypes_kind(res)) == (protos[s][1], protos[s][0]) and protos[s] == twins[s[:-4]], s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    kernels = _device_kernels(built.lib_path(built.MLA_NAME))
    names = " ".join(k[0] for k in kernels)
    assert names.count("mla_index_scores_fp8_kernel") == 2 and "mla_index_append_fp8_kernel" in names
    assert all(scratch == 0 and vgpr <= 512 for _, scratch, vgpr in kernels), kernels


# ---- refusals, before any HIP call: the bf16 list, with the 2 GiB bound at 144 bytes per row ----
_BAD = [(o, m) for o, m in bf16._BAD if m != "2 GiB"] + [(dict(Ncap=1 << 24), "2 GiB")]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_fp8_indexer_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(bf16._GOOD, **over), built.mla()
    rc = lib.fa_mi355x_mla_indexer_fp8(*[a[n] or None for n in ("q", "w", "new", "kidx", "scores", "idx", "lens", "table")],
                                       *[a[n] for n in ("B", "HI", "Nq", "topk", "Ncap", "num_pages", "page_size", "max_pages", "causal")], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


def test_python_checks_name_the_fp8_index_cache_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops, modules_transformer as mt
    monkeypatch.setattr(_lib, "mla", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.uint8: torch.zeros(*shape, dtype=dtype)
    lens, q, w, new = z(2, dtype=torch.int32), z(2, 1, 4, DI, dtype=torch.bfloat16), z(2, 1, 4, dtype=torch.float32), z(2, 1, DI, dtype=torch.bfloat16)
    for cache, msg in [(z(2, 256, DI), "kidx_cache must be (B, Ncap, 144)"), (z(2, 256, 132).view(E4M3), "kidx_cache must be"),
                       (z(256, ROW), "rows of 144 bytes"), (z(3, 256, ROW), "with B = 2"), (z(2, 512, ROW)[:, ::2], "kidx_cache must be contiguous")]:
        for call in (lambda: ops.mla_indexer(q, w, cache, lens, 64), lambda: ops.mla_index_scores(q, w, cache, lens),
                     lambda: ops.mla_index_append(new, cache, lens)):
            with pytest.raises(ValueError, match=re.escape(msg)):
                call()
    with pytest.raises(ValueError, match="kidx_new must be"):   # kidx_new stays bf16 rows of 128
        ops.mla_indexer(q, w, z(2, 256, ROW), lens, 64, kidx_new=z(2, 1, ROW, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="index_keys must be"):
        mt.LatentKVCache(1, 2, 128, "cpu", index_keys="fp4")
    c = mt.LatentKVCache(1, 2, 128, "cpu", page_size=128, index_keys="fp8")
    assert c.kidx[0].dtype is torch.uint8 and c.kidx[0].shape == (2, 128, ROW) and c.kv[0].dtype is torch.bfloat16
