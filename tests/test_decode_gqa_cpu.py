"""CPU-side checks of grouped-query (GQA / MQA) decode, the *_gqa entry points of include/flash_attn_mi355x_decode.h: exported symbols,
the split policy and workspace for Hkv <= H, argument validation before any HIP call (the new arguments, and the ungrouped table of
tests/test_decode_cpu.py through the grouped entry point), and the Python layer's shape checks and cache allocation."""
import ctypes

import pytest

from test_decode_cpu import _BAD, _GOOD, _SHAPES, _declared, built  # noqa: F401  (built: the module-scoped build fixture)

GQA_SYMBOLS = {"fa_mi355x_fwd_decode_gqa", "fa_mi355x_decode_workspace_bytes_gqa", "fa_mi355x_decode_splits_gqa"}


def test_gqa_symbols_are_declared_and_exported(built):
    assert GQA_SYMBOLS <= set(_declared())
    lib = built.decode()
    for s in GQA_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in built.DECODE_ABI


def _divisors(h):
    return [k for k in range(1, h + 1) if h % k == 0]


def test_gqa_policy_with_all_heads_is_the_ungrouped_policy(built):
    lib = built.decode()
    for B, H, Nq, Ncap, d in _SHAPES:
        for dt in (0, 1):
            assert lib.fa_mi355x_decode_splits_gqa(B, H, H, Nq, Ncap, d, dt) == lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, dt)
        assert lib.fa_mi355x_decode_workspace_bytes_gqa(B, H, H, Nq, Ncap, d) == lib.fa_mi355x_decode_workspace_bytes(B, H, Nq, Ncap, d)


def test_gqa_policy_is_pure_and_sizes_the_workspace_by_query_heads(built):
    lib = built.decode()
    seen = set()
    for B, H, Nq, Ncap, d in _SHAPES:
        for Hkv in _divisors(H)[:-1]:
            ns = [lib.fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, dt) for dt in (0, 1, 1)]
            ws = [lib.fa_mi355x_decode_workspace_bytes_gqa(B, H, Hkv, Nq, Ncap, d) for _ in range(2)]
            assert ns[0] == ns[1] == ns[2] >= 1 and ws[0] == ws[1]
            ns = ns[0]
            seen.add(ns > 1)
            # chunks of at least 256 keys (a multiple of 256) that cover Ncap: the last split starts below Ncap
            assert ns == 1 or (ns - 1) * 256 < Ncap
            assert ws[0] == (0 if ns == 1 else B * H * ns * Nq * (d + 2) * 4), (B, H, Hkv, Nq, Ncap, d, ns, ws[0])
            # fewer kv heads never mean fewer splits: the policy counts B * Hkv * ceil(G * Nq / 32) workgroups per split
            assert ns >= lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, 1)
    assert seen == {True, False}
    # 32 query heads on 8 kv heads at B = 32: 256 workgroups per split instead of 1024, so the call splits where the ungrouped one
    # does not
    assert lib.fa_mi355x_decode_splits(32, 32, 1, 4096, 128, 1) == 1
    assert lib.fa_mi355x_decode_splits_gqa(32, 32, 8, 1, 4096, 128, 1) == 4
    assert lib.fa_mi355x_decode_splits_gqa(32, 32, 1, 1, 4096, 128, 1) == 16
    # G * Nq rows fill blocks of 32: 8 heads x 4 queries are one block, 8 x 5 are two
    assert lib.fa_mi355x_decode_splits_gqa(64, 8, 1, 4, 4096, 64, 1) == 16
    assert lib.fa_mi355x_decode_splits_gqa(64, 8, 1, 5, 4096, 64, 1) == 8
    for bad in ((0, 8, 2), (2, 8, 0), (2, 8, -1), (2, 8, 3), (2, 2, 4)):
        assert lib.fa_mi355x_decode_splits_gqa(bad[0], bad[1], bad[2], 1, 65536, 128, 1) == 0
        assert lib.fa_mi355x_decode_workspace_bytes_gqa(bad[0], bad[1], bad[2], 1, 65536, 128) == 0


def _call(lib, **over):
    a = dict(_GOOD, Hkv=_GOOD["H"])
    a.update(over)
    if "H" in over and "Hkv" not in over:   # the ungrouped table's cases: Hkv follows H
        a["Hkv"] = a["H"]
    vp = ctypes.c_void_p
    return lib.fa_mi355x_fwd_decode_gqa(vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["out"]), vp(a["lse"]), vp(a["lens"]), vp(a["ws"]), a["B"],
                                        a["H"], a["Hkv"], a["Nq"], a["Ncap"], a["d"], a["layout"], a["scale"], a["causal"], a["dtype"],
                                        None)


_BAD_GQA = [
    (dict(Hkv=0), 1, ("Hkv", "positive")), (dict(Hkv=-2), 1, ("Hkv", "positive")),
    (dict(H=8, Hkv=3), 1, ("H = 8", "Hkv = 3")), (dict(H=2, Hkv=4), 1, ("H = 2", "Hkv = 4")),
    # the 2 GiB bound is the cache's: 2^21 rows of bf16 d = 64 pass with one kv head and fail with sixteen
    (dict(H=16, Hkv=16, Ncap=1 << 21), 1, ("2 GiB",)),
    (dict(H=16, Hkv=1, Ncap=1 << 21, ws=0), 1, ("workspace",)),
]


@pytest.mark.parametrize("over,code,msgs", _BAD_GQA, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _, _ in _BAD_GQA])
def test_gqa_rejects_each_new_bad_argument_before_any_hip_call(built, over, code, msgs):
    lib = built.decode()
    assert _call(lib, **over) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    for m in msgs:
        assert m in err, err


@pytest.mark.parametrize("field,value,code,msg", _BAD, ids=[f"{f}={v}" for f, v, _, _ in _BAD])
def test_gqa_entry_point_answers_the_ungrouped_table_alike(built, field, value, code, msg):
    lib = built.decode()
    for over in ({field: value}, {field: value, "H": 4, "Hkv": 2} if field != "H" else {field: value, "Hkv": 1}):
        assert _call(lib, **over) == code, over
        err = lib.fa_mi355x_decode_last_error().decode()
        assert err and msg in err, (over, err)


def test_flash_attn_decode_accepts_a_grouped_cache_and_rejects_heads_that_do_not_divide(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q = torch.zeros(2, 1, 4, 64)
    for hkv in (2, 1):
        kc = torch.zeros(2, 256, hkv, 64)
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):   # past every shape check: the tensors are not on a GPU
            device_ops.flash_attn_decode(q, kc, kc.clone())
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.flash_attn_decode(q.transpose(1, 2).contiguous(), torch.zeros(2, 2, 256, 64), torch.zeros(2, 2, 256, 64), layout="bhnd")
    for shape in ((2, 256, 3, 64), (2, 256, 8, 64), (3, 256, 2, 64)):
        with pytest.raises(ValueError, match=r"\(B, H\)"):
            device_ops.flash_attn_decode(q, torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match=r"\(B, H\)"):
        device_ops.decode_workspace(q, torch.zeros(2, 256, 3, 64))
    # the workspace of a grouped call is the library's answer for (H, Hkv)
    q8 = torch.zeros(1, 1, 8, 128)
    ws = device_ops.decode_workspace(q8, torch.zeros(1, 65536, 2, 128))
    assert ws is not None and ws.numel() * 4 == built.decode().fa_mi355x_decode_workspace_bytes_gqa(1, 8, 2, 1, 65536, 128) > 0


def test_kv_cache_allocates_kv_heads_only():
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt

    cache = mt.KVCache(3, 2, 64, 8, 48, torch.bfloat16, "cpu", n_kv_head=2)
    assert len(cache.k) == len(cache.v) == 3
    assert all(t.shape == (2, 64, 2, 64) and t.dtype == torch.bfloat16 for t in cache.k + cache.v)
    assert cache.n_head == 8 and cache.n_kv_head == 2
    assert mt.KVCache(1, 2, 64, 8, 32, torch.float32, "cpu").k[0].shape == (2, 64, 8, 32)
    with pytest.raises(ValueError, match="n_kv_head"):
        mt.KVCache(1, 2, 64, 8, 32, torch.float32, "cpu", n_kv_head=3)


def test_grouped_projection_and_expansion_shapes():
    """wk, wv of shape (E, Hkv * d) project Hkv heads; the expansion repeats each kv head for its G query heads in head order."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt

    g = torch.Generator().manual_seed(0)
    B, N, E, H, Hkv = 2, 5, 64, 8, 2
    d = E // H
    x, wq = torch.randn(B, N, E, generator=g), torch.randn(E, E, generator=g)
    wk, wv = torch.randn(E, Hkv * d, generator=g), torch.randn(E, Hkv * d, generator=g)
    q, k, v = mt._project(x, wq, wk, wv, H)
    assert q.shape == (B, N, H, d) and k.shape == v.shape == (B, N, Hkv, d)
    ke = mt._expand_kv(k, H)
    assert ke.shape == (B, N, H, d) and torch.equal(ke, k.repeat_interleave(H // Hkv, dim=2))
    assert mt._expand_kv(q, H) is q
    with pytest.raises(ValueError, match="Hkv"):
        mt._project(x, wq, torch.randn(E, 3 * d), torch.randn(E, 3 * d), H)
