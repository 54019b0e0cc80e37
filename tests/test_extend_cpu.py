"""CPU-side checks of the extend entry points (fa_mi355x_*extend* of include/flash_attn_mi355x_decode.h: any number of new queries
against a KV cache): exported and bound symbols, argument validation before any HIP call on fake pointers, Nq beyond the decode
call's 128 passing validation, the split policy (pure, sizing the workspace, with the split counts the shapes of
tests/test_gpu_extend.py rely on), the Python layer's checks and the model layer's calls.  The fp64 reference of the GPU tests is
decode_reference of tests/test_decode_cpu.py, which takes any Nq."""
import ctypes

import pytest

from test_decode_cpu import _declared, built  # noqa: F401  (built: the module-scoped build fixture)

EXTEND_SYMBOLS = {"fa_mi355x_extend_splits", "fa_mi355x_extend_workspace_bytes", "fa_mi355x_fwd_extend", "fa_mi355x_extend_append",
                  "fa_mi355x_fwd_extend_append"}


def test_extend_symbols_are_declared_exported_and_bound(built):
    declared = {s for s in _declared() if "extend" in s}
    assert declared == EXTEND_SYMBOLS
    lib = built.decode()
    for s in declared:
        assert hasattr(lib, s), s
        assert s in built.DECODE_ABI


# one valid call (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, k_new=_ONE, v_new=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, lens=_ONE, ws=_ONE, B=1, H=2, Hkv=2, Nq=160, Ncap=2048,
             d_new=64, d=64, layout=1, scale=0.0, causal=1, dtype=1)
BAD_ARG, BAD_D = 1, 2
_BAD = [
    (dict(q=0), BAD_ARG, "null"), (dict(k=0), BAD_ARG, "null"), (dict(v=0), BAD_ARG, "null"), (dict(out=0), BAD_ARG, "null"),
    (dict(B=0), BAD_ARG, "positive"), (dict(H=-1, Hkv=-1), BAD_ARG, "positive"), (dict(Nq=0), BAD_ARG, "positive"),
    (dict(Ncap=0), BAD_ARG, "positive"), (dict(d=0), BAD_ARG, "positive"), (dict(Hkv=0), BAD_ARG, "Hkv"),
    (dict(H=8, Hkv=3), BAD_ARG, "Hkv = 3"),
    (dict(layout=2), BAD_ARG, "layout"), (dict(dtype=5), BAD_ARG, "dtype"),
    (dict(d=48, d_new=48), BAD_D, "32, 64, 128"), (dict(d=256, d_new=256), BAD_D, "32, 64, 128"),
    (dict(scale=-1.0), BAD_ARG, "softmax_scale"), (dict(scale=float("nan")), BAD_ARG, "softmax_scale"),
    (dict(scale=float("inf")), BAD_ARG, "softmax_scale"),
    (dict(ws=0), BAD_ARG, "fa_mi355x_extend_workspace_bytes"),
    (dict(Ncap=1 << 24), BAD_ARG, "2 GiB"),                      # the cache: 2^24 rows of 2 heads of 64 bf16
    (dict(Nq=1 << 23), BAD_ARG, "2 GiB"),                        # q: 2^23 rows of 2 heads of 64 bf16
    (dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25"),   # G * Nq = 2^25 rows of one kv head
]
_BAD_APPEND = [
    (dict(k_new=0), BAD_ARG, "null"), (dict(v_new=0), BAD_ARG, "null"),
    (dict(d_new=0), BAD_ARG, "d_new = 0"), (dict(d_new=-3), BAD_ARG, "d_new = -3"), (dict(d_new=65), BAD_ARG, "d_new = 65"),
    (dict(d=128, d_new=129), BAD_ARG, "d_new = 129"),
]


def _ids(table):
    return [",".join(f"{k}={v}" for k, v in o.items()) for o, _, _ in table]


def _vp(x):
    return ctypes.c_void_p(x)


def _fwd(lib, **over):
    a = dict(_GOOD, **over)
    return lib.fa_mi355x_fwd_extend(_vp(a["q"]), _vp(a["k"]), _vp(a["v"]), _vp(a["out"]), _vp(a["lse"]), _vp(a["lens"]), _vp(a["ws"]), a["B"],
                                    a["H"], a["Hkv"], a["Nq"], a["Ncap"], a["d"], a["layout"], a["scale"], a["causal"], a["dtype"], None)


def _append(lib, **over):
    a = dict(_GOOD, **over)
    return lib.fa_mi355x_extend_append(_vp(a["k_new"]), _vp(a["v_new"]), _vp(a["k"]), _vp(a["v"]), _vp(a["lens"]), a["B"], a["Hkv"], a["Nq"],
                                       a["Ncap"], a["d_new"], a["d"], a["layout"], a["dtype"], None)


def _fused(lib, **over):
    a = dict(_GOOD, **over)
    return lib.fa_mi355x_fwd_extend_append(_vp(a["q"]), _vp(a["k_new"]), _vp(a["v_new"]), _vp(a["k"]), _vp(a["v"]), _vp(a["out"]),
                                           _vp(a["lse"]), _vp(a["lens"]), _vp(a["ws"]), a["B"], a["H"], a["Hkv"], a["Nq"], a["Ncap"],
                                           a["d_new"], a["d"], a["layout"], a["scale"], a["causal"], a["dtype"], None)


@pytest.mark.parametrize("over,code,msg", _BAD, ids=_ids(_BAD))
def test_extend_rejects_each_bad_argument_before_any_hip_call(built, over, code, msg):
    lib = built.decode()
    assert lib.fa_mi355x_extend_splits(1, 2, 2, 160, 2048, 64, 1) > 1   # (so the null workspace case needs one)
    for call in (_fwd, _fused):
        assert call(lib, **over) == code
        err = lib.fa_mi355x_decode_last_error().decode()
        assert err and msg in err, err


@pytest.mark.parametrize("over,code,msg", _BAD_APPEND, ids=_ids(_BAD_APPEND))
def test_extend_append_rejects_each_bad_argument_before_any_hip_call(built, over, code, msg):
    lib = built.decode()
    for call in (_append, _fused):
        assert call(lib, **over) == code
        err = lib.fa_mi355x_decode_last_error().decode()
        assert err and msg in err, err


_BAD_APPEND_OWN = [
    (dict(k=0), BAD_ARG, "null"), (dict(v=0), BAD_ARG, "null"), (dict(B=0), BAD_ARG, "positive"), (dict(Hkv=-1), BAD_ARG, "positive"),
    (dict(Nq=0), BAD_ARG, "positive"), (dict(Ncap=0), BAD_ARG, "positive"), (dict(d=0), BAD_ARG, "positive"),
    (dict(layout=2), BAD_ARG, "layout"), (dict(dtype=5), BAD_ARG, "dtype"), (dict(d=48, d_new=48), BAD_D, "32, 64, 128"),
    (dict(B=1 << 30, Nq=128, Hkv=64), BAD_ARG, "too many"),
]


@pytest.mark.parametrize("over,code,msg", _BAD_APPEND_OWN, ids=_ids(_BAD_APPEND_OWN))
def test_extend_append_keeps_the_decode_appends_own_checks(built, over, code, msg):
    lib = built.decode()
    assert _append(lib, **over) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    assert err and msg in err, err


def test_extend_row_and_grid_bounds(built):
    """G * Nq at 2^25 (the range over which the kernels' row -> query map is exact) and launches whose workgroup counts do not fit an
    unsigned int are refused by the size arithmetic alone.  (No call here passes every check: with a device present a launch on the
    fake pointers would fault, so a bound is shown to PASS by the message of a later check that fails.)"""
    lib = built.decode()
    rows = dict(H=1 << 12, Hkv=1, Nq=1 << 13, Ncap=1 << 26, d=32, d_new=32)
    assert _fwd(lib, **rows) == BAD_ARG and "2^25" in lib.fa_mi355x_decode_last_error().decode()
    # one query less, G * Nq = 2^25 - 2^12: the row check passes, and the next one (the cache's 2 GiB) answers
    assert _fwd(lib, **dict(rows, Nq=(1 << 13) - 1)) == BAD_ARG and "2 GiB" in lib.fa_mi355x_decode_last_error().decode()
    # B * H * Nq = 2^32 workgroups of a combine launch (no other bound in the way: one batch element of q holds 2^17 rows)
    big = dict(B=1 << 15, H=1, Hkv=1, Nq=1 << 17, Ncap=2048, d=32, d_new=32)
    for call in (_fwd, _fused):
        assert call(lib, **big) == BAD_ARG and "unsigned int" in lib.fa_mi355x_decode_last_error().decode()


@pytest.mark.parametrize("Nq", [129, 5000])
def test_nq_beyond_128_passes_validation_and_the_decode_entry_points_keep_their_limit(built, Nq):
    """The extend entry points take Nq = 129 and 5000 past their Nq check: the answer comes from a check BEHIND it (the null workspace
    of a several-split call, d_new out of range), never about Nq.  (A call that passes every check would launch on the fake pointers.)
    The decode entry points answer the same Nq as they did."""
    lib = built.decode()
    assert lib.fa_mi355x_extend_splits(1, 2, 2, Nq, 2048, 64, 1) > 1
    for call in (_fwd, _fused):
        assert call(lib, Nq=Nq, ws=0) == BAD_ARG
        err = lib.fa_mi355x_decode_last_error().decode()
        assert "workspace" in err and "Nq" not in err, err
    for call in (_append, _fused):
        assert call(lib, Nq=Nq, d_new=65) == BAD_ARG
        err = lib.fa_mi355x_decode_last_error().decode()
        assert "d_new = 65" in err and "Nq" not in err, err
    a = _GOOD
    rc = lib.fa_mi355x_fwd_decode_gqa(_vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), a["B"], a["H"], a["Hkv"],
                                      Nq, a["Ncap"], a["d"], a["layout"], a["scale"], a["causal"], a["dtype"], None)
    assert rc == BAD_ARG and "fa_mi355x_fwd_layout" in lib.fa_mi355x_decode_last_error().decode()
    rc = lib.fa_mi355x_decode_append(_vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), a["B"], a["Hkv"], Nq, a["Ncap"], a["d_new"],
                                     a["d"], a["layout"], a["dtype"], None)
    assert rc == BAD_ARG and "128" in lib.fa_mi355x_decode_last_error().decode()
    rc = lib.fa_mi355x_fwd_decode_append(_vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE), _vp(_ONE),
                                         a["B"], a["H"], a["Hkv"], Nq, a["Ncap"], a["d_new"], a["d"], a["layout"], a["scale"], a["causal"],
                                         a["dtype"], None)
    assert rc == BAD_ARG and "fa_mi355x_fwd_layout" in lib.fa_mi355x_decode_last_error().decode()


def test_extend_optional_pointers_are_not_required(built):
    lib = built.decode()
    # lse and cache_seqlens may be NULL, and a one-split call needs no workspace (not called: it would reach the launch)
    assert lib.fa_mi355x_extend_splits(1, 2, 2, 300, 256, 64, 1) == 1 and lib.fa_mi355x_extend_workspace_bytes(1, 2, 2, 300, 256, 64) == 0


def _policy(B, H, Hkv, Nq, Ncap):
    """The policy as the header states it: B * Hkv * ceil(G * Nq / 128) groups, 512 workgroups wanted, chunks a multiple of 256."""
    groups = B * Hkv * -(-(H // Hkv) * Nq // 128)
    want = max(1, -(-512 // groups))
    chunk = max(256, -(-(-(-Ncap // want)) // 256) * 256)
    return -(-Ncap // chunk)


# (B, H, Hkv, Nq, Ncap, d)
_SHAPES = [(1, 2, 2, 160, 2048, 64), (1, 2, 2, 160, 256, 64), (8, 32, 8, 2048, 8192 + 2048, 128), (8, 32, 32, 256, 4096 + 256, 128),
           (1, 8, 1, 1, 65536, 128), (2, 3, 3, 33, 300, 32), (4, 8, 2, 129, 520, 32), (1, 1, 1, 5000, 5000, 64), (64, 32, 8, 512, 4608, 128),
           (1, 1, 1, 1, 1, 32), (2, 4, 4, 257, 1300, 64)]


def test_extend_split_policy_is_pure_and_sizes_the_workspace(built):
    lib = built.decode()
    seen = set()
    for B, H, Hkv, Nq, Ncap, d in _SHAPES:
        ns = [lib.fa_mi355x_extend_splits(B, H, Hkv, Nq, Ncap, d, dt) for dt in (0, 1, 1)]
        ws = [lib.fa_mi355x_extend_workspace_bytes(B, H, Hkv, Nq, Ncap, d) for _ in range(2)]
        assert ns[0] == ns[1] == ns[2] == _policy(B, H, Hkv, Nq, Ncap) >= 1, (B, H, Hkv, Nq, Ncap)
        assert ws[0] == ws[1] == (0 if ns[0] == 1 else B * H * ns[0] * Nq * (d + 2) * 4), (B, H, Hkv, Nq, Ncap, d, ns[0], ws[0])
        assert ns[0] == 1 or Ncap / ns[0] >= 128   # at least 256 keys per chunk; the chunks cover Ncap
        seen.add(ns[0] > 1)
    assert seen == {True, False}
    assert all(lib.fa_mi355x_extend_splits(1, 2, 2, nq, 256, 64, 1) == 1 for nq in (1, 129, 100000))   # Ncap <= 256: one split
    assert lib.fa_mi355x_extend_splits(0, 2, 2, 160, 2048, 64, 1) == 0
    assert lib.fa_mi355x_extend_splits(1, 8, 3, 160, 2048, 64, 1) == 0
    assert lib.fa_mi355x_extend_workspace_bytes(1, 2, 2, 0, 2048, 64) == 0


# the shapes of tests/test_gpu_extend.py whose path depends on the policy: (B, H, Hkv, Nq, Ncap, d) -> splits
GPU_SPLITS = [((1, 2, 2, 160, 2048, 64), 8),         # several splits of 256 keys: two row blocks, the second one partial
              ((1, 2, 2, 160, 2048, 128), 8),
              ((1, 8, 2, 129, 1300, 64), 6),         # grouped, several splits, the last chunk short
              ((4, 128, 128, 300, 700, 32), 1),      # 1536 workgroups without splitting: one chunk of six super tiles
              ((8, 2, 2, 200, 520, 64), 3),          # the per-batch lengths shape (Ncap = 520): chunks of 256 keys
              ((8, 2, 2, 1, 520, 64), 3),
              ((2, 2, 2, 257, 257, 64), 2),          # len = Nq = Ncap against the square causal forward
              ((2, 4, 4, 200, 1000, 64), 4)]         # graph capture and repeatability


def test_extend_split_counts_that_the_gpu_tests_rely_on(built):
    lib = built.decode()
    for (B, H, Hkv, Nq, Ncap, d), ns in GPU_SPLITS:
        for dt in (0, 1):
            assert lib.fa_mi355x_extend_splits(B, H, Hkv, Nq, Ncap, d, dt) == ns, (B, H, Hkv, Nq, Ncap, d)
        assert lib.fa_mi355x_extend_workspace_bytes(B, H, Hkv, Nq, Ncap, d) == (0 if ns == 1 else B * H * ns * Nq * (d + 2) * 4)


def test_flash_attn_extend_python_checks(built):
    """The checks of test_flash_attn_decode_python_checks and of the k_new / v_new checks of tests/test_decode_append_cpu.py, on
    flash_attn_extend with more than 128 queries."""
    import torch
    from flash_attention_minitorch_amd import device_ops

    q = torch.zeros(2, 200, 4, 64)
    kc = torch.zeros(2, 256, 4, 64)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.flash_attn_extend(q, kc, kc.clone())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.flash_attn_extend(q, kc.bfloat16(), kc.bfloat16())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.flash_attn_extend(q.double(), kc.double(), kc.double())
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="cache_seqlens"):
            device_ops.flash_attn_extend(q, kc, kc.clone(), cache_seqlens=bad)
    with pytest.raises(ValueError, match=r"\(B, H\)"):
        device_ops.flash_attn_extend(q, torch.zeros(2, 256, 8, 64), torch.zeros(2, 256, 8, 64))
    with pytest.raises(ValueError, match="layout"):
        device_ops.flash_attn_extend(q, kc, kc.clone(), layout="nbhd")
    with pytest.raises(ValueError, match="row length"):
        device_ops.flash_attn_extend(torch.zeros(2, 200, 4, 80), kc, kc.clone())
    kn = torch.zeros(2, 200, 4, 48)
    call = lambda k_new, v_new, **kw: device_ops.flash_attn_extend(q, kc, kc.clone(), k_new=k_new, v_new=v_new, **kw)
    for a, b in ((kn, None), (None, kn)):
        with pytest.raises(ValueError, match="together"):
            call(a, b)
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        call(torch.zeros(2, 200, 2, 48), torch.zeros(2, 200, 2, 48))
    with pytest.raises(TypeError, match="dtype"):
        call(kn, kn.bfloat16())
    with pytest.raises(ValueError, match="head dim"):
        call(torch.zeros(2, 200, 4, 65), torch.zeros(2, 200, 4, 65))
    with pytest.raises(ValueError, match="new tokens"):
        call(torch.zeros(2, 199, 4, 48), torch.zeros(2, 199, 4, 48))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(2, 200, 4, 96)[..., :48], kn)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        call(kn, kn.clone())


def test_extend_append_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    kc, vc = torch.zeros(2, 256, 2, 64), torch.zeros(2, 256, 2, 64)
    kn = torch.zeros(2, 200, 2, 48)
    with pytest.raises(ValueError, match="layout"):
        device_ops.extend_append(kn, kn, kc, vc, layout="nbhd")
    with pytest.raises(ValueError, match="one shape"):
        device_ops.extend_append(kn, kn, kc, torch.zeros(2, 128, 2, 64))
    with pytest.raises(TypeError, match="dtype"):
        device_ops.extend_append(kn, kn, kc, vc.bfloat16())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.extend_append(kn.double(), kn.double(), kc.double(), vc.double())
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        device_ops.extend_append(kn, kn, torch.zeros(2, 256, 4, 64), torch.zeros(2, 256, 4, 64))
    with pytest.raises(ValueError, match="head dim"):
        device_ops.extend_append(torch.zeros(2, 200, 2, 80), torch.zeros(2, 200, 2, 80), kc, vc)
    with pytest.raises(ValueError, match="cache_seqlens"):
        device_ops.extend_append(kn, kn, kc, vc, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        device_ops.extend_append(kn, kn, torch.zeros(2, 256, 2, 128)[..., :64], torch.zeros(2, 256, 2, 128)[..., :64])
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.extend_append(kn, kn.clone(), kc, vc, torch.zeros(2, dtype=torch.int32))


def test_model_extend_calls_under_the_recorder(monkeypatch):
    """The C calls of the model layer under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): above 128 tokens
    attention_stack_extend makes one fa_mi355x_fwd_extend_append call per layer on the cache's own (grouped) heads with its own
    workspace query; at or below 128 it is attention_stack_step_fused; chunked prefill resets the lengths and feeds the pieces."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, T, H, Hkv, d, cap = 2, 16, 200, 4, 2, 48, 512
    g = torch.Generator().manual_seed(0)
    x, xt = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((B, P, H * d), (B, T, H * d)))
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    mt.attention_stack_prefill(x, layers, H, cache)
    rec.reset({})
    y = mt.attention_stack_extend(xt, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    sizes = [c for c in rec.calls if "workspace_bytes" in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_append(") for c in calls), calls
    # ... B, H, Hkv, Nq, Ncap, d_new, d, layout, scale, causal, dtype, stream
    assert all(c.endswith(f",{B},{H},{Hkv},{T},{cap},48,64,1,{48 ** -0.5!r},1,1,null)") for c in calls), calls
    assert sizes and all(c.startswith("fa_mi355x_extend_workspace_bytes(") for c in sizes), sizes
    assert y.shape == (B, T, H * d) and cache.length_bound == P + T and cache.lengths.tolist() == [P + T] * B
    rec.reset({})
    mt.attention_stack_extend(xt[:, :5].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_decode_append(") for c in calls), calls
    assert cache.length_bound == P + T + 5
    with pytest.raises(ValueError, match="capacity"):
        mt.attention_stack_extend(torch.zeros(B, cap - P - T - 4, H * d, dtype=torch.bfloat16), layers, H, cache)
    rec.reset({})
    y = mt.attention_stack_prefill_chunked(torch.cat([x, xt], 1), layers, H, cache, 130)   # pieces of 130 and 86 tokens
    calls = [c.split("(")[0] for c in rec.calls if "workspace_bytes" not in c]
    assert calls == ["fa_mi355x_fwd_extend_append"] * 2 + ["fa_mi355x_fwd_decode_append"] * 2, calls
    assert y.shape == (B, P + T, H * d) and cache.length_bound == P + T and cache.lengths.tolist() == [P + T] * B
    with pytest.raises(ValueError, match="capacity"):
        mt.attention_stack_prefill_chunked(torch.zeros(B, cap + 1, H * d, dtype=torch.bfloat16), layers, H, cache, 130)
